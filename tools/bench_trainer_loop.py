#!/usr/bin/env python
"""What the training loop costs on top of the step: images/s of

  a  DefaultTrainer.train() with the default hooks (writer period 20, no periodic checkpoint, no periodic evaluation),
     same-size host-mapped record batches fed from memory -- routed to the captured step, metrics through the device ring
  b  the same with CTDET_METRICS_SYNC=1: the reference's per-step read-back and gather instead of the ring
  d  a with the records' images already on the device: what is left of the gap to c is not the batch's host-to-device copy
  c  a bare `run_step_tensors` loop on a device-resident batch: the step alone.  `--root DIR` takes package and library from
     another checkout (the parent commit's), which is the number to hold against

DLA-34, batch 16 at 512^2 of the synthetic set, `--steps` timed iterations after `--warmup`.  Every configuration runs in a
fresh child process; `c` runs `--repeat-c` times to show its run-to-run noise.  Prints one JSON line with all figures.

    python tools/bench_trainer_loop.py [--precision f16x3] [--steps 200] [--warmup 50] [--root PARENT_CHECKOUT]"""
import argparse
import itertools
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def records(batch, size, n_batches):
    from detectron2_centernet_amd.data.catalog import synthetic_sample
    from detectron2_centernet_amd.structures import Boxes, Instances
    out = []
    for j in range(n_batches):
        recs = []
        for b in range(batch):
            s = synthetic_sample(j * batch + b, size=size)
            inst = Instances((size, size))
            inst.gt_boxes, inst.gt_classes = Boxes(s["boxes"]), s["classes"]
            recs.append({"image": s["image"], "instances": inst, "height": size, "width": size})
        out.append(recs)
    return out


def run_trainer(args):
    """configurations a, b (the switch is in the environment) and d"""
    import torch

    import bench
    from detectron2_centernet_amd.engine import DefaultTrainer, hooks
    dev = torch.device("cuda:0")
    batches = records(args.batch, args.size, 4)
    if args.one == "d":
        for recs in batches:
            for r in recs:
                r["image"] = r["image"].to(dev)
    clock = {}
    model, cfg = bench.build_model(args.precision, dev, seed=1, calibrate=False)

    class Trainer(DefaultTrainer):
        @classmethod
        def build_model(cls, cfg):
            return model

        @classmethod
        def build_train_loader(cls, cfg):
            return itertools.cycle(batches)

        @classmethod
        def test(cls, cfg, model, evaluators=None):      # the evaluation after the last iteration is outside the clock
            return {}

    def tick(trainer):
        # the clock starts behind iteration warmup - 1 and stops behind the last but one: the final iteration's checkpoint
        # and evaluation are not part of the loop's cost
        if trainer.iter in (args.warmup - 1, trainer.max_iter - 2):
            torch.cuda.synchronize()
            clock[trainer.iter] = time.perf_counter()

    cfg.SOLVER.IMS_PER_BATCH = args.batch
    cfg.SOLVER.MAX_ITER = args.warmup + args.steps + 1
    cfg.SOLVER.CHECKPOINT_PERIOD = 0
    cfg.TEST.EVAL_PERIOD = 0
    cfg.OUTPUT_DIR = tempfile.mkdtemp(prefix="ctdet_loop_")
    trainer = Trainer(cfg)
    trainer.register_hooks([hooks.CallbackHook(after_step=tick)])
    trainer.train()
    t0, t1 = clock[args.warmup - 1], clock[trainer.max_iter - 2]
    return {"images_per_s": args.steps * args.batch / (t1 - t0), "ms_per_step": (t1 - t0) / args.steps * 1e3,
            "graph_state": trainer.graph_state, "flushes": trainer.metric_ring.flushes,
            "metrics_sync": trainer.metric_ring.sync_mode}


def run_bare(args):
    """configuration c; uses only what the parent commit has"""
    import torch

    import bench
    from detectron2_centernet_amd.engine.bench_train import synthetic_batch
    from detectron2_centernet_amd.engine.train_loop import SimpleTrainer
    dev = torch.device("cuda:0")
    model, cfg = bench.build_model(args.precision, dev, seed=1, calibrate=False)
    cfg.SOLVER.IMS_PER_BATCH = args.batch
    trainer = SimpleTrainer(model, None, cfg)
    batch = synthetic_batch(args.batch, args.size, 0, dev)
    for _ in range(args.warmup):
        trainer.run_step_tensors(*batch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        trainer.run_step_tensors(*batch)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    return {"images_per_s": args.steps * args.batch / (t1 - t0), "ms_per_step": (t1 - t0) / args.steps * 1e3,
            "graph_state": trainer.graph_state}


def child(args, which, root=None, env=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--one", which, "--precision", args.precision, "--steps", str(args.steps),
           "--warmup", str(args.warmup), "--batch", str(args.batch), "--size", str(args.size)]
    if root:
        cmd += ["--root", root]
    done = subprocess.run(cmd, env=dict(os.environ, **(env or {})), capture_output=True, text=True, timeout=args.timeout)
    if done.returncode != 0:
        raise RuntimeError(f"configuration {which} failed:\n{done.stdout[-2000:]}\n{done.stderr[-4000:]}")
    return json.loads([l for l in done.stdout.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--repeat-c", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=600, help="seconds a configuration's child process may take")
    ap.add_argument("--root", default=None, help="checkout whose package and library configuration c uses (default: this one)")
    ap.add_argument("--one", choices=["a", "b", "c", "d"], default=None, help="(internal) run one configuration in this process")
    args = ap.parse_args()
    if args.one:
        root = os.path.abspath(args.root) if args.root and args.one == "c" else HERE
        sys.path.insert(0, root)
        os.chdir(root)
        print(json.dumps((run_bare if args.one == "c" else run_trainer)(args)), flush=True)
        return
    out = {"precision": args.precision, "batch": args.batch, "size": args.size, "steps": args.steps, "warmup": args.warmup,
           "c_root": os.path.abspath(args.root) if args.root else HERE}
    out["c"] = [child(args, "c", root=args.root) for _ in range(args.repeat_c)]
    out["a"] = child(args, "a", env={"CTDET_METRICS_SYNC": "0"})
    out["b"] = child(args, "b", env={"CTDET_METRICS_SYNC": "1"})
    out["d"] = child(args, "d", env={"CTDET_METRICS_SYNC": "0"})
    cs = [r["images_per_s"] for r in out["c"]]
    out["summary"] = {"a_images_per_s": out["a"]["images_per_s"], "b_images_per_s": out["b"]["images_per_s"],
                      "c_images_per_s_mean": sum(cs) / len(cs), "c_noise_images_per_s": max(cs) - min(cs),
                      "a_minus_c_mean": out["a"]["images_per_s"] - sum(cs) / len(cs),
                      "a_minus_b": out["a"]["images_per_s"] - out["b"]["images_per_s"],
                      "d_images_per_s": out["d"]["images_per_s"],
                      "h2d_ms_per_step": out["a"]["ms_per_step"] - out["d"]["ms_per_step"]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
