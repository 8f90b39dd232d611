#!/usr/bin/env python3
"""The training input on the host against the device (INPUT.DEVICE_AUGMENT): 480x640 JPEGs, MIN_SIZE_TRAIN 512
(-> 512x683), batches of 16.

  mapper    images/s of the dataset mapper -- the host pipeline (decode, Pillow resize, colour jitters), the raw-record mapper
            (decode and the draws only) and the decode alone -- on one thread and through the training DataLoader with 16
            worker processes (best of three windows of `--batches` batches).  host resize + jitter per batch = host batch time - decode-only batch time, both from the
            16-worker run.  Taken BEFORE the GPU is initialised (the workers are forked).
  device    device time (HIP events around `--reps` back-to-back launches, after warm-up) of the three launches of
            CenterNet.stage_raw_train for a batch of 16 device-resident raw images: the resize, the byte sum, the jitter;
            once with all four transforms drawn for every image, once with draws made at the pipeline's own 0.15.
  staging   host clock, synchronised: the 16 host-to-device copies of a host-mapped batch against stage_raw_train of the raw
            batch (pinned staging copy, one upload, the three launches).
  step      the eager training step (SimpleTrainer.run_step, DLA-34, batch 16) on host-mapped records against raw records of
            the same images and draws; host clock, synchronised, three alternating legs of `--steps` steps after `--warmup`.

The condition DESIGN.md 7.9 sets: the three launches together take less time than the 16-worker host mapper spends on resize
plus jitter for the batch.  It is printed as holding or not.

    python tools/bench_train_input.py [--out profiles/NAME.txt] [--modes f16x3,f16] [--no-step]

`--affine` runs the INPUT.AFFINE leg alone: the device time of the warp launch (ops.warp_affine_u8) for a
batch of 16 from 480x640 and from 1080x1920 sources next to the resize launch on the same inputs, and DefaultTrainer images/s
on raw records with INPUT.AFFINE off and on, with the share of steps that replayed a captured graph.  No threshold is set.

    python tools/bench_train_input.py --affine [--out profiles/NAME.txt] [--modes f16x3] [--steps 40] [--warmup 10]

Needs a GPU: there is no CPU fallback, a time taken without one would mean nothing."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SRC_HW, MIN_SIZE, BATCH, WORKERS, N_IMAGES = (480, 640), 512, 16, 16, 64
DATASET = "bench_train_input_ds"


def write_dataset(root):
    from PIL import Image
    rng = np.random.RandomState(0)
    dicts = []
    for i in range(N_IMAGES):
        base = rng.randint(0, 256, (30, 40, 3)).astype(np.uint8)
        arr = np.asarray(Image.fromarray(base).resize((SRC_HW[1], SRC_HW[0]), Image.BICUBIC))      # smooth: realistic JPEG sizes
        path = os.path.join(root, f"{i}.jpg")
        Image.fromarray(arr).save(path, quality=90)
        anns = [{"bbox": [int(rng.randint(0, 500)), int(rng.randint(0, 380)), 100, 80], "bbox_mode": 1, "category_id": j % 3,
                 "iscrowd": 0} for j in range(8)]
        dicts.append({"file_name": path, "image_id": i, "height": SRC_HW[0], "width": SRC_HW[1], "annotations": anns})
    return dicts


class DecodeOnly:
    """the part of the mapper both pipelines share: read the file, hand the pixels over as a tensor"""

    def __init__(self, cfg):
        self.fmt = cfg.INPUT.FORMAT

    def __call__(self, d):
        import torch
        from detectron2_centernet_amd.data import detection_utils as du
        return {"image_raw": torch.from_numpy(np.require(du.read_image(d["file_name"], format=self.fmt), requirements="CW"))}


def make_cfg(device_augment):
    from detectron2_centernet_amd.config import get_cfg
    cfg = get_cfg()
    cfg.INPUT.MIN_SIZE_TRAIN, cfg.INPUT.MIN_SIZE_TRAIN_SAMPLING, cfg.INPUT.MAX_SIZE_TRAIN = (MIN_SIZE,), "choice", 1333
    cfg.INPUT.DEVICE_AUGMENT = device_augment
    cfg.DATASETS.TRAIN = (DATASET,)
    cfg.SOLVER.IMS_PER_BATCH = BATCH
    return cfg


def mapper_rates(dicts, mapper, cfg, batches):
    """(images/s on one thread, images/s through the DataLoader with WORKERS processes)"""
    from detectron2_centernet_amd.data import build_detection_train_loader
    np.random.seed(0)
    for d in dicts[:4]:
        mapper(d)
    t0 = time.perf_counter()
    for d in dicts:
        mapper(d)
    one = len(dicts) / (time.perf_counter() - t0)
    it = build_detection_train_loader(cfg, mapper=mapper, num_workers=WORKERS)
    for _ in range(2 * WORKERS // BATCH + 4):
        next(it)
    many = 0.0
    for _ in range(3):      # best of three windows: the machine's other tenants show in a single one
        t0 = time.perf_counter()
        for _ in range(batches):
            next(it)
        many = max(many, batches * BATCH / (time.perf_counter() - t0))
    del it
    return one, many


def records(dicts, prob, seed):
    """(raw records, host records) of the first BATCH images from the same seed; prob: the jitter probability (None: 0.15)"""
    from detectron2_centernet_amd.data import TrafficLightDatasetMapper, dataset_mapper
    keep = dataset_mapper._JITTER_PROB
    if prob is not None:
        dataset_mapper._JITTER_PROB = prob
    try:
        out = []
        for augment in (True, False):
            mapper = TrafficLightDatasetMapper(make_cfg(augment), is_train=True)
            np.random.seed(seed)
            out.append([mapper(d) for d in dicts[:BATCH]])
    finally:
        dataset_mapper._JITTER_PROB = keep
    return out


def device_times(torch, ops, dev, raw, host, reps):
    """ms of the resize launch, the sum launch and the jitter launch for the batch; the staged bytes are checked first"""
    srcs = [r["image_raw"].to(dev).permute(2, 0, 1) for r in raw]
    sizes = [tuple(r["resize_hw"]) for r in raw]
    plan = ops.resize_u8_prepare(srcs, sizes)
    images = plan.launch()
    jit = ops.colour_jitter_u8_prepare(images, [r["jitter"] for r in raw])
    jit.launch()
    torch.cuda.synchronize()
    for im, h in zip(images, host):
        assert torch.equal(im.cpu(), h["image"]), "the device pipeline differs from the host pipeline"
    # repeated in place: the same work on other bytes
    out = [launch_ms(torch, fn, reps) for fn in (plan.launch, jit.launch_sum, jit.launch_jitter)]
    return out, jit.n, jit.sums.numel()


def launch_ms(torch, fn, reps):
    """device ms of one call of `fn`: HIP events around `reps` back-to-back calls after 5 warm-up calls, best of three"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(5):
        fn()
    best = None
    for _ in range(3):
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1) / reps
        best = ms if best is None else min(best, ms)
    return best


def staging_times(torch, dev, raw, host, reps=20):
    """host clock, synchronised, ms per batch: what each path does to get its 16 uint8 images onto the device -- the host
    path's 16 copies of resized images, the raw path's pinned staging, one upload and three launches"""
    import bench
    model, _ = bench.build_model("f16", dev, seed=1)
    out = {}
    for name, fn in (("host", lambda: [h["image"].to(dev) for h in host]), ("raw", lambda: model.stage_raw_train(raw))):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
            torch.cuda.synchronize()
        out[name] = (time.perf_counter() - t0) / reps * 1e3
    return out


def step_times(torch, dev, mode, raw, host, steps, warmup):
    import bench
    from detectron2_centernet_amd.engine.train_loop import SimpleTrainer
    model, cfg = bench.build_model(mode, dev, seed=1)
    cfg.SOLVER.IMS_PER_BATCH = BATCH
    model.train()
    tr = SimpleTrainer(model, None, cfg)
    out = {"host": [], "raw": []}
    for _ in range(3):      # the two kinds alternate; every leg is reported
        for name, recs in (("host", host), ("raw", raw)):
            for _ in range(warmup):
                tr.run_step(recs)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.run_step(recs)
            torch.cuda.synchronize()
            out[name].append((time.perf_counter() - t0) / steps)
    return out


# ------------------------------------------------------------------------------------------------ --affine
AFFINE_SOURCES = ((480, 640), (1080, 1920))
AFFINE_LEGS = (("AFFINE off, MIN_SIZE_TRAIN (512,)", False, (MIN_SIZE,)), ("AFFINE off, MIN_SIZE_TRAIN (448, 512, 576)", False, (448, 512, 576)),
               ("AFFINE on, OUTPUT_SIZE (512, 512)", True, (MIN_SIZE,)))


def affine_cfg(affine, sizes=(MIN_SIZE,)):
    cfg = make_cfg(True)
    cfg.INPUT.MIN_SIZE_TRAIN = sizes
    cfg.INPUT.AFFINE.ENABLED = affine
    return cfg


def affine_device_times(torch, ops, dev, reps):
    """per source size: device ms of the warp launch and of the resize launch for BATCH device-resident raw images, the
    warps drawn by the sampler itself (seeded); the warp's bytes are checked against the host reference first"""
    from detectron2_centernet_amd.data import transforms as T
    from detectron2_centernet_amd.data.warp import warp_affine_u8_reference
    crop = T.RandomAffineCrop(affine_cfg(True))
    resize = T.ResizeShortestEdge((MIN_SIZE,), 1333, "choice")
    out = {}
    for h, w in AFFINE_SOURCES:
        rng = np.random.RandomState(h)
        imgs = [rng.randint(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(BATCH)]
        np.random.seed(7)
        tfms = [crop.get_transform(im) for im in imgs]
        srcs = [torch.from_numpy(im).to(dev).permute(2, 0, 1) for im in imgs]
        plan = ops.warp_affine_u8_prepare(srcs, [(t.Minv, t.flip) for t in tfms], (crop.out_h, crop.out_w))
        got = plan.launch()
        for k in (0, BATCH - 1):
            assert np.array_equal(got[k].permute(1, 2, 0).cpu().numpy(), tfms[k].apply_image(imgs[k])), "the device warp differs from the host's"
        new = resize.output_size(h, w, MIN_SIZE, 1333)
        rplan = ops.resize_u8_prepare(srcs, [new] * BATCH)
        out[(h, w)] = (launch_ms(torch, plan.launch, reps), launch_ms(torch, rplan.launch, reps), new, sum(t.flip for t in tfms))
    return out


def affine_trainer_leg(torch, dev, dicts, affine, sizes, mode, steps, warmup):
    """DefaultTrainer.train() on raw records (INPUT.DEVICE_AUGMENT) mapped once by the real mapper and fed from memory:
    images/s (host clock, synchronised) and the share of the timed steps that replayed a captured graph"""
    import itertools

    import bench
    from detectron2_centernet_amd.data import TrafficLightDatasetMapper
    from detectron2_centernet_amd.engine import DefaultTrainer, hooks
    mapper = TrafficLightDatasetMapper(affine_cfg(affine, sizes), is_train=True)
    np.random.seed(3)
    batches = [[mapper(d) for d in dicts[i:i + BATCH]] for i in range(0, N_IMAGES, BATCH)]
    model, cfg = bench.build_model(mode, dev, seed=1, calibrate=False)
    clock, replays = {}, [0]
    real_replay = torch.cuda.CUDAGraph.replay

    def counted(self):
        replays[0] += 1
        return real_replay(self)

    class Trainer(DefaultTrainer):
        @classmethod
        def build_model(cls, cfg):
            return model

        @classmethod
        def build_train_loader(cls, cfg):
            return itertools.cycle(batches)

        @classmethod
        def test(cls, cfg, model, evaluators=None):
            return {}

    def tick(trainer):
        if trainer.iter in (warmup - 1, trainer.max_iter - 2):
            torch.cuda.synchronize()
            clock[trainer.iter] = (time.perf_counter(), replays[0])

    cfg.SOLVER.IMS_PER_BATCH = BATCH
    cfg.SOLVER.MAX_ITER = warmup + steps + 1
    cfg.SOLVER.CHECKPOINT_PERIOD = 0
    cfg.TEST.EVAL_PERIOD = 0
    cfg.OUTPUT_DIR = tempfile.mkdtemp(prefix="ctdet_affine_")
    trainer = Trainer(cfg)
    trainer.register_hooks([hooks.CallbackHook(after_step=tick)])
    torch.cuda.CUDAGraph.replay = counted
    try:
        trainer.train()
    finally:
        torch.cuda.CUDAGraph.replay = real_replay
    (t0, r0), (t1, r1) = clock[warmup - 1], clock[trainer.max_iter - 2]
    return steps * BATCH / (t1 - t0), (r1 - r0) / steps, sorted({tuple(r["resize_hw"]) for b in batches for r in b})


def affine_main(args, say, rec):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_input needs a ROCm GPU: nothing here is measurable without one")
    from detectron2_centernet_amd import ops
    from detectron2_centernet_amd.data import DatasetCatalog
    dev = torch.device("cuda:0")
    say(f"# tools/bench_train_input.py --affine on {torch.cuda.get_device_name(0)}; batch {BATCH}, numpy {np.__version__}")
    say("device time of ONE launch for the batch, device-resident HWC sources (HIP events):")
    for (h, w), (t_warp, t_resize, new, flips) in affine_device_times(torch, ops, dev, args.reps).items():
        rec.update({f"warp_{h}x{w}_us": t_warp * 1e3, f"resize_{h}x{w}_us": t_resize * 1e3})
        say(f"  {h}x{w}: warp to 512x512 ({flips} of {BATCH} flipped) {t_warp * 1e3:.1f} us; resize to {new[0]}x{new[1]} {t_resize * 1e3:.1f} us")
    if not args.no_step:
        with tempfile.TemporaryDirectory(prefix="ctdet_train_input_") as root:
            dicts = write_dataset(root)
            if DATASET not in DatasetCatalog:
                DatasetCatalog.register(DATASET, lambda: dicts)
            say(f"DefaultTrainer.train(), DLA-34, batch {BATCH}, raw records ({SRC_HW[0]}x{SRC_HW[1]} JPEGs) fed from memory, {args.steps} steps "
                f"after {args.warmup} (host clock, synchronised):")
            for mode in [m for m in args.modes.split(",") if m]:
                for name, affine, sizes in AFFINE_LEGS:
                    rate, share, hws = affine_trainer_leg(torch, dev, dicts, affine, sizes, mode, args.steps, args.warmup)
                    key = f"{mode}_{'affine' if affine else 'resize_' + '_'.join(map(str, sizes))}"
                    rec.update({f"trainer_{key}_img_s": rate, f"trainer_{key}_graph_share": share})
                    say(f"  {mode:6s} {name:44s} {rate:7.1f} img/s, {share * 100:5.1f} % of the steps replayed a captured graph; "
                        f"sizes after mapping {hws}")
    say(json.dumps({"bench_train_input_affine": rec}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--affine", action="store_true", help="the INPUT.AFFINE leg alone (DESIGN.md 7.12)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--batches", type=int, default=100)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--modes", default="f16x3,f16")
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    lines, rec = [], {}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if args.affine:
        affine_main(args, say, rec)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    import PIL
    from detectron2_centernet_amd.data import DatasetCatalog, TrafficLightDatasetMapper
    with tempfile.TemporaryDirectory(prefix="ctdet_train_input_") as root:
        dicts = write_dataset(root)
        if DATASET not in DatasetCatalog:
            DatasetCatalog.register(DATASET, lambda: dicts)
        # ---- host side, before the GPU is touched: the loader's workers are forked
        rates = {}
        for name, mapper, cfg in (("host", TrafficLightDatasetMapper(make_cfg(False), True), make_cfg(False)),
                                  ("raw", TrafficLightDatasetMapper(make_cfg(True), True), make_cfg(True)),
                                  ("decode", DecodeOnly(make_cfg(False)), make_cfg(False))):
            rates[name] = mapper_rates(dicts, mapper, cfg, args.batches)
        batches = {"all four on": records(dicts, 1.0, 0), "p = 0.15": records(dicts, None, 0)}

        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench_train_input needs a ROCm GPU: nothing here is measurable without one")
        from detectron2_centernet_amd import ops
        dev = torch.device("cuda:0")
        say(f"# tools/bench_train_input.py on {torch.cuda.get_device_name(0)}; {SRC_HW[0]}x{SRC_HW[1]} JPEGs, MIN_SIZE_TRAIN "
            f"{MIN_SIZE} -> {tuple(batches['p = 0.15'][0][0]['resize_hw'])}, batch {BATCH}, Pillow {PIL.__version__}, numpy {np.__version__}")
        say("mapper, images/s (one thread | DataLoader with %d worker processes):" % WORKERS)
        for name, what in (("host", "host pipeline (decode + resize + jitters)"), ("raw", "raw records (decode + draws)"),
                           ("decode", "decode only")):
            say(f"  {what:44s} {rates[name][0]:8.1f} | {rates[name][1]:8.1f}")
            rec[f"mapper_{name}_1_thread_img_s"], rec[f"mapper_{name}_{WORKERS}_workers_img_s"] = rates[name]
        host_ms = BATCH / rates["host"][1] * 1e3
        decode_ms = BATCH / rates["decode"][1] * 1e3
        host_aug_ms = host_ms - decode_ms
        rec.update(host_batch_ms=host_ms, decode_batch_ms=decode_ms, host_resize_jitter_batch_ms=host_aug_ms)
        say(f"  per batch of {BATCH} with {WORKERS} workers: host pipeline {host_ms:.2f} ms, decode only {decode_ms:.2f} ms -> resize + "
            f"jitter {host_aug_ms:.2f} ms")
        # ---- device side
        say("device time of the three launches for the batch (HIP events):")
        for name, (raw, host) in batches.items():
            (t_resize, t_sum, t_jit), n_desc, n_sums = device_times(torch, ops, dev, raw, host, args.reps)
            total = t_resize + t_sum + t_jit
            holds = total < host_aug_ms
            key = "all_on" if name.startswith("all") else "p015"
            rec.update({f"device_{key}_resize_ms": t_resize, f"device_{key}_sum_ms": t_sum, f"device_{key}_jitter_ms": t_jit,
                        f"device_{key}_total_ms": total, f"condition_{key}_holds": holds})
            say(f"  {name:12s} ({n_desc} images drew a transform, {n_sums} drew contrast): resize {t_resize * 1e3:.1f} us, byte sum "
                f"{t_sum * 1e3:.1f} us, jitter {t_jit * 1e3:.1f} us -> {total * 1e3:.1f} us; host resize + jitter {host_aug_ms:.2f} ms: "
                f"the condition {'HOLDS' if holds else 'DOES NOT HOLD'} ({host_aug_ms / total:.0f}x)")
        raw, host = batches["p = 0.15"]
        stg = staging_times(torch, dev, raw, host)
        rec.update(staging_host_ms=stg["host"], staging_raw_ms=stg["raw"])
        nb_host, nb_raw = sum(h["image"].numel() for h in host), sum(r["image_raw"].numel() for r in raw)
        say(f"getting the batch's images onto the device (host clock, synchronised): host-mapped records, {BATCH} copies of "
            f"{nb_host / 1e6:.1f} MB: {stg['host']:.2f} ms; raw records, stage_raw_train of {nb_raw / 1e6:.1f} MB: {stg['raw']:.2f} ms")
        # ---- the training step
        if not args.no_step:
            say(f"eager training step (SimpleTrainer.run_step, DLA-34, batch {BATCH}; records with the p = 0.15 draws):")
            for mode in [m for m in args.modes.split(",") if m]:
                st = step_times(torch, dev, mode, raw, host, args.steps, args.warmup)
                rec.update({f"step_{mode}_{k}_ms": [t * 1e3 for t in v] for k, v in st.items()})
                legs = {k: " / ".join(f"{t * 1e3:.2f}" for t in v) for k, v in st.items()}
                say(f"  {mode:6s} host-mapped records {legs['host']} ms (best {BATCH / min(st['host']):.0f} img/s), raw records "
                    f"{legs['raw']} ms (best {BATCH / min(st['raw']):.0f} img/s); legs alternate host, raw, host, ...")
        say(json.dumps({"bench_train_input": rec}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
