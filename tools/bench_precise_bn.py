#!/usr/bin/env python
"""Dev tool: what TEST.PRECISE_BN costs on DLA-34 (f16x3, batch 16 at 512^2, 200 batches by default).  Not part of the product
or of the tests; no figure here is a pass mark.  DESIGN.md 7.15 records a run.

  1. the statistics-only forward (train_step.stats_forward_tensors, eager, under no_grad) per batch, next to the eager and
     the captured training step of the same build (a fresh trainer per leg);
  2. the ONE merge launch per batch (ops.precise_bn_merge_ over every covered layer) next to the torch ops of fvcore's recipe,
     two per layer per batch (`mean += (running_mean - mean) / (i + 1)` and the same for the variance), on the same buffers;
     and the finish launch;
  3. the wall time of the whole update_bn_stats over --batches record batches (host-mapped records: the pinned upload, the
     preprocess launches and the target build of `preprocess_image` are inside, as they are in the hook)."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from detectron2_centernet_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batches", type=int, default=200)
ap.add_argument("--batch-size", type=int, default=16)
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--precision", default="f16x3")
ap.add_argument("--steps", type=int, default=40, help="timed training steps per leg")
a = ap.parse_args()
dev = torch.device("cuda:0")


def timed(f, warm, reps):
    """(device ms, wall ms) per call"""
    for _ in range(warm):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, (time.perf_counter() - t0) / reps * 1e3


def records(n, first):
    from detectron2_centernet_amd.data.catalog import synthetic_sample
    from detectron2_centernet_amd.structures import Boxes, Instances
    out = []
    for i in range(n):
        s = synthetic_sample(first + i, size=a.size, max_boxes=32)
        inst = Instances((a.size, a.size))
        inst.gt_boxes, inst.gt_classes = Boxes(s["boxes"]), s["classes"]
        out.append({"image": s["image"], "instances": inst, "height": a.size, "width": a.size})
    return out


def main():
    from detectron2_centernet_amd.engine import train_step
    from detectron2_centernet_amd.engine.bench_train import synthetic_batch
    from detectron2_centernet_amd.engine.precise_bn import get_bn_modules, update_bn_stats
    from detectron2_centernet_amd.engine.train_loop import SimpleTrainer

    B, what = a.batch_size, f"{a.precision} DLA-34, {a.batch_size} x {a.size}^2"
    batch = synthetic_batch(B, a.size, 0, dev)

    # 1. forward legs
    model, cfg = bench.build_model(a.precision, dev, seed=1)
    model.train()
    mods = get_bn_modules(model)
    x = ops.preprocess(batch[0], model._mean_host, model._std_host, a.size, a.size, out_dtype=model._ctx.dtype)

    def stats_forward():
        with torch.no_grad():
            train_step.stats_forward_tensors(model, x)

    d, w = timed(stats_forward, 8, a.steps)
    print(f"{what}: statistics forward, eager        {d:8.3f} ms device  {w:8.3f} ms wall / batch  ({len(mods)} covered layers)",
          flush=True)
    for mode in ("0", "1"):
        os.environ["CTDET_TRAIN_GRAPH"] = mode
        m2, c2 = bench.build_model(a.precision, dev, seed=1)
        m2.train()
        c2.SOLVER.IMS_PER_BATCH = B
        tr = SimpleTrainer(m2, None, c2)
        d, w = timed(lambda: tr.run_step_tensors(*batch), 8, a.steps)
        print(f"{what}: training step, {tr.graph_state:8s}         {d:8.3f} ms device  {w:8.3f} ms wall / step", flush=True)
        del tr, m2
    os.environ.pop("CTDET_TRAIN_GRAPH", None)

    # 2. the merge: one launch against two torch ops per layer
    numels = [m.running_mean.numel() for m in mods]
    starts = [0]
    for n in numels:
        starts.append(starts[-1] + n)
    total = starts[-1]
    mean_ptrs = torch.tensor([m.running_mean.data_ptr() for m in mods], dtype=torch.int64, device=dev)
    var_ptrs = torch.tensor([m.running_var.data_ptr() for m in mods], dtype=torch.int64, device=dev)
    seg_start = torch.tensor(starts, dtype=torch.int64, device=dev)
    state = torch.zeros(3, total, dtype=torch.float64, device=dev)
    rows = [B * a.size * a.size // 4] * len(mods)
    rows_dev = torch.tensor(rows, dtype=torch.int64, device=dev)
    d, w = timed(lambda: ops.precise_bn_merge_(mean_ptrs, var_ptrs, seg_start, rows, max(numels), state, rows_dev=rows_dev),
                 200, 1000)
    print(f"merge, one launch over {len(mods)} layers / {total} channels:   {d * 1e3:8.1f} us device  {w * 1e3:8.1f} us wall / batch")
    slots = state.unsqueeze(0).clone()
    keep = [(m.running_mean.clone(), m.running_var.clone()) for m in mods]
    d, w = timed(lambda: ops.precise_bn_finish_(mean_ptrs, var_ptrs, seg_start, max(numels), slots), 200, 1000)
    print(f"finish, one launch (world 1):                          {d * 1e3:8.1f} us device  {w * 1e3:8.1f} us wall")
    for m, (mean, var) in zip(mods, keep):
        m.running_mean.copy_(mean)
        m.running_var.copy_(var)
    avg_mean, avg_var = [torch.zeros_like(m.running_mean) for m in mods], [torch.zeros_like(m.running_var) for m in mods]

    def fvcore_recipe(i=3):
        for m, am, av in zip(mods, avg_mean, avg_var):
            am += (m.running_mean - am) / (i + 1)
            av += (m.running_var - av) / (i + 1)

    d, w = timed(fvcore_recipe, 20, 100)
    print(f"fvcore's recipe, {2 * len(mods)} running-average updates in torch:   {d * 1e3:8.1f} us device  {w * 1e3:8.1f} us wall / batch")

    # 3. the whole thing
    batches = [records(B, B * i) for i in range(4)]

    def loader():
        i = 0
        while True:
            yield batches[i % len(batches)]
            i += 1

    update_bn_stats(model, loader(), 3)        # warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    update_bn_stats(model, loader(), a.batches)
    torch.cuda.synchronize()
    t = time.perf_counter() - t0
    print(f"{what}: update_bn_stats over {a.batches} record batches: {t:.2f} s wall ({t / a.batches * 1e3:.1f} ms / batch)")


if __name__ == "__main__":
    main()
