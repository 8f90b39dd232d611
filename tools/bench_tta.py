#!/usr/bin/env python
"""Dev tool: what the flip test (TEST.AUG.FLIP, modeling/test_time_augmentation.py) costs.  Not part of the product or of the
tests.

Eval step (the engine's call: base kernel / input copy, graph replay, post-processing; device events around --step-reps calls
after --step-warm; a replayed step is in its steady state after 20 steps) for every --configs x --precisions:
    plain  B     the plain engine at batch B
    flip   B     the flip-test engine at batch B (the network runs on 2B images, one decode of B merged maps)
    plain 2B     the plain engine at batch 2B: the same network work, two decodes' worth of selection
The decode alone (200 warm + 1000 timed launches, --warm / --reps: single kernels need the long warm-up) on
trained-like maps (background on the clamp floor) of --decode-shape:
    decode plain B / decode flip B (reads 2B maps) / decode plain 2B
and, as the separate-merge alternative the fused form replaces, a torch merge of the 2B maps followed by decode plain B.
The legs alternate over --rounds, so that a drift of the machine shows as spread inside a leg.

  --multi-scale  instead of the above, multi-scale testing (TEST.SOFT_NMS):
                 the merge alone (ops.soft_nms_merge) at B = --batch, --ms-passes passes of 100 clustered candidates, with 80
                 classes and with 1 class (the deepest sequential chain): per call in a back-to-back stream, and its device time
                 from a captured graph of 10 merges;
                 the multi-size step of CenterNetWithTTA on raw device records (--ms-sizes, wall clock around whole calls, one
                 host synchronisation each) against the single-size steps at the same sizes, alternating in the same run.

  --lib PATH     the plain legs (plain B, plain 2B, decode plain B / 2B) once more in a child process that loads another
                 build of libctdet_hip.so (a parent commit's: it needs none of the new entry points): the plain path of this
                 build against the parent's, and the parent's own run-to-run spread"""
import argparse
import ctypes
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--configs", default="dla34,r50")
ap.add_argument("--precisions", default="f16x3,f16,f32")
ap.add_argument("--step-warm", type=int, default=20)
ap.add_argument("--step-reps", type=int, default=100)
ap.add_argument("--warm", type=int, default=200)
ap.add_argument("--reps", type=int, default=1000)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--decode-shape", default="128,128,80", help="H,W,C of the decode-alone legs (batch: --batch)")
ap.add_argument("--no-steps", action="store_true")
ap.add_argument("--no-decode", action="store_true")
ap.add_argument("--multi-scale", action="store_true")
ap.add_argument("--ms-sizes", default="384,512,640")
ap.add_argument("--ms-passes", type=int, default=5)
ap.add_argument("--ms-warm", type=int, default=5)
ap.add_argument("--ms-reps", type=int, default=20)
ap.add_argument("--lib", default=None)
ap.add_argument("--plain-only", action="store_true", help="(the --lib child) the legs every ABI-8 build can run")
a = ap.parse_args()

from detectron2_centernet_amd import _lib  # noqa: E402

TAG = ""
if a.plain_only and a.lib:
    # another build's library under this tree's Python: bind what it has (the plain path calls nothing newer)
    have = ctypes.CDLL(a.lib)
    for name in [n for n in _lib.SIGNATURES if not hasattr(have, n)]:
        del _lib.SIGNATURES[name]
    _lib.LIB_PATH = a.lib
    TAG = f" [{os.path.basename(os.path.dirname(os.path.dirname(a.lib))) or a.lib}]"

import bench  # noqa: E402
from detectron2_centernet_amd import ops  # noqa: E402
from detectron2_centernet_amd.structures import ImageList  # noqa: E402

dev = torch.device("cuda:0")


def timed(f, warm, reps):
    for _ in range(warm):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps      # ms


def step_legs(config, precision):
    model, cfg = bench.build_model(precision, dev, seed=1, config=config)
    model.eval()
    B, S = a.batch, a.size
    imgs = {n: bench.synthetic_images(n, S, 0, dev) for n in (B, 2 * B)}
    Hp, Wp = ImageList.padded_size([(S, S)], model.size_divisibility)
    legs = [("plain  B", B, False), ("flip   B", B, True), ("plain 2B", 2 * B, False)]
    if a.plain_only:
        legs = [l for l in legs if not l[2]]
    engines = {}
    with torch.no_grad():
        for name, n, flip in legs:
            eng = model._engine(n, S, S, Hp, Wp, torch.uint8, flip) if flip else model._engine(n, S, S, Hp, Wp, torch.uint8)
            eng.img_params.copy_(torch.tensor([[1.0, 1.0, S, S]] * n))
            engines[name] = (eng, imgs[n])
        for r in range(a.rounds):
            for name, n, flip in legs:
                eng, x = engines[name]
                ms = timed(lambda: eng(x), a.step_warm, a.step_reps)
                print(f"round {r}  step {config:5s} {precision:5s} {name} (B={a.batch}, {S}x{S}){TAG}: {ms:8.3f} ms", flush=True)


def decode_legs():
    H, W, C = [int(v) for v in a.decode_shape.split(",")]
    B, K = a.batch, 100
    g = torch.Generator().manual_seed(0)

    def maps(n):      # a trained network's map: background on the clamp floor, a few hundred blobs per image
        logits = torch.full((n, H, W, C), -12.0)
        idx = torch.randint(0, n * H * W * C, (300 * n,), generator=g)
        logits.view(-1)[idx] = torch.randn(300 * n, generator=g) * 3.0
        hm = torch.clamp(torch.sigmoid(logits), 1e-4, 1 - 1e-4).to(dev)
        return hm, (torch.rand(n, H, W, 2, generator=g) * 20).to(dev), torch.rand(n, H, W, 2, generator=g).to(dev)
    m1, m2 = maps(B), maps(2 * B)
    ws1, ws2 = ops.DecodeWorkspace(B, H, W, C, K, dev), ops.DecodeWorkspace(2 * B, H, W, C, K, dev)
    floor = ops.SIGMOID_CLAMP_FLOOR
    mb = B * H * W * C * 4 / 1e6

    def merged():
        hm, wh, reg = m2
        return ops.decode((hm[:B] + hm[B:].flip(2)) * 0.5, (wh[:B] + wh[B:].flip(2)) * 0.5, reg[:B], K, 4.0, workspace=ws1,
                          heat_floor=floor)
    legs = [("decode plain  B", lambda: ops.decode(*m1, K, 4.0, workspace=ws1, heat_floor=floor), mb),
            ("decode plain 2B", lambda: ops.decode(*m2, K, 4.0, workspace=ws2, heat_floor=floor), 2 * mb)]
    if not a.plain_only:
        legs.insert(1, ("decode flip   B", lambda: ops.decode(*m2, K, 4.0, workspace=ws1, heat_floor=floor, flip=True), 2 * mb))
        legs.append(("torch merge + decode plain B", merged, 0.0))
    for r in range(a.rounds):
        for name, f, mbytes in legs:
            us = timed(f, a.warm, a.reps) * 1e3
            rate = f"  heat bytes read {mbytes:7.1f} MB -> {mbytes / us:5.2f} TB/s" if mbytes else ""
            print(f"round {r}  {name:30s} (B={B}, {H}x{W}x{C}){TAG}: {us:9.2f} us{rate}", flush=True)


def merge_inputs(B, npass, C, seed=0):
    """npass passes of 100 detections per image: 25 objects, every pass sees each one four times, jittered"""
    import numpy as np
    g = np.random.default_rng(seed)
    K, nobj = 100, 25
    xy = g.uniform(0, 900, (B, nobj, 2))
    wh = g.uniform(20, 150, (B, nobj, 2))
    cls = g.integers(0, C, (B, nobj))
    base = g.uniform(0.1, 0.95, (B, nobj))
    passes = []
    for _ in range(npass):
        o = np.tile(np.arange(nobj), K // nobj)
        p1 = xy[:, o] + g.normal(0, 0.05, (B, K, 2)) * wh[:, o]
        p2 = p1 + wh[:, o] * (1 + g.normal(0, 0.05, (B, K, 2)))
        sc = base[:, o] * g.uniform(0.3, 1.0, (B, K))
        order = np.argsort(-sc, axis=1)                      # a pass returns its detections best first
        bx = np.take_along_axis(np.concatenate([p1, p2], axis=2), order[:, :, None], axis=1)
        passes.append((torch.from_numpy(bx.astype(np.float32)).to(dev), torch.from_numpy(np.take_along_axis(sc, order, 1).astype(np.float32)).to(dev),
                       torch.from_numpy(np.take_along_axis(cls[:, o], order, 1).astype(np.int32)).to(dev),
                       torch.full((B,), K, dtype=torch.int32, device=dev)))
    return passes


def merge_legs():
    B = a.batch
    legs = []
    for C in (80, 1):
        passes = merge_inputs(B, a.ms_passes, C)

        def f(passes=passes, C=C):
            return ops.soft_nms_merge(passes, C, 0.5, 0.001, 100)
        f()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(10):
                f()
        legs.append((C, f, g))
    for r in range(a.rounds):
        for C, f, g in legs:
            us = timed(f, a.warm, a.reps) * 1e3
            dev_us = timed(g.replay, 20, 100) * 1e2
            print(f"round {r}  soft_nms_merge (B={B}, {a.ms_passes} passes of 100, {C:2d} classes): {us:9.2f} us per call, "
                  f"{dev_us:9.2f} us device time (graph of 10)", flush=True)


def multi_scale_step_legs(config, precision):
    import time

    from detectron2_centernet_amd.modeling import CenterNetWithTTA
    model, cfg = bench.build_model(precision, dev, seed=1, config=config)
    model.eval()
    model.score_threshold = 0.0            # every pass returns its 100 candidates: the merge at its fullest
    model.wh[-1].bias.data.fill_(3.0)      # boxes of non-degenerate size (random-init wh is ~0: every box would be dropped as empty)
    B, S = a.batch, a.size
    sizes = tuple(int(v) for v in a.ms_sizes.split(","))
    imgs = bench.synthetic_images(B, S, 0, dev)
    recs = [{"image_raw": imgs[b].permute(1, 2, 0).contiguous()} for b in range(B)]

    def wrapper(min_sizes, soft_nms):
        c = cfg.clone()
        c.TEST.AUG.ENABLED, c.TEST.AUG.MIN_SIZES, c.TEST.AUG.FLIP, c.TEST.SOFT_NMS.ENABLED = True, min_sizes, True, soft_nms
        return CenterNetWithTTA(c, model)
    legs = [(f"single {s}", wrapper((s,), False)) for s in sizes] + [(f"multi {sizes}", wrapper(sizes, True))]

    def wall(t):
        for _ in range(a.ms_warm):
            t(recs)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.ms_reps):
            t(recs)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.ms_reps * 1e3
    with torch.no_grad():
        for r in range(a.rounds):
            row = [wall(t) for _, t in legs]
            for (name, _), ms in zip(legs, row):
                print(f"round {r}  step {config:5s} {precision:5s} flip {name} (B={B}, raw {S}x{S}): {ms:8.3f} ms", flush=True)
            print(f"round {r}  step {config:5s} {precision:5s} multi - sum of singles: {row[-1] - sum(row[:-1]):+8.3f} ms "
                  f"(sum {sum(row[:-1]):8.3f} ms)", flush=True)


def main():
    if a.multi_scale:
        print(f"merge legs: {a.warm} warm + {a.reps} timed calls; step legs: {a.ms_warm} warm + {a.ms_reps} timed calls (wall clock); "
              f"{a.rounds} rounds", flush=True)
        merge_legs()
        if not a.no_steps:
            for config in a.configs.split(","):
                for precision in a.precisions.split(","):
                    multi_scale_step_legs(config, precision)
        return
    if not a.plain_only:
        print(f"step legs: {a.step_warm} warm + {a.step_reps} timed steps; decode legs: {a.warm} warm + {a.reps} timed launches; "
              f"{a.rounds} rounds", flush=True)
    if not a.no_steps:
        for config in a.configs.split(","):
            for precision in a.precisions.split(","):
                step_legs(config, precision)
    if not a.no_decode:
        decode_legs()
    if a.lib and not a.plain_only:
        argv = [sys.executable, os.path.abspath(__file__), "--plain-only"] + [v for v in sys.argv[1:]]
        sys.stdout.flush()
        subprocess.check_call(argv)      # a fresh process: one library per process


main()
