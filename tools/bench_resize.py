#!/usr/bin/env python3
"""Device resize against the host resize, for the two cases DESIGN.md 7.8 records: 480x640 -> 512x683 (the workload's own
ratio) and 1080x1920 -> 512x910, 64 images each.

Per case:
  host      Pillow's resize of the 64 images (ResizeTransform.apply_image), single-threaded, and spread over 16 worker
            processes that hold their images already and return nothing: resize compute alone, the host at its best.
            Taken BEFORE the GPU is initialised (the workers are forked).
  kernel    device time of the ONE batched launch (ops.resize_u8_prepare(...).launch(): device-resident HWC sources,
            the engine's CHW staging layout as destination), HIP events around `--reps` back-to-back launches after
            warm-up; the bytes it must move (sources read once, destination written once) over that time as a share of the
            HBM peak.
  call      ops.resize_u8 from 64 HOST images, as the model calls it: pinned staging copy, one upload, one launch; host
            clock around `--reps` calls ending in a synchronise.
  eval      the model's eval step on 64 records, host-resized ("image": resize not in the time) against raw
            ("image_raw": upload and device resize in the time); host clock, synchronised, `--steps` steps after warm-up.

    python tools/bench_resize.py [--out profiles/NAME.txt] [--modes f16x3,f16] [--no-eval]

--affine-test runs another leg alone: evaluation.inference_on_dataset over a set that mixes 480x640, 640x480,
427x640 and 375x500 sources, DLA-34 f16x3, TEST.BATCH_SIZE 16, raw records, once per test input -- ResizeShortestEdge
(MIN_SIZE_TEST 512), INPUT.AFFINE.TEST_MODE fix_res 512x512 and keep_res: images/s and the share of batches that replayed a
captured engine; then the device time of ctdet_postprocess_affine against ctdet_postprocess at B = 64, K = 100.  The three
inputs feed different pixel counts: the images/s are what a user of each setting gets, no like-for-like comparison.

    python tools/bench_resize.py --affine-test [--out profiles/NAME.txt] [--batches 40] [--reps 200]

Needs a GPU: there is no CPU fallback, a time taken without one would mean nothing."""
import argparse
import json
import multiprocessing
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [((480, 640), (512, 683)), ((1080, 1920), (512, 910))]
BATCH = 64
WORKERS = 16
HBM_PEAK_GBS = 8000.0      # MI355X HBM3E peak, the figure bench.py's roofline uses

_worker_images = None


def _images(hw, n, seed=0):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, (hw[0], hw[1], 3), dtype=np.uint8) for _ in range(n)]


def _pil_resize(img, new):
    from detectron2_centernet_amd.data import transforms as T
    return T.ResizeTransform(img.shape[0], img.shape[1], new[0], new[1]).apply_image(img)


def _worker_init(hw, per_worker):
    global _worker_images
    _worker_images = _images(hw, per_worker, seed=os.getpid())


def _worker_run(new):
    s = 0
    for img in _worker_images:
        s += int(_pil_resize(img, new)[0, 0, 0])
    return s


def host_times(hw, new, rounds=5):
    """(single-threaded seconds, 16-worker seconds) per 64-image batch, best of `rounds`"""
    imgs = _images(hw, BATCH)
    _pil_resize(imgs[0], new)
    single = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for img in imgs:
            _pil_resize(img, new)
        single.append(time.perf_counter() - t0)
    pooled = []
    with multiprocessing.get_context("fork").Pool(WORKERS, _worker_init, (hw, BATCH // WORKERS)) as pool:
        pool.map(_worker_run, [new] * WORKERS, chunksize=1)      # warm-up: every worker has run once
        for _ in range(rounds):
            t0 = time.perf_counter()
            pool.map(_worker_run, [new] * WORKERS, chunksize=1)
            pooled.append(time.perf_counter() - t0)
    return min(single), min(pooled)


def kernel_time(ops, torch, dev, hw, new, reps):
    srcs = [torch.from_numpy(a).to(dev) for a in _images(hw, BATCH)]
    stage = torch.zeros(BATCH, 3, new[0], new[1], dtype=torch.uint8, device=dev)
    plan = ops.resize_u8_prepare([s.permute(2, 0, 1) for s in srcs], [new] * BATCH, outs=[stage[b] for b in range(BATCH)])
    for _ in range(5):
        plan.launch()
    torch.cuda.synchronize()
    want = torch.from_numpy(np.array(_pil_resize(srcs[3].cpu().numpy(), new))).permute(2, 0, 1)      # a writable copy
    assert torch.equal(stage[3].cpu(), want), "the device resize differs from Pillow"
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = None
    for _ in range(3):
        e0.record()
        for _ in range(reps):
            plan.launch()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1) / reps
        best = ms if best is None else min(best, ms)
    return best * 1e-3


def call_time(ops, torch, dev, hw, new, reps):
    imgs = _images(hw, BATCH)
    stage = torch.zeros(BATCH, 3, new[0], new[1], dtype=torch.uint8, device=dev)
    outs = [stage[b] for b in range(BATCH)]
    views = [a.transpose(2, 0, 1) for a in imgs]
    for _ in range(3):
        ops.resize_u8(views, [new] * BATCH, outs=outs)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        ops.resize_u8(views, [new] * BATCH, outs=outs)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def eval_times(torch, dev, mode, hw, new, steps, warmup):
    import bench
    model, _ = bench.build_model(mode, dev, seed=1)
    model.eval()
    imgs = _images(hw, BATCH)
    raw = [{"image_raw": a, "resize_hw": new, "height": hw[0], "width": hw[1]} for a in imgs]
    host = [{"image": torch.from_numpy(np.ascontiguousarray(_pil_resize(a, new).transpose(2, 0, 1))), "height": hw[0],
             "width": hw[1]} for a in imgs]
    out = {}
    with torch.no_grad():
        for name, recs in (("host_resized", host), ("raw", raw)):
            for _ in range(warmup):
                model(recs)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                model(recs)
            torch.cuda.synchronize()
            out[name] = (time.perf_counter() - t0) / steps
    return out


# ------------------------------------------------------------------------------- --affine-test
AT_SOURCES = ((480, 640), (640, 480), (427, 640), (375, 500))      # (h, w): a COCO-like mix
AT_BATCH = 16
AT_LEGS = (("ResizeShortestEdge 512", ""), ("fix_res 512x512", "fix_res"), ("keep_res", "keep_res"))
AT_DATASET = "bench_affine_test_mixed"


def _at_dataset(root, batches):
    """batches * AT_BATCH JPEGs, the four source sizes in rotation (every batch holds all four)"""
    from PIL import Image
    rng = np.random.RandomState(5)
    dicts = []
    for i in range(batches * AT_BATCH):
        h, w = AT_SOURCES[i % len(AT_SOURCES)]
        path = os.path.join(root, f"{i:04d}.jpg")
        Image.fromarray(rng.randint(0, 256, (h // 8, w // 8, 3), dtype=np.uint8)).resize((w, h), Image.BILINEAR).save(path, quality=90)
        dicts.append({"file_name": path, "image_id": i, "height": h, "width": w})
    return dicts


def _at_leg(torch, model, cfg, mode):
    """(images/s, share of batches that replayed a captured graph, sizes after mapping) of inference_on_dataset over the mixed
    set: raw records of the test loader, mapped once and fed from memory (no decode in the time)"""
    from detectron2_centernet_amd.data import build_detection_test_loader
    from detectron2_centernet_amd.evaluation import inference_on_dataset
    c = cfg.clone()
    c.INPUT.MIN_SIZE_TEST, c.INPUT.DEVICE_RESIZE, c.TEST.BATCH_SIZE = 512, True, AT_BATCH
    c.INPUT.AFFINE.TEST_MODE, c.INPUT.AFFINE.OUTPUT_SIZE = mode, (512, 512)
    batches = list(build_detection_test_loader(c, AT_DATASET, num_workers=0))
    assert all(len(b) == AT_BATCH and "image_raw" in b[0] and (("warp" in b[0]) == bool(mode)) for b in batches)
    replays = [0]
    real_replay = torch.cuda.CUDAGraph.replay

    def counted(self):
        replays[0] += 1
        return real_replay(self)
    model._engines = {}
    torch.cuda.CUDAGraph.replay = counted
    try:
        inference_on_dataset(model, batches, None)
    finally:
        torch.cuda.CUDAGraph.replay = real_replay
    timing = inference_on_dataset.last_timing
    sizes = sorted({tuple(r["resize_hw"]) for b in batches for r in b})
    return AT_BATCH / timing["total_s_per_iter"], replays[0] / len(batches), sizes, len(batches), timing["iters"]


def _at_post_times(torch, ops, dev, reps, B=64, K=100):
    """per launch of ctdet_postprocess_affine / ctdet_postprocess, HIP events, warm-up, best of three, the two alternating:
    (a) `reps` launches captured in one graph, ten replays per timing -- the device's time, the host's launch cost left out;
    (b) `reps` calls of the Python wrapper back to back -- what a caller pays, launch-bound for a kernel this small"""
    g = torch.Generator().manual_seed(3)
    xy = torch.rand(B, K, 2, generator=g) * 400
    boxes = torch.cat([xy, xy + torch.rand(B, K, 2, generator=g) * 100 + 1], 2).to(dev)
    scores, classes = torch.rand(B, K, generator=g).to(dev), torch.randint(0, 80, (B, K), generator=g, dtype=torch.int32).to(dev)
    p4 = torch.tensor([[1.25, 1.25, 640.0, 480.0]] * B, device=dev)
    p6 = torch.tensor([[1.25, 1.25, 0.0, -80.0, 640.0, 480.0]] * B, device=dev)
    legs = (("ctdet_postprocess_affine", ops.postprocess_affine, p6), ("ctdet_postprocess", ops.postprocess, p4))
    graphs = {}
    for name, fn, params in legs:
        for _ in range(10):
            fn(boxes, scores, classes, K, 0.3, params)
        torch.cuda.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            for _ in range(reps):
                fn(boxes, scores, classes, K, 0.3, params)
        for _ in range(3):
            graphs[name].replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = {}
    for _ in range(3):
        for name, fn, params in legs:
            e0.record()
            for _ in range(10):
                graphs[name].replay()
            e1.record()
            e1.synchronize()
            t = e0.elapsed_time(e1) / (10 * reps) * 1e-3
            out[name + "_graph"] = min(out.get(name + "_graph", t), t)
            e0.record()
            for _ in range(reps):
                fn(boxes, scores, classes, K, 0.3, params)
            e1.record()
            e1.synchronize()
            t = e0.elapsed_time(e1) / reps * 1e-3
            out[name + "_call"] = min(out.get(name + "_call", t), t)
    return out


def affine_test_main(args, say):
    """the --affine-test leg: one MI355X, DLA-34 f16x3, TEST.BATCH_SIZE 16, raw records of a set that mixes four source sizes"""
    import tempfile

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_resize needs a ROCm GPU: nothing here is measurable without one")
    import bench
    from detectron2_centernet_amd import ops
    from detectron2_centernet_amd.data import DatasetCatalog
    dev = torch.device("cuda:0")
    rec = {}
    say(f"# tools/bench_resize.py --affine-test on {torch.cuda.get_device_name(0)}; DLA-34 f16x3, TEST.BATCH_SIZE {AT_BATCH}, raw records")
    say("sources (h x w) in rotation: " + ", ".join(f"{h}x{w}" for h, w in AT_SOURCES))
    model, cfg = bench.build_model("f16x3", dev, seed=1)
    model.eval()
    with tempfile.TemporaryDirectory(prefix="ctdet_affine_test_") as root:
        dicts = _at_dataset(root, args.batches)
        if AT_DATASET not in DatasetCatalog:
            DatasetCatalog.register(AT_DATASET, lambda: dicts)
        say("inference_on_dataset, records mapped once and fed from memory (host clock over the timed batches):")
        for name, mode in AT_LEGS:
            rate, share, sizes, n, timed = _at_leg(torch, model, cfg, mode)
            key = mode or "resize_shortest_edge"
            rec.update({f"{key}_img_s": rate, f"{key}_graph_share": share})
            say(f"  {name:24s} {rate:8.1f} img/s, {share * 100:5.1f} % of the {n} batches replayed a captured engine "
                f"({timed} timed); sizes after mapping {sizes}")
    t = _at_post_times(torch, ops, dev, args.reps)
    rec.update({k + "_us": v * 1e6 for k, v in t.items()})
    say("per launch at B = 64, K = 100 (HIP events, warm-up, best of three, the two alternating):")
    for name in ("ctdet_postprocess_affine", "ctdet_postprocess"):
        say(f"  {name:26s} {t[name + '_graph'] * 1e6:6.2f} us in a captured graph of {args.reps} launches (device time), "
            f"{t[name + '_call'] * 1e6:6.2f} us per call of the Python wrapper back to back")
    say(json.dumps({"bench_affine_test": rec}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--affine-test", action="store_true", help="the INPUT.AFFINE.TEST_MODE leg alone (DESIGN.md 7.13)")
    ap.add_argument("--batches", type=int, default=40, help="--affine-test: batches of the mixed set")
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--modes", default="f16x3,f16")
    ap.add_argument("--no-eval", action="store_true")
    args = ap.parse_args()

    lines, record = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if args.affine_test:
        affine_test_main(args, say)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return

    host = [host_times(hw, new) for hw, new in CASES]      # before the GPU is touched: the workers are forked

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_resize needs a ROCm GPU: nothing here is measurable without one")
    import detectron2_centernet_amd  # noqa: F401
    from detectron2_centernet_amd import ops
    dev = torch.device("cuda:0")
    say(f"# tools/bench_resize.py on {torch.cuda.get_device_name(0)}; {BATCH} images per batch, Pillow {__import__('PIL').__version__}")
    for (hw, new), (t1, t16) in zip(CASES, host):
        tk = kernel_time(ops, torch, dev, hw, new, args.reps)
        tc = call_time(ops, torch, dev, hw, new, max(args.reps // 10, 5))
        nbytes = BATCH * 3 * (hw[0] * hw[1] + new[0] * new[1])
        gbs = nbytes / tk / 1e9
        rec = {"case": f"{hw[0]}x{hw[1]}->{new[0]}x{new[1]}", "host_1_thread_ms": t1 * 1e3, "host_16_workers_ms": t16 * 1e3,
               "kernel_ms": tk * 1e3, "bytes": nbytes, "kernel_GBs": gbs, "share_of_hbm_peak": gbs / HBM_PEAK_GBS,
               "call_from_host_images_ms": tc * 1e3, "kernel_faster_than_16_workers": tk < t16}
        say(f"{rec['case']}: host Pillow {t1 * 1e3:.2f} ms single-threaded ({BATCH / t1:.0f} img/s), {t16 * 1e3:.2f} ms with "
            f"{WORKERS} workers ({BATCH / t16:.0f} img/s)")
        say(f"  batched launch {tk * 1e6:.1f} us device time ({BATCH / tk:.0f} img/s); {nbytes / 1e6:.1f} MB to move -> "
            f"{gbs:.0f} GB/s = {100 * gbs / HBM_PEAK_GBS:.1f}% of the {HBM_PEAK_GBS:.0f} GB/s HBM peak; "
            f"{t16 / tk:.0f}x the {WORKERS}-worker host path")
        say(f"  ops.resize_u8 from host images (pinned copy + upload + launch): {tc * 1e3:.2f} ms per batch ({BATCH / tc:.0f} img/s)")
        if not args.no_eval:
            for mode in [m for m in args.modes.split(",") if m]:
                ev = eval_times(torch, dev, mode, hw, new, args.steps, args.warmup)
                rec[f"eval_{mode}_host_resized_ms"] = ev["host_resized"] * 1e3
                rec[f"eval_{mode}_raw_ms"] = ev["raw"] * 1e3
                say(f"  eval step {mode}: host-resized records {ev['host_resized'] * 1e3:.2f} ms, raw records {ev['raw'] * 1e3:.2f} ms "
                    f"(host resize of the batch not in the first figure: +{t16 * 1e3:.1f} ms with {WORKERS} workers)")
        record.append(rec)
    say(json.dumps({"bench_resize": record}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
