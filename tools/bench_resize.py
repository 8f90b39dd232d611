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


def main():
    ap = argparse.ArgumentParser()
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
