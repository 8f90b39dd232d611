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
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for fn in (plan.launch, jit.launch_sum, jit.launch_jitter):      # repeated in place: the same work on other bytes
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
        out.append(best)
    return out, jit.n, jit.sums.numel()


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


def main():
    ap = argparse.ArgumentParser()
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
