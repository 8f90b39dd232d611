#!/usr/bin/env python
"""Dev tool: the deformable ResNet-50 (MODEL.RESNETS.DEFORM_ON_PER_STAGE [False, True, True, True]) on the MI355X.

  1. per layer: the deformable 3x3 of res3 (128 ch, 64x64) and res4 (256 ch, 32x32) at batch 16 (a 512^2 training batch), in
     f16x3 / f32 / f16, forward (ops.dcnv2) and backward (columns, dW, d(columns), scatter: ops_train._dcn_backward) --
     mask mode NONE (DCNv1, the mask-free kernels, 20-float offset rows) against the modulated kernels fed an all-ones
     probability mask (28-float rows), the A/B baseline of the mask-free variants;
  2. the whole f16x3 training step at 16 x 512^2, plain R50 against R50-dconv (DCNv1), images/s;
  3. eval at 8 x 800^2 (f16x3), images/s.
200 warm-up launches and 1000 timed per layer figure (shorter runs from an idle device measure the clock ramp).  Prints one
line per figure and one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402  (its config texts; nothing of bench.py is changed or run)
from detectron2_centernet_amd import ops  # noqa: E402
from detectron2_centernet_amd import ops_train as ot  # noqa: E402

dev = torch.device("cuda:0")
LAYERS = {"res3": (16, 64, 64, 128), "res4": (16, 32, 32, 256)}
COMP = {"f16x3": ops.F16X3, "f32": ops.F32, "f16": ops.F16}


def timed(fn, warm, iters):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1000.0      # us per call


def layer_bench(warm, iters):
    out = []
    g = torch.Generator(device=dev).manual_seed(0)
    for name, (B, H, W, C) in LAYERS.items():
        for prec, comp in COMP.items():
            dt = torch.float16 if prec == "f16" else torch.float32
            x = torch.randn(B, H, W, C, generator=g, device=dev).to(dt)
            w = torch.randn(C, C, 3, 3, generator=g, device=dev) / (C * 9) ** 0.5
            off = torch.randn(B, H, W, 18, generator=g, device=dev)        # ~1 px offsets
            om1 = torch.zeros(B, H, W, 20, device=dev)
            om1[..., :18] = off
            omp = torch.zeros(B, H, W, 28, device=dev)
            omp[..., :18] = off
            omp[..., 18:27] = 1.0
            dy = (torch.randn(B, H, W, C, generator=g, device=dev) * 0.1).to(dt)
            p = ops.PackedConv(w, None, None, stride=1, pad=1, compute=comp, cout_align=64 if prec == "f16" else None)
            r = {"layer": name, "B": B, "H": H, "W": W, "C": C, "precision": prec}
            for tag, om, mm in (("v1", om1, ops.DCN_MASK_NONE), ("ones", omp, ops.DCN_MASK_PROB)):
                r[f"{tag}_fwd_us"] = timed(lambda: ops.dcnv2(x, om, p, mask_is_prob=mm), warm, iters)
                r[f"{tag}_bwd_us"] = timed(lambda: ot._dcn_backward(x, om, w, dy, mm, comp, 1.0), max(2, warm // 10),
                                           max(5, iters // 10))
            print(f"{name} {B}x{H}x{W}x{C} {prec:6s} fwd v1 {r['v1_fwd_us']:8.1f} us  ones-mask {r['ones_fwd_us']:8.1f} us | "
                  f"bwd v1 {r['v1_bwd_us']:8.1f} us  ones-mask {r['ones_bwd_us']:8.1f} us", flush=True)
            out.append(r)
    return out


def build(precision, deform, seed=0):
    from detectron2_centernet_amd.config import get_cfg
    from detectron2_centernet_amd.data.catalog import register_synthetic
    from detectron2_centernet_amd.modeling import build_model

    d = tempfile.mkdtemp(prefix="ctdet_cfg_")
    with open(os.path.join(d, "Base-CenterNet.yaml"), "w") as f:
        f.write(bench.BASE_YAML)
    with open(os.path.join(d, "ctdet_res_50_1x.yaml"), "w") as f:
        f.write(bench.RES50_YAML)
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(d, "ctdet_res_50_1x.yaml"))
    cfg.MODEL.CENTERNET.HIP_PRECISION = precision
    cfg.MODEL.DEVICE = str(dev)
    if deform:
        cfg.MODEL.RESNETS.DEFORM_ON_PER_STAGE = [False, True, True, True]
        cfg.MODEL.RESNETS.DEFORM_MODULATED = False
    register_synthetic("bulb_train", num_classes=80)
    torch.manual_seed(seed)
    model = build_model(cfg)
    g = torch.Generator().manual_seed(seed + 1)
    for name, m in model.named_modules():
        if name.endswith("conv2_offset"):      # ~1 px offsets: data-dependent gathers, not the zero-init regular grid
            m.weight.data.copy_((torch.randn(m.weight.shape, generator=g) * (0.5 / (m.weight.shape[1] * 9) ** 0.5)).to(dev))
            m.bias.data.copy_((torch.randn(m.bias.shape, generator=g) * 0.5).to(dev))
    model.wh[-1].bias.data.fill_(3.0)
    for m in model.deconv_layers.modules():
        if isinstance(m, torch.nn.ConvTranspose2d):
            m.weight.data.normal_(0, (2.0 / (m.weight.shape[0] * 4)) ** 0.5)
    return model, cfg


def train_bench(deform, steps, warmup, B=16, size=512):
    from detectron2_centernet_amd.engine.bench_train import synthetic_batch
    from detectron2_centernet_amd.engine.train_loop import SimpleTrainer

    model, cfg = build("f16x3", deform)
    model.train()
    cfg.SOLVER.IMS_PER_BATCH = B
    trainer = SimpleTrainer(model, None, cfg)
    batch = synthetic_batch(B, size, 0, dev)
    for _ in range(warmup):
        trainer.run_step_tensors(*batch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        trainer.run_step_tensors(*batch)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    losses = trainer.metrics()
    return {"images_per_s": B * steps / el, "step_ms": el / steps * 1e3, "losses": {k: float(v) for k, v in losses.items()}}


def eval_bench(deform, steps, warmup, B=8, size=800):
    model, _ = build("f16x3", deform)
    model.eval()
    g = torch.Generator().manual_seed(3)
    img = torch.randint(0, 256, (B, 3, size, size), generator=g, dtype=torch.uint8).to(dev)
    with torch.no_grad():
        for _ in range(warmup):
            model.infer_batch_tensor(img)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            model.infer_batch_tensor(img)
        torch.cuda.synchronize()
    el = time.perf_counter() - t0
    return {"images_per_s": B * steps / el, "batch_ms": el / steps * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=200)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip", default="", help="comma-separated parts to skip: layers, train, eval")
    args = ap.parse_args()
    skip = set(filter(None, args.skip.split(",")))
    res = {"device": torch.cuda.get_device_name(0)}
    if "layers" not in skip:
        res["layers"] = layer_bench(args.warm, args.iters)
    if "train" not in skip:
        res["train_16x512_f16x3"] = {k: train_bench(k == "r50_dconv", args.steps, args.warmup) for k in ("r50", "r50_dconv")}
        for k, v in res["train_16x512_f16x3"].items():
            print(f"train 16x512^2 f16x3 {k:10s} {v['images_per_s']:8.1f} img/s ({v['step_ms']:.1f} ms/step)", flush=True)
    if "eval" not in skip:
        res["eval_8x800_f16x3"] = {k: eval_bench(k == "r50_dconv", args.steps, args.warmup) for k in ("r50", "r50_dconv")}
        for k, v in res["eval_8x800_f16x3"].items():
            print(f"eval 8x800^2 f16x3 {k:10s} {v['images_per_s']:8.1f} img/s ({v['batch_ms']:.1f} ms/batch)", flush=True)
    print(json.dumps({"bench_deform_resnet": res}))


if __name__ == "__main__":
    main()
