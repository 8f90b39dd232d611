#!/usr/bin/env python
"""Dev tool: the depthwise VoVNet-19 bodies (`V-19-slim-dw-eSE`, `V-19-dw-eSE`) on the MI355X.

  1. per depthwise layer at batch 64 x 512^2 (the eval batch), both bodies, f32 and f16 tensors: ops.dwconv3x3 in us and in
     GB/s of algorithmic bytes (input + output read / written once) against the achievable HBM rate (6.3 TB/s), next to the
     1x1 + FrozenBN + ReLU (pw) that follows each dw layer (f32 tensors: the f16x3 kernel the headline mode runs; f16: f16)
     -- the split that decides whether fusing the dw into the pw conv's operand load is worth it;
  2. input and weight gradient at the training shapes (16 x 512^2: stage3 and stage4 layers);
  3. whole model, f16x3: eval images/s at 64 x 512^2 and training-step images/s at 16 x 512^2, V-19-slim-dw-eSE against
     V-19-slim-eSE.
200 warm-up launches and 1000 timed per layer figure.  Prints one line per figure and one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402  (its config texts and image generator; nothing of bench.py is changed or run)
from detectron2_centernet_amd import _lib, ops  # noqa: E402
from detectron2_centernet_amd import ops_train as ot  # noqa: E402

dev = torch.device("cuda:0")
HBM_GBS = 6300.0
BODIES = {"V-19-slim-dw-eSE": [64, 80, 96, 112], "V-19-dw-eSE": [128, 160, 192, 224]}
VOV_YAML = """
_BASE_: "./Base-CenterNet.yaml"
MODEL:
  BACKBONE:
    NAME: "build_vovnet_backbone"
  VOVNET:
    OUT_FEATURES: ["stage2", "stage3", "stage4", "stage5"]
    CONV_BODY: "{body}"
  CENTERNET:
    HEAD_CONV: 64
    FOCAL_LOSS_ALPHA: [1]
DATASETS:
  TRAIN: ("bulb_train",)
  TEST: ("bulb_val",)
VERSION: 2
"""


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


def dw_layers(stage_ch, B=64):
    """(name, map size, C, stride) of every distinct dw layer shape of a body at 512^2 input"""
    return [("stem_2", 256, 64, 1), ("stem_3", 256, 64, 2), ("stage2", 128, stage_ch[0], 1), ("stage3", 64, stage_ch[1], 1),
            ("stage4", 32, stage_ch[2], 1), ("stage5", 16, stage_ch[3], 1)]


def layer_bench(warm, iters, B=64):
    out = []
    g = torch.Generator(device=dev).manual_seed(0)
    for body, stage_ch in BODIES.items():
        for name, S, C, stride in dw_layers(stage_ch):
            for prec in ("f32", "f16"):
                dt = torch.float16 if prec == "f16" else torch.float32
                x = torch.randn(B, S, S, C, generator=g, device=dev).to(dt)
                w = torch.randn(C, 1, 3, 3, generator=g, device=dev) * 0.3
                So = (S - 1) // stride + 1
                y = torch.empty(B, So, So, C, dtype=dt, device=dev)
                wk = ops.dw3_weight(w)
                t_dw = timed(lambda: ops.dwconv3x3(x, w, stride, out=y, prepared=wk), warm, iters)
                nbytes = (B * S * S + B * So * So) * C * x.element_size()
                pw = torch.randn(C, C, 1, 1, generator=g, device=dev) / C ** 0.5
                comp = ops.F16 if prec == "f16" else ops.F16X3
                p = ops.PackedConv(pw, torch.ones(C, device=dev), torch.zeros(C, device=dev), compute=comp)
                z = torch.empty(B, So, So, C, dtype=dt, device=dev)
                t_pw = timed(lambda: ops.conv2d(y, p, out=z, act=ops.ACT_RELU), warm, iters)
                gbs = nbytes / t_dw / 1e3
                r = {"body": body, "layer": name, "B": B, "H": S, "W": S, "C": C, "stride": stride, "precision": prec,
                     "dw_us": round(t_dw, 2), "dw_GBs": round(gbs, 1), "dw_hbm_frac": round(gbs / HBM_GBS, 3),
                     "pw_us": round(t_pw, 2), "pw_mode": "f16" if prec == "f16" else "f16x3",
                     "dw_share": round(t_dw / (t_dw + t_pw), 3)}
                print(f"{body:17s} {name:7s} {S:3d}^2 C={C:3d} s{stride} {prec}: dw {t_dw:8.1f} us {gbs:7.0f} GB/s "
                      f"({100 * gbs / HBM_GBS:4.1f}% HBM) | pw({r['pw_mode']}) {t_pw:8.1f} us | dw share {r['dw_share']:.2f}",
                      flush=True)
                out.append(r)
                del x, y, z
    return out


def grad_bench(warm, iters, B=16):
    out = []
    g = torch.Generator(device=dev).manual_seed(1)
    for body, stage_ch in BODIES.items():
        for name, S, C in (("stage3", 64, stage_ch[1]), ("stage4", 32, stage_ch[2])):
            for prec in ("f32", "f16"):
                dt = torch.float16 if prec == "f16" else torch.float32
                x = torch.randn(B, S, S, C, generator=g, device=dev).to(dt)
                dy = torch.randn(B, S, S, C, generator=g, device=dev).to(dt)
                w = torch.randn(C, 1, 3, 3, generator=g, device=dev) * 0.3
                wk = ops.dw3_weight(w)
                dx = torch.empty_like(x)
                t_dx = timed(lambda: ops.dwconv3x3(dy, w, 1, out=dx, rot180=True, prepared=wk), warm, iters)
                nb = _lib.lib().ctdet_dwconv3x3_wgrad_workspace_bytes(B, S, S, C, ops.dt_of(x))
                ws = torch.empty(nb // 4, device=dev)
                dw = torch.empty(C, 1, 3, 3, device=dev)
                t_dw = timed(lambda: ot.dwconv3x3_wgrad(x, dy, scale=1.0, into=dw, workspace=ws), warm, iters)
                nbytes = 2 * B * S * S * C * x.element_size()
                r = {"body": body, "layer": name, "B": B, "H": S, "W": S, "C": C, "precision": prec,
                     "dx_us": round(t_dx, 2), "dx_GBs": round(nbytes / t_dx / 1e3, 1),
                     "dw_us": round(t_dw, 2), "dw_GBs": round(nbytes / t_dw / 1e3, 1), "wgrad_workspace_bytes": nb}
                print(f"{body:17s} {name} {B}x{S}^2 C={C:3d} {prec}: dX {t_dx:7.1f} us ({r['dx_GBs']:6.0f} GB/s) | "
                      f"dW {t_dw:7.1f} us ({r['dw_GBs']:6.0f} GB/s)", flush=True)
                out.append(r)
    return out


def build(body, precision="f16x3", seed=0):
    from detectron2_centernet_amd.config import get_cfg
    from detectron2_centernet_amd.data.catalog import register_synthetic
    from detectron2_centernet_amd.modeling import build_model

    d = tempfile.mkdtemp(prefix="ctdet_cfg_")
    with open(os.path.join(d, "Base-CenterNet.yaml"), "w") as f:
        f.write(bench.BASE_YAML)
    with open(os.path.join(d, "vov.yaml"), "w") as f:
        f.write(VOV_YAML.format(body=body))
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(d, "vov.yaml"))
    cfg.MODEL.CENTERNET.HIP_PRECISION = precision
    cfg.MODEL.DEVICE = str(dev)
    register_synthetic("bulb_train", num_classes=80)
    torch.manual_seed(seed)
    model = build_model(cfg)
    model.wh[-1].bias.data.fill_(3.0)
    return model, cfg


def train_bench(body, steps, warmup, B=16, size=512):
    from detectron2_centernet_amd.engine.bench_train import synthetic_batch
    from detectron2_centernet_amd.engine.train_loop import SimpleTrainer

    model, cfg = build(body)
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
    return {"images_per_s": B * steps / el, "step_ms": el / steps * 1e3, "graph_state": trainer.graph_state,
            "losses": {k: float(v) for k, v in trainer.metrics().items()}}


def eval_bench(body, steps, warmup, B=64, size=512):
    model, _ = build(body)
    model.eval()
    img = bench.synthetic_images(B, size, 0, dev)
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
    ap.add_argument("--skip", default="", help="comma-separated parts to skip: layers, grads, train, eval")
    args = ap.parse_args()
    skip = set(filter(None, args.skip.split(",")))
    res = {"device": torch.cuda.get_device_name(0)}
    if "layers" not in skip:
        res["layers_64x512"] = layer_bench(args.warm, args.iters)
    if "grads" not in skip:
        res["grads_16x512"] = grad_bench(args.warm, args.iters)
    pair = ("V-19-slim-dw-eSE", "V-19-slim-eSE")
    if "eval" not in skip:
        res["eval_64x512_f16x3"] = {b: eval_bench(b, args.steps, args.warmup) for b in pair}
        for k, v in res["eval_64x512_f16x3"].items():
            print(f"eval 64x512^2 f16x3 {k:17s} {v['images_per_s']:8.1f} img/s ({v['batch_ms']:.1f} ms/batch)", flush=True)
        torch.cuda.empty_cache()
    if "train" not in skip:
        res["train_16x512_f16x3"] = {b: train_bench(b, args.steps, args.warmup) for b in pair}
        for k, v in res["train_16x512_f16x3"].items():
            print(f"train 16x512^2 f16x3 {k:17s} {v['images_per_s']:8.1f} img/s ({v['step_ms']:.1f} ms/step, "
                  f"{v['graph_state']})", flush=True)
    print(json.dumps({"bench_vovnet_dw": res}))


if __name__ == "__main__":
    main()
