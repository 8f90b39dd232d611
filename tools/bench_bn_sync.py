#!/usr/bin/env python
"""Dev tool: the SyncBatchNorm split kernels (ctdet_bn_local_stats -> [collective] -> ctdet_bn_sync_fwd, and
ctdet_bn_local_grad_sums -> [collective] -> ctdet_bn_sync_bwd) against the fused single-GPU kernels (ctdet_bn_train_fwd /
_bwd) at the BatchNorm shapes of ResNet-18's trainable stages for a per-GPU batch of 3 at 800^2: res3 M = 3*100*100,
C = 128; res4 M = 3*50*50, C = 256; f32 and f16 tensors.  The collective is not part of the timed work (the slot buffers are
summed once, outside the loop, as the all-reduce would).  200 warm-up launches, 1000 timed (README: shorter runs from an
idle device measure the clock ramp).  Prints one line per shape, direction and dtype, and one JSON line."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from detectron2_centernet_amd import ops_train as ot  # noqa: E402

dev = torch.device("cuda:0")
SHAPES = {"res3": (3, 100, 100, 128), "res4": (3, 50, 50, 256)}
WARM, ITERS = 200, 1000


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ITERS * 1000.0      # us per call


def main():
    out = []
    g = torch.Generator(device=dev).manual_seed(0)
    for name, (B, H, W, C) in SHAPES.items():
        for dt in (torch.float32, torch.float16):
            y = (torch.randn(B, H, W, C, generator=g, device=dev) * 2 + 0.5).to(dt)
            res = torch.randn(B, H, W, C, generator=g, device=dev).to(dt)
            dz = torch.randn(B, H, W, C, generator=g, device=dev).to(dt)
            gamma, beta = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev)
            rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
            z, mean, invstd, scale = ot.bn_train_fwd(y, gamma, beta, rm, rv, 1e-5, 0.1, res=res, relu=True)
            stats = ot.bn_local_stats(y, 0, 1)
            sums, _, _ = ot.bn_local_grad_sums(dz, z, y, mean, invstd, 0, 1, relu=True)
            r = {"shape": name, "M": B * H * W, "C": C, "dtype": str(dt).split(".")[-1]}
            r["fused_fwd_us"] = timed(lambda: ot.bn_train_fwd(y, gamma, beta, rm, rv, 1e-5, 0.1, res=res, relu=True))
            r["split_fwd_us"] = timed(lambda: (ot.bn_local_stats(y, 0, 1),
                                               ot.bn_sync_fwd(y, stats, gamma, beta, rm, rv, 1e-5, 0.1, res=res, relu=True)))
            r["fused_bwd_us"] = timed(lambda: ot.bn_train_bwd(dz, z, y, mean, invstd, scale, relu=True, want_dres=True))
            r["split_bwd_us"] = timed(lambda: (ot.bn_local_grad_sums(dz, z, y, mean, invstd, 0, 1, relu=True),
                                               ot.bn_sync_bwd(dz, z, y, mean, invstd, scale, stats, sums, relu=True,
                                                              want_dres=True)))
            print(f"{name} M={r['M']:6d} C={C:3d} {r['dtype']:8s} fwd fused {r['fused_fwd_us']:6.1f} us  split "
                  f"{r['split_fwd_us']:6.1f} us | bwd fused {r['fused_bwd_us']:6.1f} us  split {r['split_bwd_us']:6.1f} us",
                  flush=True)
            out.append(r)
    print(json.dumps({"bench_bn_sync": out, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
