#!/usr/bin/env python
"""Dev tool: what Pascal VOC box-AP scoring costs at VOC2007-test scale (4 952 images x 100 detections, 20 classes, ~15 k
objects, synthetic: `voc_scale_inputs` of tests/voc_cases.py, the oracle module this tool needs anyway).  Prints
  * device time of ctdet_voceval_match and ctdet_voceval_ap separately (HIP events, after warm-up; --repeats windows of --iters
    calls each, every window's mean reported: the spread is part of the figure),
  * wall time of VOCevalHIP.evaluate() (upload of the ground truth, both calls, copy back of the two [K, T] tables),
  * tests/voc_cases.py (the numpy restatement, Python loops) on a --subset of the images, scaled to the whole set: the host
    alternative,
and one JSON line with all of them.  --images-per-s puts the device time of the eval pass that produces the detections next
to them (images / the images/s `bench.py` measured)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import voc_cases as VC  # noqa: E402
from _evalbench import f64, ptr as p, stream as current_stream, timed, workspace  # noqa: E402
from detectron2_centernet_amd import _lib  # noqa: E402
from detectron2_centernet_amd.evaluation import VOCevalHIP  # noqa: E402
from detectron2_centernet_amd.evaluation.voceval import RECALL_POINTS_07  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=4952)
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=100, help="calls per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--subset", type=int, default=300)
    ap.add_argument("--images-per-s", type=float, default=0.0, help="measured eval throughput of bench.py, for the comparison")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_voceval.py measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda:0")
    I, K, T = args.images, args.classes, len(VC.THRESHOLDS)
    gt, boxes, scores, classes, image = VC.voc_scale_inputs(I=I, K=K)
    N, NG = len(scores), len(gt["difficult"])
    dgt = {"image_ids": list(range(I)), "class_names": list(range(K)), "boxes": gt["boxes"], "difficult": gt["difficult"],
           "off": gt["off"]}
    d = [torch.as_tensor(a).to(dev) for a in (boxes, scores, classes, image)]
    # ---- wall time of the whole scorer, the first call (module load, allocations) reported apart
    walls = []
    for _ in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev = VOCevalHIP(dgt, *d)
        ev.evaluate(VC.THRESHOLDS, 2007)
        walls.append((time.perf_counter() - t0) * 1e3)
    # ---- the two calls on their own
    L = _lib.voceval_lib()
    gb, gd, go = f64(gt["boxes"], dev), torch.as_tensor(gt["difficult"]).to(dev), torch.as_tensor(gt["off"]).to(dev)
    thr, pts = f64(VC.THRESHOLDS, dev), f64(RECALL_POINTS_07, dev)
    ws, wsp = workspace(L.ctdet_voceval_workspace_bytes(N, NG, I, K, T), dev)
    order, cls_off = torch.empty(N, dtype=torch.int32, device=dev), torch.empty(K + 1, dtype=torch.int32, device=dev)
    flags, npos = torch.empty((N, T), dtype=torch.uint8, device=dev), torch.empty(K, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ap07, ap12 = (torch.empty((K, T), dtype=torch.float64, device=dev) for _ in range(2))
    stream = current_stream(dev)

    def match():
        _lib.check(L.ctdet_voceval_match(p(d[0]), p(d[1]), p(d[2]), p(d[3]), N, p(gb), p(gd), p(go), NG, I, K, p(thr), T, wsp,
                                         p(order), p(cls_off), p(flags), p(npos), p(status), stream), "ctdet_voceval_match")

    def ap_call():
        _lib.check(L.ctdet_voceval_ap(p(order), p(cls_off), p(flags), p(npos), N, K, T, p(pts), wsp, p(ap07), p(ap12), None, None,
                                      stream), "ctdet_voceval_ap")
    t_match = timed(match, args.warmup, args.iters, args.repeats)
    t_ap = timed(ap_call, args.warmup, args.iters, args.repeats)
    assert int(status.item()) == 0 and np.array_equal(ap07.cpu().numpy(), ev.ap07)
    # ---- the host alternative on the first --subset images
    sub = min(args.subset, I)
    keep = image < sub
    sgt = {"I": sub, "K": K, "boxes": gt["boxes"][:gt["off"][sub * K]], "difficult": gt["difficult"][:gt["off"][sub * K]],
           "off": gt["off"][:sub * K + 1]}
    t0 = time.perf_counter()
    host = VC.voc_score(sgt, boxes[keep], scores[keep], classes[keep], image[keep])
    host_s = time.perf_counter() - t0
    out = {"images": I, "classes": K, "detections": N, "ground_truths": NG, "thresholds": T,
           "match_ms": [round(v, 4) for v in t_match], "ap_ms": [round(v, 4) for v in t_ap],
           "evaluate_wall_ms_first": round(walls[0], 2), "evaluate_wall_ms": [round(v, 2) for v in walls[1:]],
           "host_subset_images": sub, "host_subset_s": round(host_s, 3), "host_scaled_s": round(host_s * I / sub, 2),
           "mAP50_07": round(float(ev.ap07[:, 0].mean() * 100), 3), "mAP50_12": round(float(ev.ap12[:, 0].mean() * 100), 3),
           "host_subset_mAP50_07": round(float(host["ap07"][:, 0].mean() * 100), 3)}
    if args.images_per_s > 0:
        out["inference_pass_s"] = round(I / args.images_per_s, 3)
        out["scoring_share_of_inference"] = round((np.mean(t_match) + np.mean(t_ap)) * 1e-3 / (I / args.images_per_s), 6)
    print(f"voceval at {I} images x {N // I} detections, {K} classes, {NG} objects, {T} thresholds")
    print(f"  ctdet_voceval_match  {np.mean(t_match):8.3f} ms  windows {out['match_ms']}")
    print(f"  ctdet_voceval_ap     {np.mean(t_ap):8.3f} ms  windows {out['ap_ms']}")
    print(f"  VOCevalHIP.evaluate  {np.mean(walls[1:]):8.2f} ms wall (first call {walls[0]:.1f} ms)")
    print(f"  numpy restatement    {host_s:8.2f} s on {sub} images -> {out['host_scaled_s']} s scaled to {I}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
