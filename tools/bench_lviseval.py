#!/usr/bin/env python
"""Dev tool: what LVIS box-AP scoring costs at LVIS-val scale (19 809 images x 300 detections, 1 203 classes, ~244 k objects,
synthetic: `lvis_scale_inputs` of tests/lvis_cases.py, the oracle module this tool needs anyway).  Prints
  * device time of ctdet_lviseval_match and ctdet_lviseval_accumulate separately (HIP events, after warm-up; --repeats windows
    of --iters calls each, every window's mean reported: the spread is part of the figure),
  * wall time of LVISevalHIP.evaluate() (upload of the ground truth and the [I, K] lists, both calls, copy back of the two
    tables, the summaries),
  * tests/lvis_cases.py (the numpy restatement, Python loops) on a --subset of the images, scaled to the whole set: the host
    alternative (its per-class part does not shrink with the subset, so the scaled figure is an upper estimate),
and one JSON line with all of them."""
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
import lvis_cases as LC  # noqa: E402
from _evalbench import f64, ptr as p, stream as current_stream, timed, workspace  # noqa: E402
from detectron2_centernet_amd import _lib  # noqa: E402
from detectron2_centernet_amd.evaluation import LVISevalHIP  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=19809)
    ap.add_argument("--classes", type=int, default=1203)
    ap.add_argument("--per-image", type=int, default=300)
    ap.add_argument("--objects", type=int, default=244000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10, help="calls per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--subset", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lviseval.py measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda:0")
    I, K = args.images, args.classes
    T, A, R = len(LC.IOU_THRS), len(LC.AREA_RNGS), len(LC.REC_THRS)
    gt, boxes, scores, classes, image, frequency = LC.lvis_scale_inputs(I=I, K=K, per_image=args.per_image, objects=args.objects)
    N, NG = len(scores), len(gt["area"])
    dgt = {"image_ids": list(range(I)), "cat_ids": list(range(K)), "boxes": gt["boxes"], "area": gt["area"], "ignore": gt["ignore"],
           "off": gt["off"], "lists": gt["lists"], "frequency": frequency}
    d = [torch.as_tensor(a).to(dev) for a in (boxes, scores, classes, image)]
    # ---- wall time of the whole scorer, the first call (module load, allocations) reported apart
    walls = []
    for _ in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev = LVISevalHIP(dgt, *d)
        res = ev.evaluate()
        walls.append((time.perf_counter() - t0) * 1e3)
    # ---- the two calls on their own
    L = _lib.lviseval_lib()
    gb, ga = f64(gt["boxes"], dev), f64(gt["area"], dev)
    gi, go, gl = (torch.as_tensor(gt[k]).to(dev) for k in ("ignore", "off", "lists"))
    thr, rng, rec = f64(LC.IOU_THRS, dev), f64(LC.AREA_RNGS, dev), f64(LC.REC_THRS, dev)
    ws, wsp = workspace(L.ctdet_lviseval_workspace_bytes(N, NG, I, K, A, T), dev)
    order, cls_off = torch.empty(N, dtype=torch.int32, device=dev), torch.empty(K + 1, dtype=torch.int32, device=dev)
    flags, npig = torch.empty((N, A * T), dtype=torch.uint8, device=dev), torch.empty((K, A), dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    precision = torch.empty((T, R, K, A), dtype=torch.float64, device=dev)
    recall = torch.empty((T, K, A), dtype=torch.float64, device=dev)
    stream = current_stream(dev)

    def match():
        _lib.check(L.ctdet_lviseval_match(p(d[0]), p(d[1]), p(d[2]), p(d[3]), N, p(gb), p(ga), p(gi), p(go), NG, p(gl), I, K, p(thr),
                                          T, p(rng), A, LC.MAX_DETS, wsp, p(order), p(cls_off), p(flags), p(npig), p(status),
                                          stream), "ctdet_lviseval_match")

    def accumulate():
        _lib.check(L.ctdet_lviseval_accumulate(p(order), p(cls_off), p(flags), p(npig), N, K, A, T, p(rec), R, p(precision),
                                               p(recall), stream), "ctdet_lviseval_accumulate")
    t_match = timed(match, args.warmup, args.iters, args.repeats)
    t_acc = timed(accumulate, args.warmup, args.iters, args.repeats)
    assert int(status.item()) == 0 and precision.cpu().numpy().tobytes() == ev.precision.tobytes()
    # ---- the host alternative on the first --subset images
    sub = min(args.subset, I)
    keep = image < sub
    end = gt["off"][sub * K]
    sgt = {"I": sub, "K": K, "boxes": gt["boxes"][:end], "area": gt["area"][:end], "ignore": gt["ignore"][:end],
           "off": gt["off"][:sub * K + 1], "lists": gt["lists"][:sub]}
    t0 = time.perf_counter()
    host = LC.lvis_score(sgt, boxes[keep], scores[keep], classes[keep], image[keep])
    host_s = time.perf_counter() - t0
    out = {"images": I, "classes": K, "detections": N, "ground_truths": NG, "thresholds": T, "area_ranges": A,
           "taking_part": int(cls_off[-1].item()),
           "match_ms": [round(v, 4) for v in t_match], "accumulate_ms": [round(v, 4) for v in t_acc],
           "evaluate_wall_ms_first": round(walls[0], 2), "evaluate_wall_ms": [round(v, 2) for v in walls[1:]],
           "host_subset_images": sub, "host_subset_s": round(host_s, 3), "host_scaled_s": round(host_s * I / sub, 2),
           "AP": round(res["AP"] * 100, 3), "APr": round(res["APr"] * 100, 3), "APc": round(res["APc"] * 100, 3),
           "APf": round(res["APf"] * 100, 3),
           "host_subset_AP": round(LC.summarize(host["precision"], host["recall"], frequency)["AP"] * 100, 3)}
    print(f"lviseval at {I} images x {N // I} detections, {K} classes, {NG} objects, {T} thresholds x {A} area ranges")
    print(f"  ctdet_lviseval_match       {np.mean(t_match):8.3f} ms  windows {out['match_ms']}")
    print(f"  ctdet_lviseval_accumulate  {np.mean(t_acc):8.3f} ms  windows {out['accumulate_ms']}")
    print(f"  LVISevalHIP.evaluate       {np.mean(walls[1:]):8.2f} ms wall (first call {walls[0]:.1f} ms)")
    print(f"  numpy restatement          {host_s:8.2f} s on {sub} images -> {out['host_scaled_s']} s scaled to {I}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
