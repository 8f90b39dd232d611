#!/usr/bin/env python
"""Dev tool: what COCO box-AP scoring costs at COCO-val scale (5 000 images x 100 detections, 80 classes, ~37 k annotations,
synthetic: `coco_scale_inputs` of tests/cocoeval_ref.py, the oracle module this tool needs anyway).  Prints
  * device time of ctdet_cocoeval_match and ctdet_cocoeval_accumulate separately (HIP events, after warm-up; --repeats windows
    of --iters calls each, every window's mean reported: the spread is part of the figure),
  * wall time of COCOEvaluator.evaluate() (concatenate, upload of the ground truth, both calls, copy back, summary),
  * tests/cocoeval_ref.py (numpy / Python loops) on a --subset of the images, scaled to the whole set: the host alternative,
and one JSON line with all of them.  --images-per-s puts the device time of the eval pass that produces the detections next
to them (5 000 / the images/s `bench.py` measured)."""
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
import cocoeval_ref as CR  # noqa: E402
from _evalbench import timed  # noqa: E402
from detectron2_centernet_amd.data.catalog import DatasetCatalog, MetadataCatalog  # noqa: E402
from detectron2_centernet_amd.evaluation import COCOEvaluator, COCOevalHIP, prepare_ground_truth  # noqa: E402
from detectron2_centernet_amd.structures import Boxes, BoxMode, Instances  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--classes", type=int, default=80)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=400, help="calls per timed window (400 x 0.4 ms: windows of >= 0.15 s)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--subset", type=int, default=500)
    ap.add_argument("--images-per-s", type=float, default=0.0, help="measured eval throughput of bench.py, for the comparison")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_cocoeval.py measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda:0")
    I, K = args.images, args.classes
    anns, boxes, scores, classes, image, _, _ = CR.coco_scale_inputs(I=I, K=K)
    gt = prepare_ground_truth(range(I), range(K), anns)
    boxes, scores, classes, image = (torch.as_tensor(a).to(dev) for a in (boxes, scores, classes, image))
    ev = COCOevalHIP(gt, boxes, scores, classes, image)
    ev.evaluate()
    ev.accumulate()
    stats = ev.summarize()
    match_w = timed(ev._match, args.warmup, args.iters, args.repeats)
    accum_w = timed(ev._accumulate, args.warmup, args.iters, args.repeats)
    match_ms, accum_ms = float(np.median(match_w)), float(np.median(accum_w))

    # ---- the evaluator, end to end: per-image device Instances in, result dict out
    name = f"bench_cocoeval_{os.getpid()}"
    anns = {}
    order = np.argsort(gt["image"], kind="stable")
    for j in order:
        anns.setdefault(int(gt["image"][j]), []).append(
            {"bbox": gt["boxes"][j].tolist(), "bbox_mode": BoxMode.XYWH_ABS, "category_id": int(gt["classes"][j]), "iscrowd": int(gt["crowd"][j])})
    recs = [{"file_name": str(i), "image_id": i, "height": 800, "width": 800, "annotations": anns.get(i, [])} for i in range(I)]
    DatasetCatalog.register(name, lambda: recs)
    MetadataCatalog.get(name).set(thing_classes=[f"class_{k}" for k in range(K)])
    evaluator = COCOEvaluator(name, None, False)
    per = int(scores.numel()) // I
    walls = []
    for rep in range(3):
        evaluator.reset()
        for i in range(I):
            inst = Instances((800, 800))
            sl = slice(i * per, (i + 1) * per)
            inst.pred_boxes, inst.scores, inst.pred_classes = Boxes(boxes[sl]), scores[sl], classes[sl].long()
            evaluator.process([{"image_id": i}], [{"instances": inst}])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = evaluator.evaluate()
        walls.append(time.perf_counter() - t0)
    # ---- the host alternative on a subset of the images
    S = min(args.subset, I)
    dsel, gsel = (image < S).cpu().numpy(), gt["image"] < S
    t0 = time.perf_counter()
    CR.evaluate(boxes.cpu().numpy()[dsel], scores.cpu().numpy()[dsel], classes.cpu().numpy()[dsel], image.cpu().numpy()[dsel],
                gt["boxes"][gsel], gt["area"][gsel], gt["crowd"][gsel], gt["image"][gsel], gt["classes"][gsel], S, K)
    ref_s = time.perf_counter() - t0
    out = {"images": I, "detections": int(scores.numel()), "annotations": int(len(gt["area"])), "classes": K,
           "match_ms": round(match_ms, 3), "accumulate_ms": round(accum_ms, 3), "iters": args.iters,
           "match_windows_ms": [round(v, 3) for v in match_w], "accumulate_windows_ms": [round(v, 3) for v in accum_w], "evaluate_wall_ms": [round(w * 1e3, 1) for w in walls],
           "host_ref_subset_images": S, "host_ref_subset_s": round(ref_s, 2), "host_ref_scaled_s": round(ref_s * I / S, 1),
           "AP": round(float(stats[0]), 4), "evaluator_AP": round(res["bbox"]["AP"], 2)}
    span = lambda w: f"{min(w):.3f} .. {max(w):.3f} over {len(w)} windows of {args.iters}"      # noqa: E731
    print(f"match      {match_ms:8.3f} ms   ({span(match_w)}; sort, offsets, ranks, one wave per (image, category) cell)")
    print(f"accumulate {accum_ms:8.3f} ms   ({span(accum_w)}; sort, one workgroup per (category, area range, maxDet, threshold))")
    print(f"COCOEvaluator.evaluate() wall: {', '.join(f'{w * 1e3:.1f}' for w in walls)} ms")
    print(f"cocoeval_ref on {S} images: {ref_s:.2f} s  -> {ref_s * I / S:.1f} s scaled to {I}")
    if args.images_per_s > 0:
        out["eval_pass_ms"] = round(I / args.images_per_s * 1e3, 1)
        print(f"eval pass that produces the detections: {I} / {args.images_per_s:.0f} images/s = {out['eval_pass_ms']:.1f} ms")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
