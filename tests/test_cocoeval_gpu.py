"""COCO box-AP scoring on the GPU: the HIP matcher and PR kernels against the G22 fixture (the reference's native scorer --
exact, every value is a ratio of integers, a copied score or an f64 IoU computed without contraction), against the numpy
restatement (tests/cocoeval_ref.py) where the fixture does not reach, through the C ABI, through `COCOevalHIP` and through
`COCOEvaluator` + `inference_on_dataset`."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

import cocoeval_ref as CR
from detectron2_centernet_amd import _lib
from detectron2_centernet_amd.evaluation import (COCOEvaluator, COCOevalHIP, inference_on_dataset, instances_to_coco_json,
                                                 prepare_ground_truth)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
G22 = os.path.join(HERE, "golden", "g22_cocoeval.npz")
KEYS = ["AP", "AP50", "AP75", "APs", "APm", "APl"]


def _annotations(d, cat_of=lambda k: k, img_of=lambda i: i):
    return [{"id": int(d["gt_ids"][n]) if "gt_ids" in d else n + 1, "image_id": img_of(int(d["gt_image"][n])),
             "category_id": cat_of(int(d["gt_classes"][n])), "bbox": [float(v) for v in d["gt_boxes"][n]],
             "area": float(d["gt_area"][n]), "iscrowd": int(d["gt_crowd"][n])} for n in range(len(d["gt_area"]))]


def _scorer(d, I, K, dev):
    gt = prepare_ground_truth(range(I), range(K), _annotations(d))
    return COCOevalHIP(gt, torch.as_tensor(d["boxes"]).to(dev), torch.as_tensor(d["scores"]).to(dev),
                       torch.as_tensor(d["classes"]).to(dev), torch.as_tensor(d["image"]).to(dev))


def _run(ev):
    ev.evaluate()
    ev.accumulate()
    ev.summarize()
    return ev.eval["precision"], ev.eval["recall"], ev.eval["scores"]


def test_iou_hook_equals_the_fixture(dev):
    d = np.load(G22)
    L = _lib.lib()
    dx = CR.det_xywh(d["boxes"])
    assert len(d["iou_cells"]) > 100
    for c, (i, k) in enumerate(d["iou_cells"]):
        ds = np.where((d["image"] == i) & (d["classes"] == k))[0]
        gs = np.where((d["gt_image"] == i) & (d["gt_classes"] == k))[0]
        dt, gt = torch.as_tensor(dx[ds]).to(dev), torch.as_tensor(d["gt_boxes"][gs]).to(dev)
        cr = torch.as_tensor(d["gt_crowd"][gs]).to(dev)
        out = torch.full((len(ds), len(gs)), -7.0, dtype=torch.float64, device=dev)
        _lib.check(L.ctdet_cocoeval_iou(C.c_void_p(dt.data_ptr()), len(ds), C.c_void_p(gt.data_ptr()), C.c_void_p(cr.data_ptr()),
                                        len(gs), C.c_void_p(out.data_ptr()),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)), "ctdet_cocoeval_iou")
        want = d["iou_flat"][d["iou_off"][c]:d["iou_off"][c + 1]].reshape(len(ds), len(gs))
        assert np.array_equal(out.cpu().numpy(), want), (i, k)


def test_g22_through_the_abi_is_exact_and_repeatable(dev):
    d = np.load(G22)
    I, K = len(d["image_ids"]), d["precision"].shape[2]
    ev = _scorer(d, I, K, dev)
    precision, recall, scores = _run(ev)
    for got, name in ((precision, "precision"), (recall, "recall"), (scores, "scores_out")):
        bad = int((got != d[name]).sum())
        print(f"G22 {name}: {bad} of {got.size} entries differ")
    assert np.array_equal(precision, d["precision"])
    assert np.array_equal(recall, d["recall"])
    assert np.array_equal(scores, d["scores_out"])
    assert ev.eval["counts"] == [10, 101, K, 4, 3] and ev.stats.shape == (12,)
    assert np.array_equal(ev.stats, CR.summarize(d["precision"], d["recall"]))
    # a second run (new buffers) and a re-run of the same object: bit-identical
    p2, r2, s2 = _run(_scorer(d, I, K, dev))
    p3, r3, s3 = _run(ev)
    for a, b in ((p2, precision), (r2, recall), (s2, scores), (p3, precision), (r3, recall), (s3, scores)):
        assert a.tobytes() == b.tobytes()
    # the C ABI with a maxDet above the matcher's max_det: it acts as max_det (the cells were cut there), nothing unwritten
    # is read -- the column of maxDet 100 becomes the column of maxDet 10, which is what it was
    ev4 = _scorer(d, I, K, dev)
    ev4._upload()
    ev4._dev["max_det"] = 10
    ev4._match()
    ev4.accumulate()
    for name, full in (("precision", precision), ("recall", recall), ("scores", scores)):
        assert np.array_equal(ev4.eval[name][..., 2], full[..., 1]) and np.array_equal(ev4.eval[name][..., :2], full[..., :2])
    # a detection outside the ground-truth set is an error, not a silent drop
    bad = dict(d)
    bad["classes"] = d["classes"].copy()
    bad["classes"][5] = K
    with pytest.raises(ValueError, match="outside the ground-truth set"):
        _run(_scorer(bad, I, K, dev))


class _Replay(torch.nn.Module):
    """a model that returns recorded detections as device Instances"""

    def __init__(self, per_image, size, dev):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1, device=dev))
        self.per_image, self.size, self.dev = per_image, size, dev

    def forward(self, inputs):
        from detectron2_centernet_amd.structures import Boxes, Instances
        out = []
        for inp in inputs:
            b, s, c = self.per_image[inp["image_id"]]
            inst = Instances(self.size)
            inst.pred_boxes = Boxes(torch.as_tensor(b).to(self.dev))
            inst.scores = torch.as_tensor(s).to(self.dev)
            inst.pred_classes = torch.as_tensor(c).to(self.dev).long()
            out.append({"instances": inst})
        return out


def test_g22_through_the_evaluator_in_shuffled_order(tmp_path, dev):
    from detectron2_centernet_amd.data.coco import register_coco_instances
    d = np.load(G22)
    ids = [int(v) for v in d["image_ids"]]
    K = d["precision"].shape[2]
    cat = lambda k: 10 + 3 * k      # noqa: E731   non-contiguous category ids; the last one has no annotation
    coco = {"images": [{"id": i, "width": 640, "height": 480, "file_name": f"{i}.png"} for i in reversed(ids)],
            "categories": [{"id": cat(k), "name": f"c{k}"} for k in reversed(range(K))],
            "annotations": _annotations(d, cat_of=cat, img_of=lambda i: ids[i])}
    (tmp_path / "g22.json").write_text(json.dumps(coco))
    name = f"g22_json_{os.getpid()}_{tmp_path.name}"
    register_coco_instances(name, {"thing_classes": [f"c{k}" for k in range(K)],
                                   "thing_dataset_id_to_contiguous_id": {cat(k): k for k in range(K)}}, str(tmp_path / "g22.json"), "")
    per_image = {}
    for i, img_id in enumerate(ids):
        sel = np.where(d["image"] == i)[0]
        per_image[img_id] = (d["boxes"][sel], d["scores"][sel], d["classes"][sel])
    order = np.random.default_rng(5).permutation(len(ids))
    loader = [[{"image_id": ids[j]} for j in order[b:b + 5]] for b in range(0, len(ids), 5)]
    ev = COCOEvaluator(name, None, False, str(tmp_path / "out"))
    res = inference_on_dataset(_Replay(per_image, (480, 640), dev), loader, ev)
    assert np.array_equal(ev.coco_eval.eval["precision"], d["precision"])
    assert np.array_equal(ev.coco_eval.eval["recall"], d["recall"])
    assert np.array_equal(ev.coco_eval.eval["scores"], d["scores_out"])
    stats = CR.summarize(d["precision"], d["recall"])
    assert list(res) == ["bbox"] and list(res["bbox"]) == KEYS + [f"AP-c{k}" for k in range(K)]
    for j, key in enumerate(KEYS):
        assert res["bbox"][key] == stats[j] * 100
    assert math.isnan(res["bbox"][f"AP-c{K - 1}"]) and all(0 < res["bbox"][f"AP-c{k}"] < 100 for k in range(K - 1))
    recs = json.load(open(tmp_path / "out" / "coco_instances_results.json"))
    assert len(recs) == len(d["scores"]) and {r["category_id"] for r in recs} <= {cat(k) for k in range(K)}
    assert {r["image_id"] for r in recs} == {ids[i] for i in set(d["image"].tolist())}
    # a second evaluator fed in another order returns the same dict
    order2 = order[::-1]
    ev2 = COCOEvaluator(name, None, False)
    res2 = inference_on_dataset(_Replay(per_image, (480, 640), dev), [[{"image_id": ids[j]} for j in order2[b:b + 7]]
                                                                      for b in range(0, len(ids), 7)], ev2)
    assert json.dumps(res2) == json.dumps(res)


def test_large_cell_and_large_category_against_the_restatement(dev):
    """what G22 does not reach: a category with more than 100 000 detections (hundreds of chunks per accumulate workgroup), a
    300-ground-truth cell and non-default parameters (A*T = 4 matchers: that cell's `taken` table is 1 200 bytes and still in
    LDS -- the workspace path is the next test's)"""
    rng = np.random.default_rng(7)
    I, K = 1040, 2
    gt_rows, dt_rows = [], []
    for i in range(I):
        ng = 300 if i == 17 else int(rng.integers(0, 4))
        for _ in range(ng):
            w, h = rng.uniform(8, 120, 2)
            x, y = rng.uniform(0, 500, 2)
            box = np.round([x, y, w, h], 1)
            gt_rows.append((i, 0, box, float(box[2] * box[3] * rng.uniform(0.5, 1.0)), int(rng.random() < 0.1)))
        mine = [r for r in gt_rows[-ng:]] if ng else []
        for n in range(100 if i != 17 else 130):
            if mine and rng.random() < 0.5:
                b = mine[int(rng.integers(0, len(mine)))][2] * (1 + rng.normal(0, 0.06, 4))
                sc = rng.uniform(0.2, 1.0)
            else:
                b = np.concatenate([rng.uniform(0, 500, 2), rng.uniform(8, 120, 2)])
                sc = rng.uniform(0.0, 0.7)
            dt_rows.append((i, 0 if n < 98 or i == 17 else 1, b, float(np.round(sc, 2))))
    for i in range(0, I, 9):
        gt_rows.append((i, 1, np.array([10.0, 10.0, 40.0, 40.0]), 1600.0, 0))
    perm = rng.permutation(len(dt_rows))
    b = np.array([dt_rows[p][2] for p in perm])
    d = {"boxes": np.stack([b[:, 0], b[:, 1], b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]], 1).astype(np.float32),
         "scores": np.array([dt_rows[p][3] for p in perm], dtype=np.float32),
         "classes": np.array([dt_rows[p][1] for p in perm], dtype=np.int32),
         "image": np.array([dt_rows[p][0] for p in perm], dtype=np.int32),
         "gt_boxes": np.array([r[2] for r in gt_rows]), "gt_area": np.array([r[3] for r in gt_rows]),
         "gt_crowd": np.array([r[4] for r in gt_rows], dtype=np.uint8), "gt_image": np.array([r[0] for r in gt_rows], dtype=np.int32),
         "gt_classes": np.array([r[1] for r in gt_rows], dtype=np.int32)}
    assert (d["classes"] == 0).sum() > 100000
    ev = _scorer(d, I, K, dev)
    ev.params.iouThrs = np.array([0.5, 0.75])
    ev.params.recThrs = np.linspace(0, 1, 11)
    ev.params.areaRng = [[0, 1e10], [0, 60 ** 2]]
    ev.params.areaRngLbl = ["all", "small"]
    ev.params.maxDets = [1, 10, 100]
    ev.evaluate()
    ev.accumulate()
    want = CR.evaluate(d["boxes"], d["scores"], d["classes"], d["image"], d["gt_boxes"], d["gt_area"], d["gt_crowd"], d["gt_image"],
                       d["gt_classes"], I, K, iou_thrs=ev.params.iouThrs, rec_thrs=ev.params.recThrs, max_dets=ev.params.maxDets,
                       area_rngs=ev.params.areaRng)
    assert want[0].shape == (2, 11, 2, 2, 3) and (want[0] > 0).any() and (want[0] < 1).any()
    assert np.array_equal(ev.eval["precision"], want[0])
    assert np.array_equal(ev.eval["recall"], want[1])
    assert np.array_equal(ev.eval["scores"], want[2])


def test_cells_whose_taken_table_is_in_the_workspace(dev):
    """G per cell is not bounded: with the default 4 x 10 matchers a cell of more than 204 ground truths has a `taken` table
    (G * A*T bytes) beyond the matcher's LDS bound and keeps it in the caller's workspace at gt_off[cell] * A*T.  Three such
    cells (300, 260 and 230 ground truths: two categories of one image and a later image, so the offsets are non-zero and
    differ) among small ones, default parameters, against the restatement, exact"""
    import re
    src = open(os.path.join(os.path.dirname(HERE), "detectron2-centernet_amd", "csrc", "cocoeval.hip")).read()
    lds_bound = int(re.search(r"#define CE_LDS_TAKEN (\d+)", src).group(1))
    rng = np.random.default_rng(13)
    I, K = 6, 3
    big = {(1, 0): 300, (1, 2): 260, (4, 1): 230}
    gt_rows, dt_rows = [], []
    for i in range(I):
        for k in range(K):
            ng = big.get((i, k), int(rng.integers(0, 5)))
            mine = []
            for _ in range(ng):
                box = np.round(np.concatenate([rng.uniform(0, 560, 2), rng.uniform(8, 120, 2)]), 1)
                mine.append(box)
                gt_rows.append((i, k, box, float(box[2] * box[3] * rng.uniform(0.4, 1.0)), int(rng.random() < 0.1)))
            for n in range(120 if (i, k) in big else int(rng.integers(0, 12))):      # 120 > maxDets[-1]: the cut applies too
                if mine and rng.random() < 0.7:
                    b = mine[int(rng.integers(0, len(mine)))] * (1 + rng.normal(0, 0.06, 4))
                    sc = rng.uniform(0.2, 1.0)
                else:
                    b = np.concatenate([rng.uniform(0, 560, 2), rng.uniform(8, 120, 2)])
                    sc = rng.uniform(0.0, 0.7)
                dt_rows.append((i, k, b, float(np.round(sc, 2))))
    perm = rng.permutation(len(dt_rows))
    b = np.array([dt_rows[p][2] for p in perm])
    d = {"boxes": np.stack([b[:, 0], b[:, 1], b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]], 1).astype(np.float32),
         "scores": np.array([dt_rows[p][3] for p in perm], dtype=np.float32),
         "classes": np.array([dt_rows[p][1] for p in perm], dtype=np.int32),
         "image": np.array([dt_rows[p][0] for p in perm], dtype=np.int32),
         "gt_boxes": np.array([r[2] for r in gt_rows]), "gt_area": np.array([r[3] for r in gt_rows]),
         "gt_crowd": np.array([r[4] for r in gt_rows], dtype=np.uint8), "gt_image": np.array([r[0] for r in gt_rows], dtype=np.int32),
         "gt_classes": np.array([r[1] for r in gt_rows], dtype=np.int32)}
    ev = _scorer(d, I, K, dev)
    AT = len(ev.params.areaRng) * len(ev.params.iouThrs)
    assert AT == 40 and all(g * AT > lds_bound for g in big.values()) and 4 * AT <= lds_bound      # both paths, in one launch
    off = ev._gt["off"]
    assert sorted(int(off[c + 1] - off[c]) for c in range(I * K))[-3:] == [230, 260, 300] and off[1 * K + 0] > 0
    precision, recall, scores = _run(ev)
    want = CR.evaluate(d["boxes"], d["scores"], d["classes"], d["image"], d["gt_boxes"], d["gt_area"], d["gt_crowd"], d["gt_image"],
                       d["gt_classes"], I, K)
    assert (want[0] > 0).any() and (want[0][want[0] > -1] < 1).any() and (want[1] > 0.3).any()
    assert np.array_equal(precision, want[0])
    assert np.array_equal(recall, want[1])
    assert np.array_equal(scores, want[2])


def test_perfect_detections_score_100(dev):
    """detections equal to the ground-truth boxes of a crowd-free set (integer coordinates, exact in f32), through the catalog
    path of the evaluator (area = box area): every reported metric is 100"""
    from detectron2_centernet_amd.data.catalog import DatasetCatalog, MetadataCatalog
    from detectron2_centernet_amd.structures import BoxMode
    rng = np.random.default_rng(11)
    K, recs, per_image = 3, [], {}
    for i in range(12):
        n = int(rng.integers(3, 30))
        side = np.array([rng.choice([12, 50, 150]) + int(rng.integers(0, 10)) for _ in range(n)], dtype=np.float64)
        side[:3] = [14, 55, 160]            # every image holds a small, a medium and a large box
        xy = np.stack([np.arange(n) * 7.0 + rng.integers(0, 3, n), rng.integers(0, 300, n).astype(np.float64)], 1)
        boxes = np.concatenate([xy, xy + side[:, None] + np.array([0.0, 3.0])], 1)
        cls = np.arange(n) % K
        recs.append({"file_name": f"{i}", "image_id": 100 - i, "height": 600, "width": 600, "annotations": [
            {"bbox": boxes[j].tolist(), "bbox_mode": BoxMode.XYXY_ABS, "category_id": int(cls[j])} for j in range(n)]})
        per_image[100 - i] = (boxes.astype(np.float32), rng.uniform(0.1, 1, n).astype(np.float32), cls.astype(np.int64))
    name = f"cocoeval_perfect_{os.getpid()}"
    if name not in DatasetCatalog:
        DatasetCatalog.register(name, lambda: recs)
        MetadataCatalog.get(name).set(thing_classes=["a", "b", "c"])
    ev = COCOEvaluator(name, None, False)
    res = inference_on_dataset(_Replay(per_image, (600, 600), dev), [[{"image_id": r["image_id"]}] for r in recs], ev)
    assert list(res["bbox"]) == KEYS + ["AP-a", "AP-b", "AP-c"]
    assert all(v == 100.0 for v in res["bbox"].values()), res
    assert all(v == 1.0 for v in ev.coco_eval.stats[7:]), ev.coco_eval.stats       # AR@10 on: every ground truth found


def _synthetic_eval_set(name, n_images, size, num_classes):
    """catalog records with the boxes of `synthetic_sample` as annotations"""
    from detectron2_centernet_amd.data.catalog import DatasetCatalog, MetadataCatalog, synthetic_sample
    from detectron2_centernet_amd.structures import BoxMode
    samples = [synthetic_sample(i, size=size, num_classes=num_classes, max_boxes=8) for i in range(n_images)]
    if name not in DatasetCatalog:
        recs = [{"file_name": f"synthetic://{name}/{i}", "image_id": i, "height": size, "width": size, "annotations": [
            {"bbox": b.tolist(), "bbox_mode": BoxMode.XYXY_ABS, "category_id": int(c)} for b, c in zip(s["boxes"], s["classes"])]}
            for i, s in enumerate(samples)]
        DatasetCatalog.register(name, lambda: recs)
        MetadataCatalog.get(name).set(thing_classes=[f"class_{i}" for i in range(num_classes)])
    return samples


def test_real_model_through_the_evaluator_flip_on_and_off(tmp_path, dev):
    from detectron2_centernet_amd.modeling import CenterNetWithTTA
    from test_model_gpu import make_model
    model, cfg = make_model(tmp_path, "f16x3", seed=6)
    model.score_threshold = 0.0
    model.wh[-1].bias.data.fill_(6.0)
    name = f"cocoeval_synth_{os.getpid()}"
    samples = _synthetic_eval_set(name, 8, 128, 80)
    loader = [[{"image": samples[i + j]["image"], "image_id": i + j, "height": 128, "width": 128} for j in range(2)]
              for i in range(0, 8, 2)]
    written = {}
    for flip in (False, True):
        tcfg = cfg.clone()
        tcfg.TEST.AUG.ENABLED, tcfg.TEST.AUG.MIN_SIZES, tcfg.TEST.AUG.FLIP = True, (), flip
        ev = COCOEvaluator(name, cfg, False, str(tmp_path / f"out{int(flip)}"))
        tta = CenterNetWithTTA(tcfg, model)
        res = inference_on_dataset(tta, loader, ev)
        assert list(res) == ["bbox"] and list(res["bbox"])[:6] == KEYS and len(res["bbox"]) == 6 + 80
        assert all(math.isfinite(res["bbox"][k]) and 0.0 <= res["bbox"][k] <= 100.0 for k in KEYS), res["bbox"]
        assert ev.coco_eval.eval["precision"].shape == (10, 101, 80, 4, 3)
        recs = json.load(open(tmp_path / f"out{int(flip)}" / "coco_instances_results.json"))
        assert 0 < len(recs) <= 8 * 100 and {r["image_id"] for r in recs} == set(range(8))
        # what was scored and written is what the model returns for these batches (graph replays are bit-identical)
        with torch.no_grad():
            want = [r for batch in loader for inp, out in zip(batch, tta(batch))
                    for r in instances_to_coco_json(out["instances"], inp["image_id"])]
        assert recs == want
        assert ev.coco_eval._dt[1].numel() == len(want)
        assert torch.equal(ev.coco_eval._dt[1].cpu(), torch.tensor([r["score"] for r in want]))
        written[flip] = recs
        print("flip", flip, {k: round(res["bbox"][k], 4) for k in KEYS})
    assert written[True] != written[False]              # the flip test reached the evaluator: other detections
    model.train()


def coco_scale_inputs(dev, **kw):
    """`cocoeval_ref.coco_scale_inputs` with the ground truth prepared and the detections on the device"""
    anns, boxes, scores, classes, image, I, K = CR.coco_scale_inputs(**kw)
    t = lambda a: torch.as_tensor(a).to(dev)      # noqa: E731
    return prepare_ground_truth(range(I), range(K), anns), t(boxes), t(scores), t(classes), t(image)


def test_coco_val_scale_completes_with_sane_results(dev):
    gt, boxes, scores, classes, image = coco_scale_inputs(dev)
    assert 30000 < len(gt["area"]) < 45000 and scores.numel() == 500000
    ev = COCOevalHIP(gt, boxes, scores, classes, image)
    precision, recall, sc = _run(ev)
    assert precision.shape == (10, 101, 80, 4, 3) and (precision > -1).all()            # every (category, area) has ground truth
    assert precision.max() <= 1.0 and precision.min() >= 0.0 and recall.max() <= 1.0 and recall.min() >= 0.0
    assert (np.diff(precision, axis=1) <= 0).all()                # the envelope: non-increasing in the recall threshold
    assert (np.diff(recall, axis=0) <= 0).all()                   # a stricter IoU threshold never finds more
    assert (np.diff(recall, axis=-1) >= 0).all()                  # more detections per image never find less
    live = sc > 0
    assert ((np.diff(sc, axis=1) <= 0) | ~live[:, 1:]).all()      # the sampled scores descend along the curve
    assert (precision[sc == 0] == 0).all()                        # no detection reaches the threshold: 0 / 0
    s = ev.stats
    assert all(0.0 < v < 1.0 for v in s), s          # partial matches everywhere: strictly inside
    assert s[1] > s[0] > s[2] * 0.5 and s[6] < s[7] <= s[8]
    print("COCO-val scale stats:", np.round(s, 4))
