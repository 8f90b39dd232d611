"""COCO box-AP scoring, the parts that need no GPU: the numpy restatement (tests/cocoeval_ref.py) against the G22 fixture (the
reference's native scorer), hand-derived answers for the summary, ground-truth preparation, the result dict, the new entry
points of the shared library (argument checks through the label dry run, host addresses standing in for device pointers),
the refusals and the rank gather of `COCOEvaluator`."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

import cocoeval_ref as CR
from detectron2_centernet_amd import _lib
from detectron2_centernet_amd.evaluation import (COCOEvaluator, COCOevalHIP, Params, convert_to_coco_dict, derive_coco_results,
                                                 load_coco_ground_truth, prepare_ground_truth, summarize_stats)

HERE = os.path.dirname(os.path.abspath(__file__))
G22 = os.path.join(HERE, "golden", "g22_cocoeval.npz")
_BUF = C.create_string_buffer(1024)
BASE = (C.addressof(_BUF) + 255) & ~255       # a 256-byte aligned address to stand in for every device pointer
NEW = ("ctdet_cocoeval_workspace_bytes", "ctdet_cocoeval_iou", "ctdet_cocoeval_match", "ctdet_cocoeval_accumulate")


def _g22_eval(d, **kw):
    return CR.evaluate(d["boxes"], d["scores"], d["classes"], d["image"], d["gt_boxes"], d["gt_area"], d["gt_crowd"], d["gt_image"],
                       d["gt_classes"], len(d["image_ids"]), d["precision"].shape[2], **kw)


def test_restatement_equals_the_reference_on_g22():
    d = np.load(G22)
    precision, recall, scores = _g22_eval(d)
    assert precision.shape == d["precision"].shape == (10, 101, 6, 4, 3)
    assert np.array_equal(precision, d["precision"])
    assert np.array_equal(recall, d["recall"])
    assert np.array_equal(scores, d["scores_out"])
    # and the IoUs the reference was fed are the restatement's
    dx = CR.det_xywh(d["boxes"])
    for c, (i, k) in enumerate(d["iou_cells"]):
        ds = np.where((d["image"] == i) & (d["classes"] == k))[0]
        gs = np.where((d["gt_image"] == i) & (d["gt_classes"] == k))[0]
        want = d["iou_flat"][d["iou_off"][c]:d["iou_off"][c + 1]].reshape(len(ds), len(gs))
        assert np.array_equal(CR.iou(dx[ds], d["gt_boxes"][gs], d["gt_crowd"][gs]), want)
    # the two summaries (the test oracle's and the package's) agree, and the fixture is in the informative range
    stats = summarize_stats(d["precision"], d["recall"], Params())
    assert np.array_equal(stats, CR.summarize(d["precision"], d["recall"]))
    assert all(0.05 <= s <= 0.95 for s in stats[:6])
    assert (d["precision"] == -1).mean() == pytest.approx(1 / 6)


def _one_image(dets, gts):
    """dets: (x, y, w, h, score); gts: (x, y, w, h, area, crowd) -- one image, one class"""
    b = np.array([[x, y, x + w, y + h] for x, y, w, h, _ in dets], dtype=np.float32)
    g = np.array([r[:4] for r in gts], dtype=np.float64)
    z = np.zeros(len(dets), dtype=np.int32)
    p, r, _ = CR.evaluate(b, np.array([d[4] for d in dets], dtype=np.float32), z, z, g, np.array([r[4] for r in gts]),
                          np.array([r[5] for r in gts]), np.zeros(len(gts), int), np.zeros(len(gts), int), 1, 1)
    return summarize_stats(p, r, Params())


def test_known_answer_two_hits_around_a_false_positive():
    """scores .9 (hit, IoU 1), .8 (no overlap), .7 (hit): tp 1 1 2, fp 0 1 1; recall .5 .5 1; precision 1 .5 2/3, envelope
    1 2/3 2/3.  Recall thresholds 0 .. 0.50 (51 of them) sample index 0, the other 50 index 2: AP = (51 + 50 * 2/3) / 101 at
    every IoU threshold.  Both ground truths are medium (area 2500)."""
    s = _one_image([(0, 0, 50, 50, .9), (300, 300, 50, 50, .8), (100, 100, 50, 50, .7)],
                   [(0, 0, 50, 50, 2500, 0), (100, 100, 50, 50, 2500, 0)])
    ap = (51 + 50 * 2 / 3) / 101
    assert s[0] == pytest.approx(ap, abs=1e-15) and s[1] == pytest.approx(ap, abs=1e-15) and s[2] == pytest.approx(ap, abs=1e-15)
    assert s[3] == -1 and s[4] == pytest.approx(ap, abs=1e-15) and s[5] == -1
    assert list(s[6:9]) == [0.5, 1.0, 1.0]          # AR@1 sees only the first detection
    assert s[9] == -1 and s[10] == 1.0 and s[11] == -1


def test_known_answer_iou_between_two_thresholds():
    """one 10x10 ground truth, one 10x6.2 detection inside it: IoU 0.62, a hit at 0.5 / 0.55 / 0.6 and a miss at the other
    seven thresholds: AP = 0.3, AP50 = 1, AP75 = 0; small object"""
    s = _one_image([(0, 0, 10, 6.2, .5)], [(0, 0, 10, 10, 100, 0)])
    assert s[0] == pytest.approx(0.3, abs=1e-15) and s[1] == 1.0 and s[2] == 0.0
    assert s[3] == pytest.approx(0.3, abs=1e-15) and s[4] == -1 and s[5] == -1
    assert s[8] == pytest.approx(0.3, abs=1e-15)


def test_known_answer_crowd_match_is_not_a_false_positive():
    """the best-scored detection lies inside a crowd region (IoU = inter / det area = 1): matched to the crowd, ignored, not a
    false positive; the second equals the one regular ground truth: AP = 1 (it would be 0.5 with the first counted)"""
    s = _one_image([(110, 110, 10, 10, .9), (0, 0, 10, 10, .8)], [(0, 0, 10, 10, 100, 0), (100, 100, 50, 50, 2500, 1)])
    assert s[0] == 1.0 and s[3] == 1.0 and s[4] == -1 and s[8] == 1.0
    # AR@1 takes the first detection of the cell only -- the ignored one: recall 0
    assert s[6] == 0.0


def _small_json():
    return {"images": [{"id": 30, "width": 64, "height": 48, "file_name": "c.png"}, {"id": 10, "width": 64, "height": 48, "file_name": "a.png"},
                       {"id": 20, "width": 64, "height": 48, "file_name": "b.png"}],
            "categories": [{"id": 7, "name": "seven"}, {"id": 3, "name": "three"}, {"id": 90, "name": "ninety"}],
            "annotations": [
                {"id": 5, "image_id": 30, "category_id": 90, "bbox": [1, 2, 10, 20], "area": 123.5, "iscrowd": 0},
                {"id": 6, "image_id": 10, "category_id": 7, "bbox": [3, 4, 5, 6], "area": 17.0, "iscrowd": 1},
                {"id": 7, "image_id": 30, "category_id": 3, "bbox": [0, 0, 8, 8], "area": 60.0, "iscrowd": 0},
                {"id": 8, "image_id": 30, "category_id": 90, "bbox": [2, 2, 4, 4], "area": 9.0}]}


def test_ground_truth_from_a_coco_json(tmp_path):
    (tmp_path / "gt.json").write_text(json.dumps(_small_json()))
    gt, names, has = load_coco_ground_truth(str(tmp_path / "gt.json"))
    assert has and names == ["three", "seven", "ninety"]
    assert gt["image_ids"] == [10, 20, 30] and gt["cat_ids"] == [3, 7, 90]           # image 20 has no annotation
    assert gt["off"].dtype == np.int32 and len(gt["off"]) == 3 * 3 + 1
    assert gt["off"].tolist() == [0, 0, 1, 1, 1, 1, 1, 2, 2, 4]
    assert gt["area"].tolist() == [17.0, 60.0, 123.5, 9.0]                            # the `area` field, not w * h
    assert gt["crowd"].tolist() == [1, 0, 0, 0] and gt["boxes"].dtype == np.float64
    assert gt["boxes"].tolist() == [[3, 4, 5, 6], [0, 0, 8, 8], [1, 2, 10, 20], [2, 2, 4, 4]]   # input order within a cell
    d = _small_json()
    del d["annotations"]
    assert load_coco_ground_truth(d)[2] is False


def _register_records(name):
    from detectron2_centernet_amd.data.catalog import DatasetCatalog, MetadataCatalog
    from detectron2_centernet_amd.structures import BoxMode
    if name not in DatasetCatalog:
        recs = [{"file_name": "a", "image_id": 4, "height": 100, "width": 100, "annotations": [
                    {"bbox": [10.0, 20.0, 30.5, 60.0], "bbox_mode": BoxMode.XYXY_ABS, "category_id": 1},
                    {"bbox": [1.0, 2.0, 3.0, 4.0], "bbox_mode": BoxMode.XYWH_ABS, "category_id": 0, "iscrowd": 1}]},
                {"file_name": "b", "image_id": 2, "height": 100, "width": 100}]
        DatasetCatalog.register(name, lambda: recs)
        MetadataCatalog.get(name).set(thing_classes=["x", "y"])
    return name


def test_ground_truth_from_catalog_records():
    d = convert_to_coco_dict(_register_records("cocoeval_host_records"))
    assert [c["id"] for c in d["categories"]] == [0, 1] and [im["id"] for im in d["images"]] == [4, 2]
    a0, a1 = d["annotations"]
    assert a0 == {"id": 1, "image_id": 4, "bbox": [10.0, 20.0, 20.5, 40.0], "area": 820.0, "iscrowd": 0, "category_id": 1}
    assert a1 == {"id": 2, "image_id": 4, "bbox": [1.0, 2.0, 3.0, 4.0], "area": 12.0, "iscrowd": 1, "category_id": 0}
    ev = COCOEvaluator("cocoeval_host_records", distributed=False)
    assert ev._gt["image_ids"] == [2, 4] and ev._gt["off"].tolist() == [0, 0, 0, 1, 2] and ev._lut == [0, 1]
    assert ev._gt["area"].tolist() == [12.0, 820.0]


def test_result_dict_keys_and_nan():
    precision = -np.ones((10, 101, 3, 4, 3))
    precision[:, :, 0, 0, :] = 0.5
    precision[:, :, 0, 2, :] = 0.25
    precision[:5, :, 1, 0, :] = 1.0
    recall = -np.ones((10, 3, 4, 3))
    stats = summarize_stats(precision, recall, Params())
    res = derive_coco_results(stats, precision, ["a", "b", "c"])
    assert list(res) == ["AP", "AP50", "AP75", "APs", "APm", "APl", "AP-a", "AP-b", "AP-c"]
    assert res["AP"] == pytest.approx(100 * (10 * 0.5 + 5 * 1.0) / 15) and res["AP50"] == pytest.approx(75.0)
    assert res["AP75"] == pytest.approx(50.0)
    assert math.isnan(res["APs"]) and res["APm"] == pytest.approx(25.0) and math.isnan(res["APl"])
    assert res["AP-a"] == pytest.approx(50.0) and res["AP-b"] == pytest.approx(100.0) and math.isnan(res["AP-c"])
    assert list(derive_coco_results(stats, precision, ["only"][:1])) == ["AP", "AP50", "AP75", "APs", "APm", "APl"]
    none = derive_coco_results(None, None, ["a", "b"])
    assert list(none) == ["AP", "AP50", "AP75", "APs", "APm", "APl"] and all(math.isnan(v) for v in none.values())
    assert list(stats[6:]) == [-1.0] * 6


def test_params_are_cocos_and_settable():
    p = Params()
    assert np.array_equal(p.iouThrs, CR.IOU_THRS) and len(p.iouThrs) == 10 and np.array_equal(p.recThrs, CR.REC_THRS)
    assert p.maxDets == [1, 10, 100] and p.areaRng == [[0, 1e10], [0, 1024], [1024, 9216], [9216, 1e10]] and p.useCats == 1
    p.maxDets, p.iouThrs = [5, 50, 500], np.array([0.3])
    assert p.maxDets[-1] == 500


def test_new_symbols_and_abi_version():
    L = _lib.lib()
    assert L.ctdet_abi_version() == 8
    raw = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(os.path.dirname(HERE), "include", "ctdet_hip.h")).read()
    for name in NEW:
        assert hasattr(raw, name) and name in _lib.SIGNATURES and name + "(" in header, name
    mk = open(os.path.join(os.path.dirname(HERE), "detectron2-centernet_amd", "csrc", "Makefile")).read()
    assert "cocoeval.hip" in mk and "FLAGS_cocoeval := -ffp-contract=off" in mk


def test_workspace_formula():
    L = _lib.lib()
    up = lambda v: (v + 255) // 256 * 256      # noqa: E731

    def want(N, NG, I, K, A, T):
        return (2 * up(8 * N) + 2 * up(4 * N) + up(4 * (max(I * K, K) + 2)) + up(NG * A * T) + up(16 * N + (16 << 20)))
    for args in ((0, 0, 1, 1, 1, 1), (2111, 401, 48, 6, 4, 10), (500000, 37000, 5000, 80, 4, 10)):
        assert L.ctdet_cocoeval_workspace_bytes(*args) == want(*args), args
    assert L.ctdet_cocoeval_workspace_bytes(500000, 37000, 5000, 80, 4, 10) < 64 << 20
    assert L.ctdet_cocoeval_workspace_bytes(10, 10, 5, 5, 7, 10) == 0 and b"64 lanes" in L.ctdet_last_error()
    assert L.ctdet_cocoeval_workspace_bytes(-1, 0, 1, 1, 1, 1) == 0
    assert L.ctdet_cocoeval_workspace_bytes(10, 0, 1 << 20, 1 << 12, 4, 10) == 0


def _match(N=10, NG=5, I=2, K=3, T=10, A=4, max_det=100, null=None, ws=None):
    p = [C.c_void_p(BASE)] * 16
    if null is not None:
        p[null] = None
    return _lib.lib().ctdet_cocoeval_match(p[0], p[1], p[2], p[3], N, p[4], p[5], p[6], p[7], NG, I, K, p[8], T, p[9], A, max_det,
                                           C.c_void_p(BASE if ws is None else ws), p[10], p[11], p[12], p[13], p[14], None)


def _accum(N=10, K=3, A=4, T=10, R=101, M=3, max_det=100, null=None):
    p = [C.c_void_p(BASE)] * 12
    if null is not None:
        p[null] = None
    return _lib.lib().ctdet_cocoeval_accumulate(p[0], p[1], p[2], p[3], p[4], p[5], N, K, A, T, p[6], R, p[7], M, max_det,
                                                C.c_void_p(BASE), p[8], p[9], p[10], None)


def test_entry_points_in_a_dry_run():
    L = _lib.lib()
    p = C.c_void_p(BASE)
    assert L.ctdet_set_label_mode(2) == 0
    try:
        assert _match() == 0, L.ctdet_last_error()
        assert L.ctdet_last_kernel_label().decode() == "ce_match_kernel<wave per cell,40 matchers>"
        assert _match(T=2, A=2) == 0 and L.ctdet_last_kernel_label().decode() == "ce_match_kernel<wave per cell,4 matchers>"
        assert _match(N=0, NG=0) == 0                       # an empty set of detections is a valid input
        assert _match(T=13, A=5) != 0 and b"64 lanes" in L.ctdet_last_error()
        assert _match(max_det=0) != 0 and b"max_det" in L.ctdet_last_error()
        assert _match(I=0) != 0 and _match(K=0) != 0 and _match(N=-1) != 0 and _match(N=1 << 31) != 0
        assert _match(I=1 << 16, K=1 << 15) != 0 and b"out of range" in L.ctdet_last_error()
        # one workgroup per cell: the grid limit bounds I*K
        assert _match(I=1 << 13, K=1 << 13) != 0 and b"2^26" in L.ctdet_last_error()
        assert _match(I=(1 << 13) - 1, K=1 << 13) == 0, L.ctdet_last_error()
        assert _match(ws=BASE + 16) != 0 and b"aligned" in L.ctdet_last_error()
        for null in (0, 3, 4, 7, 8, 9, 10, 12, 13, 14):
            assert _match(null=null) != 0 and b"null" in L.ctdet_last_error(), null
        assert _accum() == 0, L.ctdet_last_error()
        assert L.ctdet_last_kernel_label().decode() == "ce_accum_kernel<workgroup per (k,a,m,t),two passes>"
        assert _accum(N=0) == 0
        assert _accum(R=0) != 0 and _accum(R=5000) != 0 and b"recall thresholds" in L.ctdet_last_error()
        assert _accum(max_det=0) != 0 and b"max_det" in L.ctdet_last_error()
        assert _accum(M=0) != 0 and _accum(T=65, A=1) != 0 and _accum(K=0) != 0
        for null in (0, 2, 4, 5, 6, 7, 8, 9, 10):
            assert _accum(null=null) != 0 and b"null" in L.ctdet_last_error(), null
        assert L.ctdet_cocoeval_iou(p, 3, p, p, 4, p, None) == 0
        assert L.ctdet_last_kernel_label().decode() == "ce_iou_kernel<f64,contract off>"
        assert L.ctdet_cocoeval_iou(p, 0, p, p, 4, p, None) == 0
        assert L.ctdet_cocoeval_iou(p, -1, p, p, 4, p, None) != 0
        assert L.ctdet_cocoeval_iou(p, 3, None, p, 4, p, None) != 0 and b"null" in L.ctdet_last_error()
    finally:
        L.ctdet_set_label_mode(0)


def _cpu_instances(n=2):
    from detectron2_centernet_amd.structures import Boxes, Instances
    inst = Instances((48, 64))
    inst.pred_boxes = Boxes(torch.tensor([[1.0, 2.0, 4.0, 6.0]] * n))
    inst.scores = torch.full((n,), 0.5)
    inst.pred_classes = torch.zeros(n, dtype=torch.int64)
    return inst


def test_refusals(tmp_path):
    from detectron2_centernet_amd.config import get_cfg
    name = _register_records("cocoeval_host_records")
    with pytest.raises(NotImplementedError, match="segm"):
        COCOEvaluator(name, tasks=("bbox", "segm"))
    with pytest.raises(NotImplementedError, match="keypoints"):
        COCOEvaluator(name, tasks=("keypoints",))
    cfg = get_cfg()
    assert COCOEvaluator(name, cfg)._tasks == ("bbox",)
    ev = COCOEvaluator(name, distributed=False)
    with pytest.raises(NotImplementedError, match="proposals"):
        ev.process([{"image_id": 4}], [{"proposals": object()}])
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        ev.process([{"image_id": 4}], [{"instances": _cpu_instances()}])
    gt = prepare_ground_truth([1], [1], [])
    z = torch.zeros(0)
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        COCOevalHIP(gt, z.reshape(0, 4), z, z.int(), z.int())
    with pytest.raises(NotImplementedError, match="bbox"):
        Params("segm")
    # no predictions at all: the warning and {}
    assert ev.evaluate() == {}


def test_rank_gather(monkeypatch):
    """two ranks: the main process concatenates every rank's arrays in rank order, the other rank returns {} from evaluate()"""
    from detectron2_centernet_amd.evaluation import coco_evaluation as CE
    ev = COCOEvaluator(_register_records("cocoeval_host_records"), distributed=True)
    mine = ([4], [2], torch.tensor([[1.0, 2, 3, 4], [5, 6, 7, 8]]), torch.tensor([0.5, 0.25]), torch.tensor([0, 1], dtype=torch.int32))
    other = ([2, 4], [1, 0], np.array([[0, 0, 9, 9]], dtype=np.float32), np.array([0.75], dtype=np.float32), np.array([1], dtype=np.int32))
    empty = ([], [], None, None, None)
    sent = []

    def gather(data, dst=0):
        sent.append(data)
        return [data, other, empty]
    monkeypatch.setattr(CE.comm, "get_world_size", lambda: 3)
    monkeypatch.setattr(CE.comm, "synchronize", lambda: None)
    monkeypatch.setattr(CE.comm, "gather", gather)
    monkeypatch.setattr(CE.comm, "is_main_process", lambda: True)
    ids, counts, boxes, scores, classes = ev._gather(mine)
    assert ids == [4, 2, 4] and counts == [2, 1, 0]
    assert isinstance(sent[0][2], np.ndarray)                       # what travels is host data
    assert boxes.tolist() == [[1, 2, 3, 4], [5, 6, 7, 8], [0, 0, 9, 9]] and scores.tolist() == [0.5, 0.25, 0.75]
    assert classes.tolist() == [0, 1, 1] and classes.dtype == np.int32
    monkeypatch.setattr(CE.comm, "is_main_process", lambda: False)
    monkeypatch.setattr(CE.comm, "gather", lambda data, dst=0: [])
    assert ev._gather(mine) is None
    monkeypatch.setattr(ev, "_local", lambda: mine)
    assert ev.evaluate() == {}
    # not distributed: the local tensors, untouched
    ev2 = COCOEvaluator("cocoeval_host_records", distributed=False)
    assert ev2._gather(mine) is mine


def test_unknown_image_id_is_an_error(monkeypatch):
    """a prediction for an image outside the ground-truth set is refused on the host, before anything reaches the device"""
    ev = COCOEvaluator(_register_records("cocoeval_host_records"), distributed=False)
    mine = ([4, 999], [1, 1], torch.tensor([[1.0, 2, 3, 4], [5, 6, 7, 8]]), torch.tensor([0.5, 0.25]), torch.tensor([0, 1], dtype=torch.int32))
    monkeypatch.setattr(ev, "_local", lambda: mine)
    with pytest.raises(ValueError, match=r"image ids that are not in the ground-truth set: \[999\]"):
        ev.evaluate()


def test_results_records_share_the_wire_format():
    from detectron2_centernet_amd.evaluation import instances_to_coco_json
    from detectron2_centernet_amd.evaluation.coco_results import coco_records
    inst = _cpu_instances(2)
    inst.pred_boxes.tensor[1] = torch.tensor([0.1, 0.2, 10.7, 20.9])
    want = instances_to_coco_json(inst, 17)
    for r in want:
        r["category_id"] = 1000 + r["category_id"]
    got = coco_records(inst.pred_boxes.tensor.numpy(), inst.scores.numpy(), inst.pred_classes.numpy(), [17, 17], {0: 1000})
    assert got == want
