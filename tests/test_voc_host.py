"""Pascal VOC scoring without a GPU: the numpy restatement of the rule (tests/voc_cases.py) against the reference's recorded
results (tests/golden/g23_voceval.npz, written by tests/golden/make_g23.py) and against hand-derived answers, the quantisation
against Python's formatting, the XML loader and the registration on a synthetic tree, the entry points of the scorer's
own library (argument checks through the label dry run, host addresses standing in for device pointers), the evaluator's
refusals and the trainer's dispatch on `evaluator_type`."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import voc_cases as VC
from detectron2_centernet_amd import _lib
from detectron2_centernet_amd.data import (CLASS_NAMES, DatasetCatalog, MetadataCatalog, load_voc_instances,
                                           register_all_pascal_voc, register_pascal_voc)
from detectron2_centernet_amd.evaluation import (COCOEvaluator, PascalVOCDetectionEvaluator, VOCevalHIP, derive_voc_results,
                                                 flatten_results_dict, parse_voc_ground_truth, print_csv_format)
from detectron2_centernet_amd.structures import BoxMode

HERE = os.path.dirname(os.path.abspath(__file__))
G23 = os.path.join(HERE, "golden", "g23_voceval.npz")
_BUF = C.create_string_buffer(1024)
BASE = (C.addressof(_BUF) + 255) & ~255       # a 256-byte aligned address to stand in for every device pointer
NEW = ("ctdet_voceval_workspace_bytes", "ctdet_voceval_match", "ctdet_voceval_ap")


def g23_inputs(g):
    objects = [(int(i), int(k), int(d), [int(v) for v in b])
               for i, k, d, b in zip(g["gt_image"], g["gt_classes"], g["gt_difficult"], g["gt_boxes"])]
    return VC.make_gt(len(g["image_ids"]), len(g["class_names"]), objects), g["boxes"], g["scores"], g["classes"], g["image"]


@pytest.fixture(scope="module")
def g23():
    g = np.load(G23)
    return g, VC.voc_score(*g23_inputs(g))


# ---- the restatement against the reference
def test_restatement_equals_the_reference_on_g23(g23):
    g, r = g23
    assert np.array_equal(r["cls_off"], g["cls_off"])
    # rec, prec and the 11-point AP bit for bit (NaN where a class has detections and no non-difficult ground truth)
    assert np.array_equal(r["rec"], g["rec"], equal_nan=True) and np.isnan(g["rec"]).any()
    assert np.array_equal(r["prec"], g["prec"])
    assert np.array_equal(r["ap07"], g["ap07"])
    # the area AP: the same bit-equal terms of total <= 1, summed in position order here and pairwise by numpy there
    assert np.array_equal(np.isnan(r["ap12"]), np.isnan(g["ap12"])) and np.isnan(g["ap12"]).sum() == g["ap12"].shape[1]
    ok = ~np.isnan(g["ap12"])
    bound = VC.area_bound(r["terms"])
    assert np.all(np.abs(r["ap12"] - g["ap12"])[ok] <= bound[ok])
    assert r["terms"].max() > 8        # numpy sums blocks of 8: the two orders do differ
    K, T = g["ap12"].shape
    for k in range(K):
        for t in range(T):
            sl = slice(r["cls_off"][k], r["cls_off"][k + 1])
            if ok[k, t]:
                assert abs(r["ap12"][k, t] - VC.fsum_area(r["rec"][t, sl], r["prec"][t, sl])) <= bound[k, t]


def test_result_dict_equals_the_reference_on_g23(g23):
    g, r = g23
    names = [str(n) for n in g["class_names"]]
    for tag, table in (("res07", g["ap07"]), ("res12", g["ap12"])):
        res = derive_voc_results(table, names)
        assert list(res) == ["bbox", "bbox_AP", "bbox_AP50", "bbox_AP75"] and list(res["bbox"]) == ["AP", "AP50", "AP75"]
        assert np.array_equal([res["bbox"][m] for m in ("AP", "AP50", "AP75")], g[tag + "_bbox"], equal_nan=True)
        for key in ("bbox_AP", "bbox_AP50", "bbox_AP75"):
            assert list(res[key]) == names
            assert np.array_equal([res[key][n] for n in names], g[tag + "_" + key], equal_nan=True), key
    assert np.isnan(g["res12_bbox"]).all() and not np.isnan(g["res07_bbox"]).any()      # one NaN class poisons the 2012 means


def test_result_dict_goes_through_the_trainers_consumers(g23, caplog):
    """the nested per-class dicts: csv log lines, and the flattening the EvalHook stores"""
    g, _ = g23
    res = derive_voc_results(g["ap07"], [str(n) for n in g["class_names"]])
    with caplog.at_level("INFO"):
        print_csv_format(res)
    text = caplog.text
    assert "copypaste: Task: bbox_AP50" in text and "copypaste: AP,AP50,AP75" in text and "aeroplane,bicycle" in text
    flat = flatten_results_dict(res)
    assert len(flat) == 3 + 3 * len(g["class_names"]) and "bbox_AP75/bird" in flat and "bbox/AP" in flat
    assert all(isinstance(float(v), float) for v in flat.values())


# ---- quantisation
def test_quantisation_equals_pythons_formatting():
    rng = np.random.default_rng(0)
    ties3 = ((2 * np.arange(0, 2000) + 1) / 2000.0).astype(np.float32)                   # (2k+1)/2000, exact or nearest f32
    s = np.concatenate([rng.random(20000).astype(np.float32), ties3, -ties3[:50], np.float32([0.0, -0.0, 1.0, 0.0005, 0.9995])])
    want = np.array([float(f"{v:.3f}") for v in s.tolist()])
    assert np.array_equal(VC.quantise_scores(s), want)
    ties1 = ((2 * np.arange(0, 4000) + 1) / 20.0).astype(np.float32)                     # x.05, x.15, ...; x.25 / x.75 are exact
    c = np.concatenate([rng.uniform(-50, 1500, 20000).astype(np.float32), ties1, np.arange(0, 500, 0.25, dtype=np.float32)])
    c = c[: len(c) // 4 * 4].reshape(-1, 4)
    plus1 = c.copy()
    plus1[:, :2] = plus1[:, :2] + np.float32(1)                                          # `xmin += 1` on an f32 scalar
    want = np.array([[float(f"{v:.1f}") for v in row] for row in plus1.tolist()])
    assert np.array_equal(VC.quantise_boxes(c), want)


# ---- hand-derived answers
def _score(objects, boxes, scores, classes, image, I, K, thr):
    return VC.voc_score(VC.make_gt(I, K, objects), np.float32(boxes), np.float32(scores), np.int32(classes), np.int32(image), thr)


def test_known_answer_tied_scores_the_input_index_decides():
    """two images, one ground truth each; a hit in image 1 and a miss in image 0 with scores that tie after quantisation.
    Input order (miss, hit): FP then TP, prec = [0, 1/2]; input order (hit, miss): TP then FP, prec = [1, 1/2]."""
    objects = [(0, 0, 0, [11, 11, 50, 50]), (1, 0, 0, [11, 11, 50, 50])]
    hit, miss = [10, 10, 50, 50], [200, 200, 240, 240]
    a = _score(objects, [miss, hit], [0.5004, 0.4996], [0, 0], [0, 1], 2, 1, [0.5])
    assert a["order"].tolist() == [0, 1] and a["flags"][:, 0].tolist() == [2, 1]
    assert a["rec"][0].tolist() == [0.0, 0.5] and a["prec"][0].tolist() == [0.0, 0.5]
    assert a["ap07"][0, 0] == sum([0.5 / 11.0] * 6) and a["ap12"][0, 0] == 0.25
    b = _score(objects, [hit, miss], [0.4996, 0.5004], [0, 0], [1, 0], 2, 1, [0.5])
    assert b["order"].tolist() == [0, 1] and b["flags"][:, 0].tolist() == [1, 2]
    assert b["prec"][0].tolist() == [1.0, 0.5] and b["ap12"][0, 0] == 0.5
    # scores that differ after quantisation: the higher one first, whatever the input order
    c = _score(objects, [miss, hit], [0.4994, 0.5006], [0, 0], [0, 1], 2, 1, [0.5])
    assert c["order"].tolist() == [1, 0] and c["prec"][0].tolist() == [1.0, 0.5]


def test_known_answer_overlap_exactly_at_the_threshold():
    """raw box [0,0,10,20] -> [1,1,10,20] (200 pixels) on ground truth [1,1,10,10] (100 pixels): overlap 100 / 200 = 0.5
    exactly; `>` is strict: a true positive under 0.45, a false positive under 0.5"""
    r = _score([(0, 0, 0, [1, 1, 10, 10])], [[0, 0, 10, 20]], [0.9], [0], [0], 1, 1, [0.45, 0.5])
    assert r["flags"][0].tolist() == [1, 2]
    ap = 0.0
    for _ in range(11):
        ap = ap + 1.0 / 11.0
    assert r["ap07"][0].tolist() == [ap, 0.0] and r["ap12"][0].tolist() == [1.0, 0.0]


def test_known_answer_identical_boxes_the_difficult_one_first():
    """two identical ground-truth boxes, the first difficult: argmax takes the first, so every detection on them is neither
    a true nor a false positive, and the non-difficult twin is never found: AP 0 with npos = 1"""
    objects = [(0, 0, 1, [11, 11, 50, 50]), (0, 0, 0, [11, 11, 50, 50])]
    r = _score(objects, [[10, 10, 50, 50], [10, 10, 50, 50]], [0.9, 0.8], [0, 0], [0, 0], 1, 1, [0.5])
    assert r["flags"][:, 0].tolist() == [0, 0] and r["npos"].tolist() == [1]
    assert r["rec"][0].tolist() == [0.0, 0.0] and r["prec"][0].tolist() == [0.0, 0.0] and r["ap07"][0, 0] == 0.0 == r["ap12"][0, 0]
    # the other way round the first detection takes the non-difficult one, the second is a duplicate: FP
    r = _score(objects[::-1], [[10, 10, 50, 50], [10, 10, 50, 50]], [0.9, 0.8], [0, 0], [0, 0], 1, 1, [0.5])
    assert r["flags"][:, 0].tolist() == [1, 2] and r["prec"][0].tolist() == [1.0, 0.5]


def test_known_answer_first_detection_on_a_difficult_box():
    """tp + fp = 0 at the first position: prec = 0 / eps = 0, not 0 / 0"""
    objects = [(0, 0, 1, [11, 11, 50, 50]), (0, 0, 0, [101, 101, 150, 150])]
    r = _score(objects, [[10, 10, 50, 50], [100, 100, 150, 150]], [0.9, 0.8], [0, 0], [0, 0], 1, 1, [0.5])
    assert r["flags"][:, 0].tolist() == [0, 1]
    assert r["rec"][0].tolist() == [0.0, 1.0] and r["prec"][0].tolist() == [0.0, 1.0]
    assert r["ap12"][0, 0] == 1.0


def test_known_answer_class_without_positives():
    r = _score([(0, 1, 1, [11, 11, 50, 50])], [[10, 10, 50, 50]], [0.9], [1], [0], 1, 3, [0.5])
    assert r["ap07"][:, 0].tolist() == [0.0, 0.0, 0.0]
    assert r["ap12"][0, 0] == 0.0 and np.isnan(r["ap12"][1, 0]) and r["ap12"][2, 0] == 0.0


# ---- the loader and the registration
OBJ = ("<object><name>{}</name><difficult>{}</difficult><bndbox><xmin>{}</xmin><ymin>{}</ymin><xmax>{}</xmax><ymax>{}</ymax>"
       "</bndbox></object>")


def write_voc_tree(root, images, split="test"):
    """images: {id: (width, height, [(name, difficult, xmin, ymin, xmax, ymax)])}"""
    os.makedirs(os.path.join(root, "ImageSets", "Main"), exist_ok=True)
    os.makedirs(os.path.join(root, "Annotations"), exist_ok=True)
    os.makedirs(os.path.join(root, "JPEGImages"), exist_ok=True)
    with open(os.path.join(root, "ImageSets", "Main", split + ".txt"), "w") as f:
        f.write("".join(i + "\n" for i in images))
    for i, (w, h, objs) in images.items():
        with open(os.path.join(root, "Annotations", i + ".xml"), "w") as f:
            f.write(f"<annotation><size><width>{w}</width><height>{h}</height><depth>3</depth></size>"
                    + "".join(OBJ.format(*o) for o in objs) + "</annotation>")


TREE = {"000005": (500, 375, [("chair", 0, 263, 211, 324, 339), ("chair", 1, 5, 244, 67, 374), ("dog", 0, 1, 1, 500, 375)]),
        "000007": (480, 360, []),
        "000009": (300, 200, [("tvmonitor", 0, 10, 20, 110, 120)])}


def test_loader_on_a_synthetic_tree(tmp_path):
    root = str(tmp_path / "VOC2007")
    write_voc_tree(root, TREE)
    recs = load_voc_instances(root, "test", CLASS_NAMES)
    assert [r["image_id"] for r in recs] == list(TREE) and recs[0]["file_name"] == os.path.join(root, "JPEGImages", "000005.jpg")
    assert (recs[0]["height"], recs[0]["width"]) == (375, 500) and recs[1]["annotations"] == []
    a = recs[0]["annotations"]
    assert [x["category_id"] for x in a] == [8, 8, 11] and all(x["bbox_mode"] == BoxMode.XYXY_ABS for x in a)
    assert a[0]["bbox"] == [262.0, 210.0, 324.0, 339.0] and a[2]["bbox"] == [0.0, 0.0, 500.0, 375.0]      # difficult ones included
    gt = parse_voc_ground_truth(root, "test", CLASS_NAMES)
    assert gt["image_ids"] == list(TREE) and gt["off"].shape == (3 * 20 + 1,) and gt["off"][-1] == 4
    assert gt["boxes"].dtype == np.float64 and gt["boxes"].tolist() == [[263, 211, 324, 339], [5, 244, 67, 374], [1, 1, 500, 375],
                                                                        [10, 20, 110, 120]]                # 1-based, unmodified
    assert gt["difficult"].tolist() == [0, 1, 0, 0] and gt["classes"].tolist() == [8, 8, 11, 19] and gt["image"].tolist() == [0, 0, 0, 2]
    assert gt["off"][8] == 0 and gt["off"][9] == 2 and gt["off"][12] == 3
    assert len(CLASS_NAMES) == 20 and list(CLASS_NAMES) == sorted(CLASS_NAMES)


def test_registration(tmp_path):
    import detectron2_centernet_amd.data  # noqa: F401  (nothing registers at import)
    from detectron2_centernet_amd.data.pascal_voc import VOC_SPLITS
    assert len(VOC_SPLITS) == 7 and not [n for n, _, _, _ in VOC_SPLITS if n in DatasetCatalog]
    root = str(tmp_path)
    assert register_all_pascal_voc(root) == []                     # no VOC2007 / VOC2012 directory: nothing is registered
    write_voc_tree(os.path.join(root, "VOC2007"), TREE)
    try:
        added = register_all_pascal_voc(root)
        assert added == ["voc_2007_trainval", "voc_2007_train", "voc_2007_val", "voc_2007_test"]
        assert "voc_2012_val" not in DatasetCatalog
        meta = MetadataCatalog.get("voc_2007_test")
        assert (meta.year, meta.split, meta.dirname, meta.evaluator_type) == (2007, "test", os.path.join(root, "VOC2007"),
                                                                             "pascal_voc")
        assert meta.thing_classes == list(CLASS_NAMES)
        assert len(DatasetCatalog.get("voc_2007_test")) == 3
        os.makedirs(os.path.join(root, "VOC2012"))
        assert register_all_pascal_voc(root) == ["voc_2012_trainval", "voc_2012_train", "voc_2012_val"]
        assert MetadataCatalog.get("voc_2012_val").year == 2012
    finally:
        for n in [n for n, _, _, _ in VOC_SPLITS if n in DatasetCatalog]:
            DatasetCatalog.remove(n)
            MetadataCatalog.remove(n)


# ---- the shared library
def test_new_symbols_and_abi_version():
    """the scorer is a library of its own: the hot-path library, its header and its ABI version are the parent's"""
    L, V = _lib.lib(), _lib.voceval_lib()
    assert L.ctdet_abi_version() == 8
    raw, main = C.CDLL(_lib.VOCEVAL_LIB_PATH), C.CDLL(_lib.LIB_PATH)
    root = os.path.dirname(HERE)
    header = open(os.path.join(root, "include", "ctdet_voceval.h")).read()
    main_header = open(os.path.join(root, "include", "ctdet_hip.h")).read()
    for name in NEW:
        assert hasattr(raw, name) and hasattr(V, name) and name in _lib.VOCEVAL_SIGNATURES and name + "(" in header, name
        assert not hasattr(main, name) and name not in _lib.SIGNATURES and name not in main_header, name
    assert len(_lib.VOCEVAL_SIGNATURES["ctdet_voceval_match"][1]) == 20 and len(_lib.VOCEVAL_SIGNATURES["ctdet_voceval_ap"][1]) == 14
    mk = open(os.path.join(root, "detectron2-centernet_amd", "csrc", "Makefile")).read()
    assert "libctdet_voceval.so" in mk and "FLAGS_voceval := -ffp-contract=off" in mk and "$(FLAGS_voceval)" in mk
    srcs = [l for l in mk.splitlines() if l.startswith("SRCS")][0]
    assert "voceval.hip" not in srcs


def test_workspace_formula():
    L, V = _lib.lib(), _lib.voceval_lib()
    up = lambda v: (v + 255) // 256 * 256      # noqa: E731

    def want(N, NG, I, K, T):
        return (up(8 * T * (N // 256 + K + 1)) + 2 * up(8 * N) + 5 * up(4 * N) + up(4 * (I * K + 2)) + up(4 * NG)
                + up(16 * N + (16 << 20)))
    for args in ((0, 0, 1, 1, 1), (160, 127, 24, 5, 10), (495200, 15000, 4952, 20, 10)):
        assert V.ctdet_voceval_workspace_bytes(*args) == want(*args), args
    assert V.ctdet_voceval_workspace_bytes(495200, 15000, 4952, 20, 10) < 64 << 20
    assert V.ctdet_voceval_workspace_bytes(10, 10, 5, 5, 33) == 0 and b"T=33" in L.ctdet_last_error()
    assert V.ctdet_voceval_workspace_bytes(-1, 0, 1, 1, 1) == 0
    assert V.ctdet_voceval_workspace_bytes(10, 0, 1 << 20, 1 << 12, 10) == 0


MATCH_POINTERS = ("boxes", "scores", "classes", "image", "gt_boxes", "gt_difficult", "gt_off", "thrs", "workspace", "order",
                  "cls_off", "flags", "npos", "status")
AP_POINTERS = ("order", "cls_off", "flags", "npos", "points", "workspace", "ap07", "ap12", "rec", "prec")


def _match(N=10, NG=5, I=2, K=3, T=10, null=None, ws=None):
    p = {n: C.c_void_p(BASE) for n in MATCH_POINTERS}
    if ws is not None:
        p["workspace"] = C.c_void_p(ws)
    if null is not None:
        p[null] = None
    return _lib.voceval_lib().ctdet_voceval_match(p["boxes"], p["scores"], p["classes"], p["image"], N, p["gt_boxes"], p["gt_difficult"],
                                          p["gt_off"], NG, I, K, p["thrs"], T, p["workspace"], p["order"], p["cls_off"],
                                          p["flags"], p["npos"], p["status"], None)


def _ap(N=10, K=3, T=10, null=(), ws=None):
    p = {n: C.c_void_p(BASE) for n in AP_POINTERS}
    if ws is not None:
        p["workspace"] = C.c_void_p(ws)
    for n in null:
        p[n] = None
    return _lib.voceval_lib().ctdet_voceval_ap(p["order"], p["cls_off"], p["flags"], p["npos"], N, K, T, p["points"], p["workspace"],
                                       p["ap07"], p["ap12"], p["rec"], p["prec"], None)


def test_entry_points_in_a_dry_run():
    L = _lib.lib()
    assert L.ctdet_set_label_mode(2) == 0
    try:
        assert _match() == 0, L.ctdet_last_error()
        assert L.ctdet_last_kernel_label().decode() == "ve_match_kernel<wave per cell,10 thresholds>"
        assert _match(T=1) == 0 and L.ctdet_last_kernel_label().decode() == "ve_match_kernel<wave per cell,1 thresholds>"
        assert _match(T=32) == 0
        assert _match(T=33) != 0 and b"T=33" in L.ctdet_last_error()          # one bit of a taken word per threshold
        assert _match(T=0) != 0
        # an empty set of detections, or of ground truths, is a valid input, with no buffer for it
        assert _match(N=0, null="boxes") == 0 and _match(NG=0, null="gt_boxes") == 0
        assert _match(I=0) != 0 and _match(K=0) != 0 and _match(N=-1) != 0 and _match(N=1 << 31) != 0 and _match(NG=-1) != 0
        assert b"ground truths out of range" in L.ctdet_last_error()
        assert _match(NG=1 << 31) != 0
        # one wave per cell: the grid limit bounds I*K
        assert _match(I=1 << 13, K=1 << 13) != 0 and b"2^26" in L.ctdet_last_error()
        assert _match(I=(1 << 13) - 1, K=1 << 13) == 0, L.ctdet_last_error()
        assert _match(ws=BASE + 16) != 0 and b"aligned" in L.ctdet_last_error()
        for null in MATCH_POINTERS:
            assert _match(null=null) != 0, null
            assert ("null pointer " + null).encode() in L.ctdet_last_error(), (null, L.ctdet_last_error())
        assert _ap() == 0, L.ctdet_last_error()
        assert L.ctdet_last_kernel_label().decode() == "ve_ap_kernel<workgroup per (k,t),two passes>"
        assert _ap(null=("rec", "prec")) == 0                                  # rec / prec are optional
        assert _ap(N=0, null=("order", "flags")) == 0
        assert _ap(T=33) != 0 and b"T=33" in L.ctdet_last_error()
        assert _ap(K=0) != 0 and _ap(N=-1) != 0 and _ap(T=0) != 0
        assert _ap(ws=BASE + 8) != 0 and b"aligned" in L.ctdet_last_error()
        for null in AP_POINTERS[:8]:
            assert _ap(null=(null,)) != 0, null
            assert ("null pointer " + null).encode() in L.ctdet_last_error(), (null, L.ctdet_last_error())
    finally:
        L.ctdet_set_label_mode(0)


# ---- the evaluator
def _cpu_instances(n=2):
    from detectron2_centernet_amd.structures import Boxes, Instances
    inst = Instances((48, 64))
    inst.pred_boxes = Boxes(torch.tensor([[1.0, 2.0, 4.0, 6.0]] * n))
    inst.scores = torch.full((n,), 0.5)
    inst.pred_classes = torch.zeros(n, dtype=torch.int64)
    return inst


@pytest.fixture
def voc_set(tmp_path):
    root = str(tmp_path / "VOC2007")
    write_voc_tree(root, TREE)
    register_pascal_voc("voc_host_2007_test", root, "test", 2007)
    register_pascal_voc("voc_host_1999_test", root, "test", 1999)
    yield "voc_host_2007_test"
    for n in ("voc_host_2007_test", "voc_host_1999_test"):
        DatasetCatalog.remove(n)
        MetadataCatalog.remove(n)


def test_evaluator_refusals(voc_set, monkeypatch):
    with pytest.raises(AssertionError, match="1999"):
        PascalVOCDetectionEvaluator("voc_host_1999_test")
    with pytest.raises(ValueError, match="register_pascal_voc"):
        PascalVOCDetectionEvaluator("voc_host_not_a_voc_set")
    MetadataCatalog.remove("voc_host_not_a_voc_set")
    ev = PascalVOCDetectionEvaluator(voc_set, distributed=False)
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        ev.process([{"image_id": "000005"}], [{"instances": _cpu_instances()}])
    gt = parse_voc_ground_truth(MetadataCatalog.get(voc_set).dirname, "test", CLASS_NAMES)
    z = torch.zeros(0)
    with pytest.raises(NotImplementedError, match="`boxes` must be a tensor on the GPU"):
        VOCevalHIP(gt, z.reshape(0, 4), z, z.int(), z.int())
    # no predictions at all: every AP is 0, as the reference's empty class files give
    res = ev.evaluate()
    assert list(res) == ["bbox", "bbox_AP", "bbox_AP50", "bbox_AP75"] and res["bbox"] == {"AP": 0.0, "AP50": 0.0, "AP75": 0.0}
    assert list(res["bbox_AP"]) == list(CLASS_NAMES) and set(res["bbox_AP50"].values()) == {0.0}
    # a prediction for an image outside the split is refused on the host, before anything reaches the device
    mine = (["000005", "123456"], [1, 1], torch.zeros(2, 4), torch.zeros(2), torch.zeros(2, dtype=torch.int32))
    monkeypatch.setattr(ev, "_local", lambda: mine)
    with pytest.raises(ValueError, match=r"not in ImageSets/Main/test.txt: \['123456'\]"):
        ev.evaluate()


def test_evaluator_on_another_rank_returns_none(voc_set, monkeypatch):
    from detectron2_centernet_amd.evaluation import coco_evaluation as CE
    ev = PascalVOCDetectionEvaluator(voc_set)
    monkeypatch.setattr(CE.comm, "get_world_size", lambda: 2)
    monkeypatch.setattr(CE.comm, "synchronize", lambda: None)
    monkeypatch.setattr(CE.comm, "gather", lambda data, dst=0: [])
    monkeypatch.setattr(CE.comm, "is_main_process", lambda: False)
    assert ev.evaluate() is None


def test_status_word_names_the_cause():
    from detectron2_centernet_amd.evaluation.voceval import status_message
    assert status_message(1) == "a class index outside [0, K)" and "image index" in status_message(2)
    assert "score" in status_message(4) and "box coordinate" in status_message(8)
    assert status_message(5).count(";") == 1


def test_build_evaluator_dispatches_on_the_evaluator_type(voc_set, tmp_path):
    from detectron2_centernet_amd.config import get_cfg
    from detectron2_centernet_amd.data.catalog import register_synthetic_files
    from detectron2_centernet_amd.engine import DefaultTrainer
    cfg = get_cfg()
    cfg.OUTPUT_DIR = str(tmp_path / "out")
    ev = DefaultTrainer.build_evaluator(cfg, voc_set)
    assert type(ev) is PascalVOCDetectionEvaluator and ev._year == 2007 and ev._distributed
    register_synthetic_files("voc_host_plain_records", str(tmp_path / "png"), length=2, size=32, num_classes=3)
    try:
        assert MetadataCatalog.get("voc_host_plain_records").get("evaluator_type") is None
        assert type(DefaultTrainer.build_evaluator(cfg, "voc_host_plain_records")) is COCOEvaluator       # no type: as before
        MetadataCatalog.get("voc_host_plain_records").evaluator_type = "coco"
        assert type(DefaultTrainer.build_evaluator(cfg, "voc_host_plain_records")) is COCOEvaluator
    finally:
        DatasetCatalog.remove("voc_host_plain_records")
        MetadataCatalog.remove("voc_host_plain_records")
