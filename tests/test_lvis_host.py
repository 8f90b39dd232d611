"""LVIS on the host: the numpy restatement of the rule (tests/lvis_cases.py) against tests/cocoeval_ref.py where LVIS coincides
with COCO and against hand-derived answers; the json loader, its metadata and refusals; the evaluator's paths that need no
device; the trainer's dispatch; the library's argument checks in a dry run."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

import cocoeval_ref as CR
import lvis_cases as LC
from detectron2_centernet_amd import _lib
from detectron2_centernet_amd.data import (DatasetCatalog, MetadataCatalog, load_lvis_json, register_all_lvis,
                                           register_lvis_instances)
from detectron2_centernet_amd.evaluation import (COCOEvaluator, LVISEvaluator, LVISevalHIP, prepare_lvis_ground_truth,
                                                 summarize_lvis)
from detectron2_centernet_amd.structures import BoxMode

HERE = os.path.dirname(os.path.abspath(__file__))
BASE = 1 << 20         # a 256-byte aligned address that is never dereferenced: the dry run returns before any launch


# ---- the restatement where LVIS coincides with COCO
def test_restatement_reduces_to_the_coco_scorer():
    """every class negative everywhere, nothing not exhaustive, no `ignore`, at most 300 detections per image: the federated
    rule is COCO's with maxDets = [300] and no crowd.  The precision formulas differ only where tp + fp = 1 (for an integer
    n >= 2, n + 2^-52 rounds to n): by 1 - 1 / (1 + 2^-52) <= 2^-52 at a lone leading true positive, by nothing elsewhere."""
    gts = {(i, k): (2 * i + 3 * k) % 5 for i in range(6) for k in range(4)}
    dets = {(i, k): (5 * i + k) % 9 + (20 if (i, k) == (1, 2) else 0) for i in range(6) for k in range(4)}
    gt, boxes, scores, classes, image = LC.cells_case(21, 6, 4, gts, dets, ignore_share=0.0, neg_share=1.0, nel_share=0.0)
    gt["lists"][:] = LC.NEG
    assert not gt["ignore"].any() and np.bincount(image).max() <= 300 and (gt["area"] < 1024).any() and (gt["area"] > 1024).any()
    got = LC.lvis_score(gt, boxes, scores, classes, image)
    want, want_recall, _ = CR.evaluate(boxes, scores, classes, image, gt["boxes"], gt["area"], np.zeros(len(gt["area"])), gt["image"],
                                       gt["classes"], 6, 4, iou_thrs=LC.IOU_THRS, rec_thrs=LC.REC_THRS, max_dets=[300],
                                       area_rngs=LC.AREA_RNGS)
    want, want_recall = want[..., 0], want_recall[..., 0]
    assert got["part"].all() and got["precision"].shape == want.shape == (10, 101, 4, 4)
    assert np.array_equal(got["recall"], want_recall)
    err = np.abs(got["precision"] - want)
    print(f"restatement vs cocoeval_ref: max |diff| = {err.max():.3e} (bound {2.0 ** -52:.3e}); "
          f"{int(got['first_tp'].sum())} of {got['first_tp'].size} (t, k, a) lead with a lone true positive")
    assert err.max() <= 2.0 ** -52
    exact = ~got["first_tp"]                                      # [T,K,A] -> over the recall axis
    assert exact.any() and got["first_tp"].any()
    assert np.array_equal(np.moveaxis(got["precision"], 1, -1)[exact], np.moveaxis(want, 1, -1)[exact])
    assert (want > 0).any() and (want == -1).any()


# ---- hand-derived answers (each derived in lvis_cases.hand_case)
@pytest.fixture(scope="module")
def hand():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = LC.lvis_score(*LC.hand_case(name))
        return cache[name]
    return get


def test_not_exhaustive_cell_ignores_the_unmatched_detection(hand):
    on, off = hand("nel_on"), hand("nel_off")
    assert np.all(on["precision"][:, :, 0, 0] == LC.ONE) and np.all(off["precision"][:, :, 0, 0] == 0.5)
    assert on["flags"][0, 0] == 2 and off["flags"][0, 0] == 0 and np.all(on["recall"][:, 0, 0] == 1.0)


def test_class_in_neither_list_takes_no_part(hand):
    a, b = hand("drop_with"), hand("drop_without")
    assert a["part"].tolist() == [False, True, True]
    for k in ("precision", "recall", "npig", "cls_off"):
        assert np.array_equal(a[k], b[k]), k
    assert np.all(a["precision"][:, :, 1, 0] == LC.ONE)


def test_negative_class_without_ground_truth_gives_false_positives(hand):
    assert np.all(hand("neg_on")["precision"][:, :, 0, 0] == 0.5)
    assert np.all(hand("neg_off")["precision"][:, :, 0, 0] == LC.ONE) and hand("neg_off")["part"].tolist() == [False, True]


def test_area_of_exactly_1024_is_small_and_medium(hand):
    r = hand("area_1024")
    assert r["npig"].tolist() == [[1, 1, 1, 0]]
    assert np.all(r["precision"][:, :, 0, :3] == LC.ONE) and np.all(r["precision"][:, :, 0, 3] == -1) and np.all(r["recall"][:, 0, 3] == -1)


def test_non_ignored_ground_truth_is_preferred_to_a_better_ignored_one(hand):
    r = hand("prefers_non_ignored")
    assert r["flags"][0, :10].tolist() == [1, 1, 1, 3, 3, 3, 3, 3, 3, 0]
    assert r["recall"][:, 0, 0].tolist() == [1.0] * 3 + [0.0] * 7
    assert np.all(r["precision"][:3, :, 0, 0] == LC.ONE) and not r["precision"][3:, :, 0, 0].any()


def test_iou_of_exactly_one_half_matches_at_one_half(hand):
    r = hand("iou_half")
    assert r["flags"][0, :10].tolist() == [1] + [0] * 9
    assert LC.iou_row(np.array([0.0, 0.0, 1.0, 1.0]), np.array([[0.0, 0.0, 2.0, 1.0]]))[0] == 0.5


def test_first_true_positive_has_precision_one_over_one_plus_epsilon(hand):
    assert LC.ONE == 1.0 / (1.0 + 2.0 ** -52) and LC.ONE < 1.0 and 1.0 - LC.ONE <= 2.0 ** -52
    assert np.all(hand("tie_in_cell")["precision"][:, :, 0, 0] == LC.ONE)


def test_score_ties_within_a_cell_and_across_images(hand):
    r = hand("tie_in_cell")
    assert r["flags"][:, 0].tolist() == [1, 0] and r["order"].tolist() == [0, 1]
    r = hand("tie_across_images")
    assert r["order"].tolist() == [1, 0] and np.all(r["precision"][:, :, 0, 0] == LC.ONE)


def test_the_301st_detection_of_an_image_is_cut(hand):
    cut, kept = hand("cut_301"), hand("cut_300")
    assert cut["part"].sum() == 300 and not cut["part"][300] and cut["part"][299]
    assert not cut["recall"][:, 0, 0].any() and not cut["precision"][:, :, 0, 0].any()
    assert kept["part"].all() and np.all(kept["recall"][:, 0, 0] == 1.0) and np.all(kept["precision"][:, :, 0, 0] == 1.0 / 300.0)


def test_summaries_leave_out_what_has_no_ground_truth():
    """K = 3 with frequencies r, c, f: class 0 scores 0.5 everywhere, class 1 scores 0.25, class 2 has no ground truth (-1): AP is
    the mean of the two, APr is class 0's alone, APf is -1; an area range that is -1 for every class is -1"""
    precision, recall = -np.ones((10, 101, 3, 4)), -np.ones((10, 3, 4))
    precision[:, :, 0, :2], precision[:, :, 1, 0] = 0.5, 0.25
    recall[:, 0, :2], recall[:, 1, 0] = 1.0, 0.5
    for fn in (LC.summarize, summarize_lvis):
        s = fn(precision, recall, ["r", "c", "f"])
        assert (s["AP"], s["AP50"], s["AP75"], s["APr"], s["APc"], s["APf"]) == (0.375, 0.375, 0.375, 0.5, 0.25, -1.0), fn
        assert (s["APs"], s["APm"], s["APl"]) == (0.5, -1.0, -1.0)
        assert (s["AR@300"], s["ARs@300"], s["ARm@300"], s["ARl@300"]) == (0.75, 1.0, -1.0, -1.0)
    precision[5, :, 0, 0] = 1.0                # AP75 is the threshold of index 5
    assert summarize_lvis(precision, recall, "rcf")["AP75"] == LC.summarize(precision, recall, "rcf")["AP75"] == 0.625


# ---- loader, metadata, registration
CATEGORIES = [{"id": 2, "name": "bun", "synonyms": ["bun", "roll"], "frequency": "c"},
              {"id": 1, "name": "aerosol_can", "synonyms": ["aerosol_can", "spray_can"], "frequency": "r"},
              {"id": 3, "name": "cup", "frequency": "f"}]
IMAGES = [{"id": 9, "height": 48, "width": 64, "coco_url": "http://images.cocodataset.org/val2017/000000000009.jpg",
           "neg_category_ids": [3], "not_exhaustive_category_ids": [2]},
          {"id": 4, "height": 32, "width": 40, "file_name": "plain/four.jpg"}]
ANNOTATIONS = [{"id": 1, "image_id": 9, "category_id": 2, "bbox": [1.0, 2.0, 10.0, 12.0], "area": 77.5,
                "segmentation": [[1, 2, 11, 2, 11, 14]]},
               {"id": 2, "image_id": 4, "category_id": 1, "bbox": [3.0, 4.0, 5.0, 6.0], "ignore": 1},
               {"id": 3, "image_id": 9, "category_id": 3, "bbox": [0.0, 0.0, 4.0, 4.0], "area": 16.0}]


def write_json(path, images=IMAGES, categories=CATEGORIES, annotations=ANNOTATIONS):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    data = {"images": images, "categories": categories}
    if annotations is not None:
        data["annotations"] = annotations
    with open(path, "w") as f:
        json.dump(data, f)
    return path


@pytest.fixture
def lvis_set(tmp_path):
    names = []

    def register(name, **kw):
        path = write_json(str(tmp_path / name / "lvis.json"), **kw)
        register_lvis_instances(name, {}, path, str(tmp_path / "coco"))
        names.append(name)
        return name
    yield register
    for n in names:
        DatasetCatalog.remove(n)
        MetadataCatalog.remove(n)


def test_loader_reads_both_file_name_forms_and_the_lists(lvis_set, tmp_path):
    name = lvis_set("lvis_host_val")
    meta = MetadataCatalog.get(name)
    assert meta.evaluator_type == "lvis" and not hasattr(meta, "thing_classes")       # nothing is read at registration
    recs = DatasetCatalog.get(name)
    root = str(tmp_path / "coco")
    assert [r["image_id"] for r in recs] == [4, 9]                                     # ascending image id
    assert recs[0]["file_name"] == os.path.join(root, "plain/four.jpg")
    assert recs[1]["file_name"] == os.path.join(root, "val2017", "000000000009.jpg")
    assert (recs[1]["height"], recs[1]["width"]) == (48, 64)
    assert recs[1]["neg_category_ids"] == [3] and recs[1]["not_exhaustive_category_ids"] == [2]
    assert recs[0]["neg_category_ids"] == [] and recs[0]["not_exhaustive_category_ids"] == []
    assert recs[1]["annotations"] == [{"bbox": [1.0, 2.0, 10.0, 12.0], "bbox_mode": BoxMode.XYWH_ABS, "category_id": 1},
                                      {"bbox": [0.0, 0.0, 4.0, 4.0], "bbox_mode": BoxMode.XYWH_ABS, "category_id": 2}]
    assert recs[0]["annotations"][0]["category_id"] == 0
    # the metadata comes from the json's categories: synonyms[0], else name, by ascending id; the frequency letters
    assert meta.thing_classes == ["aerosol_can", "bun", "cup"] and meta.class_frequency == "rcf"
    assert not hasattr(meta, "thing_dataset_id_to_contiguous_id")


def test_loader_refusals(tmp_path):
    twice = ANNOTATIONS + [dict(ANNOTATIONS[0])]
    with pytest.raises(ValueError, match="annotation ids in .* are not unique"):
        load_lvis_json(write_json(str(tmp_path / "a" / "x.json"), annotations=twice), "root")
    gap = [dict(CATEGORIES[0], id=5)] + CATEGORIES[1:]
    with pytest.raises(ValueError, match=r"category ids of .* are not 1 \.\. 3"):
        load_lvis_json(write_json(str(tmp_path / "b" / "x.json"), categories=gap), "root")
    stray = ANNOTATIONS[:2] + [dict(ANNOTATIONS[2], category_id=7)]
    with pytest.raises(ValueError, match="category id 7 outside 1 .. 3"):
        load_lvis_json(write_json(str(tmp_path / "c" / "x.json"), annotations=stray), "root")


def test_cocofied_set_maps_through_its_own_ids(lvis_set):
    cats = [{"id": 17, "name": "cat"}, {"id": 3, "name": "car"}]
    anns = [{"id": 1, "image_id": 4, "category_id": 17, "bbox": [0.0, 0.0, 4.0, 4.0], "area": 16.0}]
    name = lvis_set("lvis_host_val_cocofied", images=IMAGES[1:], categories=cats, annotations=anns)
    recs = DatasetCatalog.get(name)
    meta = MetadataCatalog.get(name)
    assert meta.thing_dataset_id_to_contiguous_id == {3: 0, 17: 1} and meta.thing_classes == ["car", "cat"]
    assert recs[0]["annotations"][0]["category_id"] == 1
    ev = LVISEvaluator(name, None, False)
    assert ev._category_ids() == [3, 17]
    assert LVISEvaluator(lvis_set("lvis_host_plain"), None, False)._category_ids() == [1, 2, 3]        # else: class index + 1


def test_register_all_lvis_registers_what_exists(tmp_path):
    from detectron2_centernet_amd.data.lvis import LVIS_SPLITS
    assert len(LVIS_SPLITS) == 10 and set(LVIS_SPLITS) >= {"lvis_v1_train", "lvis_v1_val", "lvis_v1_test_dev",
                                                           "lvis_v1_test_challenge", "lvis_v0.5_val_rand_100",
                                                           "lvis_v0.5_train_cocofied"}
    root = str(tmp_path / "datasets")
    before = set(DatasetCatalog.list())
    assert not any(n.startswith("lvis_") for n in before)                        # nothing registers at import
    assert register_all_lvis(root) == []
    write_json(os.path.join(root, "lvis", "lvis_v1_val.json"))
    try:
        assert register_all_lvis(root) == ["lvis_v1_val"]
        meta = MetadataCatalog.get("lvis_v1_val")
        assert (meta.evaluator_type, meta.json_file, meta.image_root) == ("lvis", os.path.join(root, "lvis", "lvis_v1_val.json"),
                                                                          os.path.join(root, "coco"))
        assert register_all_lvis(root) == []                                     # registered already: left alone
        assert len(DatasetCatalog.get("lvis_v1_val")) == 2
    finally:
        DatasetCatalog.remove("lvis_v1_val")
        MetadataCatalog.remove("lvis_v1_val")
    assert set(DatasetCatalog.list()) == before


def test_prepare_ground_truth_from_the_json():
    gt = prepare_lvis_ground_truth({"images": IMAGES, "categories": CATEGORIES, "annotations": ANNOTATIONS})
    assert gt["image_ids"] == [4, 9] and gt["cat_ids"] == [1, 2, 3] and gt["frequency"] == ["r", "c", "f"]
    assert gt["off"].tolist() == [0, 1, 1, 1, 1, 2, 3]
    assert gt["boxes"].tolist() == [[3.0, 4.0, 5.0, 6.0], [1.0, 2.0, 10.0, 12.0], [0.0, 0.0, 4.0, 4.0]]
    assert gt["area"].tolist() == [30.0, 77.5, 16.0]                              # the field; w * h where it is absent
    assert gt["ignore"].tolist() == [1, 0, 0]
    assert gt["lists"].tolist() == [[0, 0, 0], [0, LC.NEL, LC.NEG]]


# ---- the evaluator
def test_evaluator_paths_without_a_device(lvis_set, tmp_path, caplog):
    name = lvis_set("lvis_host_eval")
    out = str(tmp_path / "inference")
    ev = LVISEvaluator(name, None, False, out)
    assert ev._do_evaluation
    with caplog.at_level("WARNING"):
        assert ev.evaluate() == {}                                                # no predictions at all
    assert "Did not receive valid predictions" in caplog.text
    # predictions without a detection: every metric is NaN
    z = torch.zeros(0)
    ev._results = {}
    ev._eval_predictions([4, 9], [0, 0], z.reshape(0, 4), z, z.int())
    res = ev._results["bbox"]
    assert list(res) == ["AP", "AP50", "AP75", "APs", "APm", "APl", "APr", "APc", "APf"] and all(math.isnan(v) for v in res.values())
    assert json.load(open(os.path.join(out, "lvis_instances_results.json"))) == []
    # a json without annotations (a test set): the results file only, category ids as class index + 1
    ev = LVISEvaluator(lvis_set("lvis_host_test", annotations=None), None, False, out)
    assert not ev._do_evaluation
    ev._results = {}
    ev._eval_predictions([9], [2], torch.tensor([[1.0, 2.0, 4.0, 6.0]] * 2), torch.tensor([0.5, 0.25]), torch.tensor([0, 2], dtype=torch.int32))
    assert ev._results == {}
    assert json.load(open(os.path.join(out, "lvis_instances_results.json"))) == [
        {"image_id": 9, "category_id": 1, "bbox": [1.0, 2.0, 3.0, 4.0], "score": 0.5},
        {"image_id": 9, "category_id": 3, "bbox": [1.0, 2.0, 3.0, 4.0], "score": 0.25}]


def test_evaluator_refusals(lvis_set):
    from detectron2_centernet_amd.config import get_cfg
    from detectron2_centernet_amd.structures import Boxes, Instances
    name = lvis_set("lvis_host_refuse")
    cfg = get_cfg()
    cfg.MODEL.MASK_ON = True
    with pytest.raises(NotImplementedError, match="'segm' is not built"):
        LVISEvaluator(name, cfg, False)
    with pytest.raises(ValueError, match="register_lvis_instances"):
        LVISEvaluator("lvis_host_not_registered", None, False)
    MetadataCatalog.remove("lvis_host_not_registered")
    ev = LVISEvaluator(name, None, False)
    with pytest.raises(NotImplementedError, match="box proposals"):
        ev.process([{"image_id": 9}], [{"proposals": None}])
    inst = Instances((48, 64))
    inst.pred_boxes, inst.scores, inst.pred_classes = Boxes(torch.tensor([[1.0, 2.0, 4.0, 6.0]])), torch.ones(1), torch.zeros(1).long()
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        ev.process([{"image_id": 9}], [{"instances": inst}])
    z = torch.zeros(0)
    with pytest.raises(NotImplementedError, match="`boxes` must be a tensor on the GPU"):
        LVISevalHIP(ev._gt, z.reshape(0, 4), z, z.int(), z.int())


def test_status_word_names_the_cause():
    from detectron2_centernet_amd.evaluation.lviseval import status_message
    assert status_message(1) == "a class index outside [0, K)" and "image index" in status_message(2)
    assert "score" in status_message(4) and "box coordinate" in status_message(8)
    assert status_message(5).count(";") == 1


def test_build_evaluator_dispatches_lvis(lvis_set, tmp_path):
    from detectron2_centernet_amd.config import get_cfg
    from detectron2_centernet_amd.engine import DefaultTrainer
    cfg = get_cfg()
    cfg.OUTPUT_DIR = str(tmp_path / "out")
    name = lvis_set("lvis_host_dispatch", annotations=[ANNOTATIONS[0], ANNOTATIONS[2]])      # no `ignore`: COCO refuses the field
    ev = DefaultTrainer.build_evaluator(cfg, name)
    assert type(ev) is LVISEvaluator and ev._distributed and ev._output_dir == os.path.join(cfg.OUTPUT_DIR, "inference")
    MetadataCatalog.get(name).evaluator_type = "coco"
    assert type(DefaultTrainer.build_evaluator(cfg, name)) is COCOEvaluator


# ---- the library
def test_a_library_of_its_own():
    main, L = _lib.lib(), _lib.lviseval_lib()
    raw = C.CDLL(_lib.LVISEVAL_LIB_PATH)
    root = os.path.dirname(HERE)
    header = open(os.path.join(root, "include", "ctdet_lviseval.h")).read()
    main_header = open(os.path.join(root, "include", "ctdet_hip.h")).read()
    for name in ("ctdet_lviseval_workspace_bytes", "ctdet_lviseval_match", "ctdet_lviseval_accumulate"):
        assert hasattr(raw, name) and hasattr(L, name) and name in _lib.LVISEVAL_SIGNATURES and name + "(" in header, name
        assert not hasattr(main, name) and name not in _lib.SIGNATURES and name not in main_header, name
    assert len(_lib.LVISEVAL_SIGNATURES["ctdet_lviseval_match"][1]) == 25
    assert len(_lib.LVISEVAL_SIGNATURES["ctdet_lviseval_accumulate"][1]) == 13
    mk = open(os.path.join(root, "detectron2-centernet_amd", "csrc", "Makefile")).read()
    assert "libctdet_lviseval.so" in mk and "FLAGS_lviseval := -ffp-contract=off" in mk and "$(FLAGS_lviseval)" in mk
    assert "lviseval.hip" not in [l for l in mk.splitlines() if l.startswith("SRCS")][0]


def test_workspace_formula():
    L, V = _lib.lib(), _lib.lviseval_lib()
    up = lambda v: (v + 255) // 256 * 256      # noqa: E731

    def want(N, NG, I, K, A, T):
        return (2 * up(8 * N) + 5 * up(4 * N) + up(4 * (I * K + 2)) + up(4 * (I + 2)) + up(NG * A * T) + up(16 * N + (16 << 20)))
    for args in ((0, 0, 1, 1, 1, 1), (160, 127, 24, 5, 4, 10), (5942700, 244000, 19809, 1203, 4, 10)):
        assert V.ctdet_lviseval_workspace_bytes(*args) == want(*args), args
    assert V.ctdet_lviseval_workspace_bytes(10, 10, 5, 5, 7, 10) == 0 and b"A=7 area ranges x T=10" in L.ctdet_last_error()
    assert V.ctdet_lviseval_workspace_bytes(-1, 0, 1, 1, 1, 1) == 0
    assert V.ctdet_lviseval_workspace_bytes(10, 0, 1 << 20, 1 << 12, 4, 10) == 0 and b"2^26" in L.ctdet_last_error()


MATCH_POINTERS = ("boxes", "scores", "classes", "image", "gt_boxes", "gt_area", "gt_ignore", "gt_off", "lists", "iou_thrs",
                  "area_rngs", "workspace", "order", "cls_off", "flags", "npig", "status")
ACC_POINTERS = ("order", "cls_off", "flags", "npig", "rec_thrs", "precision", "recall")


def _match(N=10, NG=5, I=2, K=3, A=4, T=10, max_det=300, null=None, ws=None):
    p = {n: C.c_void_p(BASE) for n in MATCH_POINTERS}
    if ws is not None:
        p["workspace"] = C.c_void_p(ws)
    if null is not None:
        p[null] = None
    return _lib.lviseval_lib().ctdet_lviseval_match(
        p["boxes"], p["scores"], p["classes"], p["image"], N, p["gt_boxes"], p["gt_area"], p["gt_ignore"], p["gt_off"], NG,
        p["lists"], I, K, p["iou_thrs"], T, p["area_rngs"], A, max_det, p["workspace"], p["order"], p["cls_off"], p["flags"],
        p["npig"], p["status"], None)


def _acc(N=10, K=3, A=4, T=10, R=101, null=()):
    p = {n: C.c_void_p(BASE) for n in ACC_POINTERS}
    for n in null:
        p[n] = None
    return _lib.lviseval_lib().ctdet_lviseval_accumulate(p["order"], p["cls_off"], p["flags"], p["npig"], N, K, A, T, p["rec_thrs"], R,
                                                         p["precision"], p["recall"], None)


def test_entry_points_in_a_dry_run():
    """every pointer, count, alignment and limit is refused by name before any launch (label mode: no launch at all)"""
    L = _lib.lib()
    assert L.ctdet_set_label_mode(2) == 0
    try:
        assert _match() == 0, L.ctdet_last_error()
        assert L.ctdet_last_kernel_label().decode() == "le_match_kernel<wave per cell,40 matchers>"
        assert _match(A=1, T=1) == 0 and L.ctdet_last_kernel_label().decode() == "le_match_kernel<wave per cell,1 matchers>"
        assert _match(A=4, T=16) == 0
        assert _match(A=5, T=13) != 0 and b"A=5 area ranges x T=13" in L.ctdet_last_error()      # one lane per matcher
        assert _match(T=0) != 0 and _match(A=0) != 0
        assert _match(max_det=0) != 0 and b"max_det=0" in L.ctdet_last_error()
        # an empty set of detections, or of ground truths, is a valid input, with no buffer for it
        assert _match(N=0, null="boxes") == 0 and _match(NG=0, null="gt_boxes") == 0
        assert _match(I=0) != 0 and _match(K=0) != 0 and _match(N=-1) != 0 and _match(N=1 << 31) != 0 and _match(NG=-1) != 0
        assert b"ground truths out of range" in L.ctdet_last_error()
        assert _match(I=1 << 13, K=1 << 13) != 0 and b"2^26" in L.ctdet_last_error()
        assert _match(I=(1 << 13) - 1, K=1 << 13) == 0, L.ctdet_last_error()
        assert _match(ws=BASE + 16) != 0 and b"aligned" in L.ctdet_last_error()
        for null in MATCH_POINTERS:
            assert _match(null=null) != 0, null
            assert ("null pointer " + null).encode() in L.ctdet_last_error(), (null, L.ctdet_last_error())
        assert _acc() == 0, L.ctdet_last_error()
        assert L.ctdet_last_kernel_label().decode() == "le_accum_kernel<workgroup per (k,a,t),two passes>"
        assert _acc(N=0, null=("order", "flags")) == 0
        assert _acc(R=0) != 0 and _acc(R=4097) != 0 and b"R=4097" in L.ctdet_last_error()
        assert _acc(K=0) != 0 and _acc(N=-1) != 0 and _acc(T=0) != 0 and _acc(A=8, T=10) != 0
        for null in ACC_POINTERS:
            assert _acc(null=(null,)) != 0, null
            assert ("null pointer " + null).encode() in L.ctdet_last_error(), (null, L.ctdet_last_error())
    finally:
        L.ctdet_set_label_mode(0)
