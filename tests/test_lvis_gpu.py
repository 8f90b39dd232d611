"""LVIS scoring on the GPU: the HIP matcher and accumulate kernels (csrc/lviseval.hip) against the numpy restatement of the rule
(tests/lvis_cases.py), bit for bit, on the hand-derived cases and at the seams of the kernels; the evaluator in shuffled
process() order; a small DLA-34 end to end over a synthetic LVIS json tree through DefaultTrainer.test."""
import json
import os

import numpy as np
import pytest
import torch

import lvis_cases as LC
from detectron2_centernet_amd.evaluation import LVISEvaluator, LVISevalHIP

pytestmark = pytest.mark.gpu


def _dev_gt(gt, frequency=None):
    return {"image_ids": list(range(gt["I"])), "cat_ids": list(range(gt["K"])), "boxes": gt["boxes"], "area": gt["area"],
            "ignore": gt["ignore"], "off": gt["off"], "lists": gt["lists"], "frequency": list(frequency or [""] * gt["K"])}


def _run(dev, gt, boxes, scores, classes, image, params=None):
    ev = LVISevalHIP(_dev_gt(gt), torch.as_tensor(boxes).reshape(-1, 4).to(dev), torch.as_tensor(scores).to(dev),
                     torch.as_tensor(classes).to(dev), torch.as_tensor(image).to(dev))
    for k, v in (params or {}).items():
        setattr(ev, k, v)
    ev.score()
    return ev


def _check(ev, want, what):
    """device arrays against the restatement's: the two tables bit for bit, and what leads to them"""
    assert ev.precision.shape == want["precision"].shape and ev.recall.shape == want["recall"].shape, what
    assert ev.precision.tobytes() == want["precision"].tobytes(), (what, np.abs(ev.precision - want["precision"]).max())
    assert ev.recall.tobytes() == want["recall"].tobytes(), what
    assert np.array_equal(ev.npig.cpu().numpy(), want["npig"]), what
    cls_off = ev.cls_off.cpu().numpy()
    assert np.array_equal(cls_off, want["cls_off"]), what
    n = int(cls_off[-1])
    assert n == int(want["part"].sum())
    order = ev.order.cpu().numpy()
    assert np.array_equal(order[:n], want["order"][:n]), what
    assert sorted(order[n:].tolist()) == sorted(want["order"][n:].tolist()), what      # what takes no part lies behind, in any order
    assert np.array_equal(ev.flags.cpu().numpy()[want["part"]], want["flags"][want["part"]]), what


@pytest.fixture(scope="module")
def restated():
    """every case's restatement, computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            case = LC.hand_case(name) + ({},) if name in LC.HAND_CASES else LC.build_case(name)
            cache[name] = (case, LC.lvis_score(*case[:5], **case[5]))
        return cache[name]
    return get


@pytest.mark.parametrize("name", LC.HAND_CASES)
def test_hand_derived_cases(dev, restated, name):
    case, want = restated(name)
    _check(_run(dev, *case), want, name)


@pytest.mark.parametrize("name", LC.CASES)
def test_seams_against_the_restatement(dev, restated, name):
    case, want = restated(name)
    ev = _run(dev, *case)
    _check(ev, want, name)
    gt, image = case[0], case[4]
    cells = np.diff(gt["off"])
    flags = want["flags"][want["part"]]
    assert (flags & 1).any() and (flags & 2).any(), name                             # true positives and ignored detections
    assert (flags == 0).any() or name == "i1", name                                  # false positives
    if name == "gt_seams":
        assert sorted(set(cells.tolist())) == sorted(set(LC.GT_COUNTS))
        assert not want["part"].all()                                                # detections of a class in neither list
    if name == "gt_130_many_dets":       # more than LE_LDS_GT = 128 ground truths: the taken flags of this cell are in the workspace
        assert cells.max() == 130 and len(image) == 300 and want["part"].all()
        assert ((flags[:, 0] & 1) == 1).sum() > 50 and (flags[:, 0] == 0).sum() > 100     # duplicates were refused on them
    if name == "det_seams":
        assert sorted(np.bincount(image).tolist()) == sorted(LC.DET_COUNTS)
    if name == "image_cut":
        assert np.bincount(image).tolist() == list(LC.IMAGE_COUNTS)
        assert np.bincount(image[~want["part"]], minlength=3).tolist()[2] >= 1       # the 301st is cut
    if name == "cut_small":
        kept = np.bincount(image[want["part"]], minlength=4)
        assert np.bincount(image).tolist() == [6, 7, 8, 20] and np.all(kept <= [6, 7, 7, 7])
    if name == "t1":
        assert ev.precision.shape == (1, 101, 2, 4)
    if name == "a1":
        assert ev.precision.shape == (10, 101, 2, 1)
    if name == "k20":
        assert ev.precision.shape == (10, 101, 20, 4) and (want["npig"][:, 0] > 0).all()
    if name == "i1":
        assert gt["I"] == 1 and want["part"].all()
    if name == "chunks":                 # a class segment of four 256-element chunks, true positives in the last one
        n = int(want["cls_off"][1])
        assert 3 * 256 < n <= 4 * 256 and (want["flags"][want["order"][768:n], 0] == 1).any()


def test_no_detections_and_no_ground_truth(dev, restated):
    case, _ = restated("i1")
    gt = case[0]
    none = (np.zeros((0, 4), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int32), np.zeros(0, np.int32))
    ev = _run(dev, gt, *none)                                                        # N = 0
    _check(ev, LC.lvis_score(gt, *none), "N = 0")
    assert ev.cls_off.cpu().tolist() == [0] * (gt["K"] + 1)
    assert not ev.precision[:, :, :2, 0].any() and not ev.recall[:, :2, 0].any() and np.all(ev.precision[:, :, 2] == -1)
    empty = LC.make_gt(gt["I"], gt["K"], [], neg=[(0, 0), (0, 1)])                   # NG = 0: two negative classes, one dropped
    ev = _run(dev, empty, *case[1:5])
    want = LC.lvis_score(empty, *case[1:5])
    _check(ev, want, "NG = 0")
    assert np.all(ev.precision == -1) and np.all(ev.recall == -1) and want["part"].sum() == 15
    ev = _run(dev, empty, *none)                                                     # both
    assert np.all(ev.precision == -1) and np.all(ev.recall == -1)


@pytest.mark.parametrize("field,value,cause", [("classes", 3, "class index"), ("classes", -1, "class index"),
                                               ("image", 1, "image index"), ("image", -1, "image index"),
                                               ("scores", float("nan"), "score that is not finite"),
                                               ("scores", float("inf"), "score that is not finite"),
                                               ("boxes", float("inf"), "box coordinate")])
def test_status_word_becomes_a_named_error(dev, restated, field, value, cause):
    (gt, boxes, scores, classes, image, _), _ = restated("i1")
    arrays = {"boxes": boxes.copy(), "scores": scores.copy(), "classes": classes.copy(), "image": image.copy()}
    arrays[field][3] = value
    with pytest.raises(ValueError, match=cause) as e:
        _run(dev, gt, arrays["boxes"], arrays["scores"], arrays["classes"], arrays["image"])
    assert str(e.value).count(";") == 0        # one cause, named alone


def test_two_runs_give_the_same_bits(dev, restated):
    case, _ = restated("k20")
    a, b = _run(dev, *case), _run(dev, *case)
    assert a.precision.tobytes() == b.precision.tobytes() and a.recall.tobytes() == b.recall.tobytes()
    for k in ("order", "cls_off", "npig"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    n = int(a.cls_off[-1])
    part = a.order[:n].long()
    assert torch.equal(a.flags[part], b.flags[part])


# ---- the evaluator
CATS = 5
FREQ = "rcffc"


def _lvis_json(case, size=128):
    """a restatement case as an LVIS json dict: image ids 10, 20, ... and category ids 1 .. K"""
    gt = case[0]
    images = []
    for i in range(gt["I"]):
        images.append({"id": 10 * (i + 1), "height": size, "width": size, "file_name": f"val2017/{i:06d}.png",
                       "neg_category_ids": [k + 1 for k in range(gt["K"]) if gt["lists"][i, k] & LC.NEG],
                       "not_exhaustive_category_ids": [k + 1 for k in range(gt["K"]) if gt["lists"][i, k] & LC.NEL]})
    cats = [{"id": k + 1, "name": f"thing_{k}", "synonyms": [f"thing_{k}"], "frequency": FREQ[k % len(FREQ)]} for k in range(gt["K"])]
    anns = [{"id": n + 1, "image_id": 10 * (int(gt["image"][n]) + 1), "category_id": int(gt["classes"][n]) + 1,
             "bbox": gt["boxes"][n].tolist(), "area": float(gt["area"][n]), "ignore": int(gt["ignore"][n])}
            for n in range(len(gt["area"]))]
    return {"images": images, "categories": cats, "annotations": anns}


def _e2e_case():
    gts = {(i, k): (i + 2 * k) % 3 for i in range(4) for k in range(CATS)}
    dets = {(i, k): (2 * i + k) % 5 + 1 for i in range(4) for k in range(CATS)}
    return LC.cells_case(31, 4, CATS, gts, dets)


def test_evaluator_in_shuffled_process_order(tmp_path, dev):
    """the order of process() decides input indices, and with them ties: the figures are compared with the restatement run on
    the detections in the order the evaluator saw them"""
    from detectron2_centernet_amd.data import DatasetCatalog, MetadataCatalog, register_lvis_instances
    from detectron2_centernet_amd.structures import Boxes, Instances
    case = _e2e_case()
    gt, boxes, scores, classes, image = case
    path = str(tmp_path / "lvis.json")
    with open(path, "w") as f:
        json.dump(_lvis_json(case), f)
    name = f"lvis_gpu_shuffled_{os.getpid()}"
    register_lvis_instances(name, {}, path, str(tmp_path))
    try:
        ev = LVISEvaluator(name, None, False, str(tmp_path / "out"))
        order = np.random.default_rng(2).permutation(gt["I"])
        seen = []
        for i in order:
            sel = np.flatnonzero(image == i)
            seen.append(sel)
            inst = Instances((128, 128))
            inst.pred_boxes = Boxes(torch.as_tensor(boxes[sel]).reshape(-1, 4).to(dev))
            inst.scores = torch.as_tensor(scores[sel]).to(dev)
            inst.pred_classes = torch.as_tensor(classes[sel]).long().to(dev)
            ev.process([{"image_id": 10 * (int(i) + 1)}], [{"instances": inst}])
        res = ev.evaluate()
    finally:
        DatasetCatalog.remove(name)
        MetadataCatalog.remove(name)
    seen = np.concatenate(seen)
    want = LC.lvis_score(gt, boxes[seen], scores[seen], classes[seen], image[seen])
    assert ev.lvis_eval.precision.tobytes() == want["precision"].tobytes()
    s = LC.summarize(want["precision"], want["recall"], [FREQ[k] for k in range(CATS)])
    assert list(res) == ["bbox"] and list(res["bbox"]) == ["AP", "AP50", "AP75", "APs", "APm", "APl", "APr", "APc", "APf"]
    for m, v in res["bbox"].items():
        assert (np.isnan(v) and s[m] == -1) or v == s[m] * 100, (m, v, s[m])
    assert 0 < res["bbox"]["AP"] < 100 and res["bbox"]["APr"] != res["bbox"]["APf"]
    assert ev.lvis_eval.ar == {k: v for k, v in s.items() if k.startswith("AR")}
    results = json.load(open(str(tmp_path / "out" / "lvis_instances_results.json")))
    assert len(results) == len(scores) and results[0]["image_id"] == 10 * (int(order[0]) + 1)
    assert [r["category_id"] for r in results] == (classes[seen] + 1).tolist()


def test_dla34_end_to_end_over_an_lvis_json(tmp_path, dev):
    from PIL import Image

    from detectron2_centernet_amd.data import DatasetCatalog, MetadataCatalog, register_all_lvis
    from detectron2_centernet_amd.engine import DefaultTrainer
    from test_trainer_gpu import _cfg
    root = tmp_path / "datasets"
    case = _e2e_case()
    data = _lvis_json(case)
    rng = np.random.default_rng(12)
    os.makedirs(str(root / "coco" / "val2017"))
    os.makedirs(str(root / "lvis"))
    for im in data["images"]:
        Image.fromarray(rng.integers(0, 256, (128, 128, 3), dtype=np.uint8)).save(str(root / "coco" / im["file_name"]))
    for split in ("train", "val"):
        with open(str(root / "lvis" / f"lvis_v1_{split}.json"), "w") as f:
            json.dump(data, f)
    added = register_all_lvis(str(root))
    try:
        assert added == ["lvis_v1_train", "lvis_v1_val"]
        cfg = _cfg(tmp_path, tmp_path / "out", "DATASETS.TRAIN", "('lvis_v1_train',)", "DATASETS.TEST", "('lvis_v1_val',)")
        torch.manual_seed(5)
        model = DefaultTrainer.build_model(cfg)
        assert model.num_classes == CATS and MetadataCatalog.get("lvis_v1_train").class_frequency == FREQ
        model.wh[-1].bias.data.fill_(6.0)          # boxes of non-degenerate size: a random-init wh head gives empty boxes
        evaluator = DefaultTrainer.build_evaluator(cfg, "lvis_v1_val")
        assert type(evaluator) is LVISEvaluator
        res = DefaultTrainer.test(cfg, model, evaluators=[evaluator])
        assert list(res) == ["bbox"] and len(res["bbox"]) == 9
        assert all(np.isnan(v) or 0.0 <= v <= 100.0 for v in res["bbox"].values()) and np.isfinite(res["bbox"]["AP"]), res
        # what was scored: the model's detections of the four images, and the figures the restatement gives for them
        boxes, scores, classes, image = (t.cpu().numpy() for t in evaluator.lvis_eval._dt)
        assert 0 < len(scores) <= 4 * 100 and set(image.tolist()) == {0, 1, 2, 3}
        want = LC.lvis_score(case[0], boxes, scores, classes, image)
        assert evaluator.lvis_eval.precision.tobytes() == want["precision"].tobytes()
        s = LC.summarize(want["precision"], want["recall"], list(FREQ))
        assert res["bbox"]["AP"] == s["AP"] * 100
        # the trainer picks the evaluator by the dataset's evaluator_type, writes the results file and reproduces the figures
        np.testing.assert_equal(DefaultTrainer.test(cfg, model), res)
        assert os.path.isfile(os.path.join(cfg.OUTPUT_DIR, "inference", "lvis_instances_results.json"))
        model.train()
    finally:
        for n in added:
            DatasetCatalog.remove(n)
            MetadataCatalog.remove(n)
