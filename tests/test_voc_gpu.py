"""Pascal VOC scoring on the GPU: the HIP matcher and AP kernels (csrc/voceval.hip) against the reference's recorded results
(tests/golden/g23_voceval.npz) and, at the seams of the kernels, against the numpy restatement of the rule
(tests/voc_cases.py); the evaluator in shuffled process() order; a small DLA-34 end to end over a synthetic VOC tree.

What is exact: the order, the flags, npos, rec, prec and the 11-point AP, bit for bit.  The area AP sums the same bit-equal
terms (total <= 1) as numpy's pairwise `np.sum` in another order: within (terms + 2) * 2^-52."""
import os

import numpy as np
import pytest
import torch

import voc_cases as VC
from detectron2_centernet_amd.evaluation import PascalVOCDetectionEvaluator, VOCevalHIP, derive_voc_results, inference_on_dataset
from test_voc_host import G23, g23_inputs, write_voc_tree

pytestmark = pytest.mark.gpu


def _dev_gt(gt):
    return {"image_ids": list(range(gt["I"])), "class_names": list(range(gt["K"])), "boxes": gt["boxes"],
            "difficult": gt["difficult"], "off": gt["off"]}


def _run(dev, gt, boxes, scores, classes, image, thresholds):
    ev = VOCevalHIP(_dev_gt(gt), torch.as_tensor(boxes).reshape(-1, 4).to(dev), torch.as_tensor(scores).to(dev),
                    torch.as_tensor(classes).to(dev), torch.as_tensor(image).to(dev))
    ev.evaluate(thresholds, 2007, keep_pr=True)
    return ev


def _arrays(ev):
    return {k: getattr(ev, k).cpu().numpy() for k in ("order", "cls_off", "npos", "flags", "rec", "prec")} | {
        "ap07": ev.ap07, "ap12": ev.ap12}


def _check(got, want, what):
    """device arrays against the restatement's (or the reference's recorded ones)"""
    for k in ("order", "cls_off", "npos", "flags"):
        if k in want:
            assert np.array_equal(got[k], want[k]), (what, k)
    assert np.array_equal(got["rec"], want["rec"], equal_nan=True), what
    assert np.array_equal(got["prec"], want["prec"]), what
    assert np.array_equal(got["ap07"], want["ap07"]), what
    nan = np.isnan(want["ap12"])
    assert np.array_equal(np.isnan(got["ap12"]), nan), what
    err = np.abs(got["ap12"] - want["ap12"])[~nan]
    bound = VC.area_bound(want["terms"])[~nan]
    print(f"{what}: area AP max |device - want| = {err.max() if err.size else 0.0:.3e} (bound {bound.min() if bound.size else 0.0:.3e})")
    assert np.all(err <= bound), (what, err.max())


@pytest.fixture(scope="module")
def g23():
    g = np.load(G23)
    return g, VC.voc_score(*g23_inputs(g))


def test_g23_through_the_abi_is_exact_and_repeatable(dev, g23):
    g, r = g23
    inputs = g23_inputs(g) + (VC.THRESHOLDS,)
    a = _arrays(_run(dev, *inputs))
    ref = {k: g[k] for k in ("cls_off", "rec", "prec", "ap07", "ap12")} | {"terms": r["terms"]}
    ref["cls_off"] = ref["cls_off"].astype(np.int32)
    _check(a, ref, "g23 vs reference")
    _check(a, r, "g23 vs restatement")
    b = _arrays(_run(dev, *inputs))
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def _register_g23_tree(g, root, name, year):
    from detectron2_centernet_amd.data import register_pascal_voc
    names = [str(n) for n in g["class_names"]]
    images = {str(i): (500, 375, []) for i in g["image_ids"]}
    for i, k, d, b in zip(g["gt_image"], g["gt_classes"], g["gt_difficult"], g["gt_boxes"]):
        images[str(g["image_ids"][i])][2].append((names[k], int(d)) + tuple(int(v) for v in b))
    write_voc_tree(root, images)
    register_pascal_voc(name, root, "test", year, class_names=names)


def test_g23_through_the_evaluator_in_shuffled_order(tmp_path, dev, g23):
    """distinct quantised scores within every class: the order of process() cannot matter"""
    from detectron2_centernet_amd.data import DatasetCatalog, MetadataCatalog
    from detectron2_centernet_amd.structures import Boxes, Instances
    g, r = g23
    names = [str(n) for n in g["class_names"]]
    order = np.random.default_rng(1).permutation(len(g["image_ids"]))
    for year, tag in ((2007, "res07"), (2012, "res12")):
        name = f"voc_gpu_g23_{year}_{os.getpid()}"
        _register_g23_tree(g, str(tmp_path / str(year)), name, year)
        try:
            ev = PascalVOCDetectionEvaluator(name, distributed=False)
            ev.reset()
            for i in order:
                sel = np.flatnonzero(g["image"] == i)
                inst = Instances((375, 500))
                inst.pred_boxes = Boxes(torch.as_tensor(g["boxes"][sel]).reshape(-1, 4).to(dev))
                inst.scores = torch.as_tensor(g["scores"][sel]).to(dev)
                inst.pred_classes = torch.as_tensor(g["classes"][sel]).long().to(dev)
                ev.process([{"image_id": str(g["image_ids"][i])}], [{"instances": inst}])
            res = ev.evaluate()
        finally:
            DatasetCatalog.remove(name)
            MetadataCatalog.remove(name)
        assert list(res) == ["bbox", "bbox_AP", "bbox_AP50", "bbox_AP75"]
        # 100 x the bound of the area AP, over sums of at most ten tables; nothing is allowed for the 11-point form
        tol = 0.0 if year == 2007 else 100 * 4 * float(VC.area_bound(r["terms"]).max())
        got = np.array([res["bbox"][m] for m in ("AP", "AP50", "AP75")])
        assert np.allclose(got, g[tag + "_bbox"], rtol=0, atol=tol, equal_nan=True), (year, got, g[tag + "_bbox"])
        for key in ("bbox_AP", "bbox_AP50", "bbox_AP75"):
            got = np.array([res[key][n] for n in names])
            assert np.allclose(got, g[tag + "_" + key], rtol=0, atol=tol, equal_nan=True), (year, key)
        assert np.array_equal(ev.voc_eval.ap07, g["ap07"])


@pytest.fixture(scope="module")
def restated():
    """every case's restatement, computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            case = VC.build_case(name)
            cache[name] = (case, VC.voc_score(*case))
        return cache[name]
    return get


@pytest.mark.parametrize("name", VC.CASES)
def test_seams_against_the_restatement(dev, restated, name):
    case, want = restated(name)
    ev = _run(dev, *case)
    _check(_arrays(ev), want, name)
    gt = case[0]
    cells = np.diff(gt["off"])
    if name == "gt_seams":
        assert sorted(set(cells.tolist())) == sorted(set(VC.GT_COUNTS)) and want["flags"].any()
    if name == "gt_130_many_dets":       # the taken words of this cell are in the workspace; duplicates were refused on them
        assert cells.max() == 130 and (want["flags"] == 2).sum() > 100 and (want["flags"] == 1).sum() > 50
    if name == "det_seams":
        assert sorted(np.bincount(case[4]).tolist()) == sorted(VC.DET_COUNTS)
    if name == "first_wins":             # ground truth 0 and its twin 64: the first wins, twice
        assert want["flags"][:, 0].tolist() == [1, 2, 1]
    if name == "chunks":
        assert len(case[2]) > 3 * 256 and (want["flags"][want["order"][-256:], 0] == 1).any()
    if name == "perfect":
        assert np.all(np.abs(ev.ap07 * 100 - 100) < 1e-12) and np.all(np.abs(ev.ap12 * 100 - 100) < 1e-11)
        assert np.all(want["flags"] == 1)


def test_no_detections(dev, restated):
    case, _ = restated("i1")
    gt = case[0]
    ev = _run(dev, gt, np.zeros((0, 4), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int32), np.zeros(0, np.int32),
              VC.THRESHOLDS)
    assert ev.ap07.shape == (gt["K"], 10) and not ev.ap07.any() and not ev.ap12.any()
    want = VC.voc_score(gt, np.zeros((0, 4), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int32), np.zeros(0, np.int32))
    assert ev.npos.cpu().tolist() == want["npos"].tolist() and ev.cls_off.cpu().tolist() == [0] * (gt["K"] + 1)


@pytest.mark.parametrize("field,value,cause", [("classes", 3, "class index"), ("classes", -1, "class index"),
                                               ("image", 1, "image index"), ("scores", float("nan"), "score that is not finite"),
                                               ("boxes", float("inf"), "box coordinate")])
def test_status_word_becomes_a_named_error(dev, restated, field, value, cause):
    (gt, boxes, scores, classes, image, thr), _ = restated("i1")
    arrays = {"boxes": boxes.copy(), "scores": scores.copy(), "classes": classes.copy(), "image": image.copy()}
    arrays[field][3] = value
    with pytest.raises(ValueError, match=cause) as e:
        _run(dev, gt, arrays["boxes"], arrays["scores"], arrays["classes"], arrays["image"], thr)
    assert str(e.value).count(";") == 0        # one cause, named alone


# ---- end to end
def _voc_e2e_tree(root, n=4, size=128):
    """a VOC2007 tree of `n` Pillow-written JPEGs with a few objects each; trainval and test list the same images"""
    from PIL import Image

    from detectron2_centernet_amd.data import CLASS_NAMES
    rng = np.random.default_rng(11)
    images = {}
    for i in range(n):
        objs = []
        for _ in range(int(rng.integers(1, 4))):
            x, y = int(rng.integers(1, size - 50)), int(rng.integers(1, size - 50))
            objs.append((CLASS_NAMES[int(rng.integers(0, 20))], int(rng.random() < 0.3), x, y, x + int(rng.integers(16, 48)),
                         y + int(rng.integers(16, 48))))
        images["%06d" % (i + 1)] = (size, size, objs)
    for split in ("trainval", "test"):
        write_voc_tree(root, images, split)
    for fileid in images:
        Image.fromarray(rng.integers(0, 256, (size, size, 3), dtype=np.uint8)).save(os.path.join(root, "JPEGImages", fileid + ".jpg"))
    return images


def test_dla34_end_to_end_over_a_voc_tree(tmp_path, dev):
    from detectron2_centernet_amd.data import (DatasetCatalog, MetadataCatalog, build_detection_test_loader,
                                               register_all_pascal_voc)
    from detectron2_centernet_amd.engine import DefaultTrainer
    from test_trainer_gpu import _cfg
    _voc_e2e_tree(str(tmp_path / "datasets" / "VOC2007"))
    added = register_all_pascal_voc(str(tmp_path / "datasets"))
    try:
        assert "voc_2007_test" in added and "voc_2012_val" not in added
        cfg = _cfg(tmp_path, tmp_path / "out", "DATASETS.TRAIN", "('voc_2007_trainval',)", "DATASETS.TEST", "('voc_2007_test',)")
        torch.manual_seed(5)
        model = DefaultTrainer.build_model(cfg)
        assert model.num_classes == 20
        model.wh[-1].bias.data.fill_(6.0)          # boxes of non-degenerate size: a random-init wh head gives empty boxes
        ev = PascalVOCDetectionEvaluator("voc_2007_test", distributed=False)
        res = inference_on_dataset(model, build_detection_test_loader(cfg, "voc_2007_test"), ev)
        assert list(res) == ["bbox", "bbox_AP", "bbox_AP50", "bbox_AP75"] and len(res["bbox_AP"]) == 20
        assert all(np.isfinite(v) and 0.0 <= v <= 100.0 for v in res["bbox"].values()), res["bbox"]
        # what was scored: the model's detections of the four images, and the figures the restatement gives for them
        boxes, scores, classes, image = (t.cpu().numpy() for t in ev.voc_eval._dt)
        assert 0 < len(scores) <= 4 * 100 and set(image.tolist()) == {0, 1, 2, 3}
        g = ev._gt
        want = VC.voc_score({"I": 4, "K": 20, "boxes": g["boxes"], "difficult": g["difficult"], "off": g["off"]}, boxes, scores,
                            classes, image)
        assert np.array_equal(ev.voc_eval.ap07, want["ap07"])
        assert res["bbox_AP50"] == derive_voc_results(want["ap07"], MetadataCatalog.get("voc_2007_test").thing_classes)["bbox_AP50"]
        # the trainer picks the evaluator by the dataset's evaluator_type and reproduces the figures
        again = DefaultTrainer.test(cfg, model)
        assert again == res
        model.train()
    finally:
        for n in added:
            DatasetCatalog.remove(n)
            MetadataCatalog.remove(n)
