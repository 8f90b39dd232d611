"""Multi-scale test augmentation's soft-NMS merge, the parts that need no GPU: the float64 restatement
against hand-derived answers, the margin condition of every committed case, the config surface, the wrapper's switch, the new
entry point of the shared library (argument checks through the label dry run, where nothing is launched and host addresses
stand in for device pointers) and its launch label."""
import ctypes as C
import glob
import os
import shutil

import numpy as np
import pytest
import torch

import soft_nms_cases as S
from detectron2_centernet_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
_BUF = C.create_string_buffer(64)
BASE = (C.addressof(_BUF) + 15) & ~15       # a 16-byte aligned address to stand in for every device pointer


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name,cands,want", S.KNOWN, ids=[k[0] for k in S.KNOWN])
def test_restatement_known_answers(name, cands, want):
    boxes = np.asarray([c[0] for c in cands], dtype=np.float32)
    scores = np.asarray([c[1] for c in cands], dtype=np.float32)
    order, out, _ = S.class_soft_nms(boxes, scores, 0.5, 0.001)
    assert order.tolist() == [w[0] for w in want]
    for k, (i, s) in enumerate(want):
        # the hand-derived weight times the f32 input score, in float64
        w = s / cands[i][1]
        assert out[k] == pytest.approx(float(scores[i]) * w, rel=1e-13), (name, k)
    # through the batch interface: one pass, one image, max_det cuts the ordered list
    passes = [(boxes[None], scores[None], np.zeros((1, len(cands)), dtype=np.int32), np.asarray([len(cands)], dtype=np.int32))]
    r = S.merge_reference(passes, 1, max_det=2)[0]
    by_score = sorted(range(len(want)), key=lambda k: (-out[k], k))[:2]
    assert r["count"] == len(by_score) and r["survivors"] == len(want)
    assert np.array_equal(r["boxes"], boxes[[want[k][0] for k in by_score]])


def test_restatement_overlap_values():
    """the numbers of the known answers, spelled out"""
    assert 0.8 * np.exp(-2.0) == pytest.approx(0.10826822658929017)
    assert np.exp(-2.0 / 9.0) == pytest.approx(0.8007374029168081)
    assert 0.006 * np.exp(-2.0) < 0.001 < 0.5 * np.exp(-4.0)
    assert 0.85 * np.exp(-2.0) < 0.3


def test_restatement_ties_and_classes():
    case = next(c for c in S.CASES if c.name == "ties")
    r = case.reference()[0]
    assert r["count"] == 11
    # 0.75 first; the 0.625 pair (class 0, in candidate order); 0.5: class 0, then class 1, then class 2's two in candidate order
    assert r["classes"].tolist()[:7] == [2, 0, 0, 0, 1, 2, 2]
    assert r["boxes"][1:3, 0].tolist() == [0.0, 300.0] and r["boxes"][5:7, 0].tolist() == [0.0, 100.0]
    assert r["decays"].tolist()[:7] == [0] * 7 and sorted(r["decays"].tolist()) == [0] * 9 + [1, 1]


def test_f32_evaluation_of_the_restatement_is_within_the_bound():
    """the bound's own sanity on the CPU: numpy f32, operation by operation, against float64 on every case"""
    for case in S.CASES:
        r32 = S.merge_reference(case.passes, case.num_classes, case.sigma, case.min_score, case.max_det, dtype=np.float32)
        for a, b in zip(case.reference(), r32):
            assert a["count"] == b["count"], case
            if a["count"] <= 0:
                continue
            assert np.array_equal(a["boxes"], b["boxes"]) and np.array_equal(a["classes"], b["classes"]), case
            rel = np.abs(b["scores"].astype(np.float64) - a["scores"]) / np.abs(a["scores"])
            assert (rel <= S.bound(a["decays"], case.sigma)).all(), case


@pytest.mark.parametrize("case", S.CASES, ids=repr)
def test_every_case_meets_the_margin_condition(case):
    assert S.check_margins(case) == []


def test_the_cases_cover_the_edges():
    names = {c.name: c for c in S.CASES}
    for n in (0, 1, 63, 64, 65, 128, 129):
        p = names[f"cell{n}"].passes
        assert sum(int(((q[2][0, :q[3][0]]) == 1).sum()) for q in p) == n
    assert [r["count"] for r in names["empty_image_B3_widths"].reference()][1] == 0
    assert [q[1].shape[1] for q in names["empty_image_B3_widths"].passes] == [100, 37, 64, 1]
    assert all(int(q[3].sum()) == 0 for q in names["all_passes_empty"].passes)
    full = names["full2048"]
    assert sum(int((q[2][0, :q[3][0]] == 1).sum()) for q in full.passes) == 2048 and len(full.passes) == 16
    assert 2000 < full.reference()[0]["count"] < 2048 and full.reference()[0]["decays"].max() >= 3
    assert names["one_class"].num_classes == 1 and names["one_class"].reference()[0]["survivors"] > 100
    c80 = names["classes80"].reference()[0]["classes"]
    assert 79 in c80 and len(set(c80.tolist())) < 80
    ns = names["survivors_equal_max_det"].reference()[0]["survivors"]
    assert names["survivors_equal_max_det"].max_det == ns
    assert names["survivors_fewer_max_det"].max_det > ns > names["survivors_more_max_det"].max_det
    assert names["survivors_more_max_det"].reference()[0]["count"] == names["survivors_more_max_det"].max_det
    assert names["near4000"].reference()[0]["boxes"].max() > 3900
    b = names["subpixel"].reference()[0]["boxes"]
    assert ((b[:, 2] - b[:, 0]) < 1).all()
    assert [r["count"] for r in names["nonfinite_flag"].reference()][1] == -1
    # decays remove candidates and re-order them in the random cases: the loop is exercised, not only the copy
    r = names["clustered91"].reference()[0]
    assert r["decays"].max() >= 3 and r["survivors"] < 150


# ------------------------------------------------------------------------------------------------ config and wrapper
def test_soft_nms_config_keys():
    from detectron2_centernet_amd.config import get_cfg
    cfg = get_cfg()
    node = cfg.TEST.SOFT_NMS
    assert node.ENABLED is False and node.SIGMA == 0.5 and node.MIN_SCORE == 0.001
    assert sorted(node.keys()) == ["ENABLED", "MIN_SCORE", "SIGMA"]
    assert sorted(cfg.TEST.AUG.keys()) == ["ENABLED", "FLIP", "MAX_SIZE", "MIN_SIZES"]
    cfg.merge_from_list(["TEST.SOFT_NMS.ENABLED", True, "TEST.SOFT_NMS.SIGMA", 0.25])
    assert cfg.TEST.SOFT_NMS.ENABLED is True and cfg.TEST.SOFT_NMS.SIGMA == 0.25


def test_golden_yamls_still_load(tmp_path):
    from detectron2_centernet_amd.config import get_cfg
    names = sorted(glob.glob(os.path.join(GOLDEN, "g16_configs", "*.yaml")) + glob.glob(os.path.join(GOLDEN, "g17_configs", "*.yaml")))
    assert len(names) >= 6
    for n in names:
        shutil.copy(n, tmp_path / os.path.basename(n))
    for n in names:
        cfg = get_cfg()
        cfg.merge_from_file(str(tmp_path / os.path.basename(n)))
        assert cfg.TEST.SOFT_NMS.ENABLED is False and cfg.TEST.SOFT_NMS.SIGMA == 0.5, n


def _cfg(tmp_path, min_sizes=(), soft_nms=False):
    from detectron2_centernet_amd.config import get_cfg
    for n in ("Base-CenterNet.yaml", "ctdet_dla_34_1x.yaml"):
        shutil.copy(os.path.join(GOLDEN, "g16_configs", n), tmp_path / n)
    cfg = get_cfg()
    cfg.merge_from_file(str(tmp_path / "ctdet_dla_34_1x.yaml"))
    cfg.MODEL.DEVICE = "cpu"
    cfg.TEST.AUG.ENABLED, cfg.TEST.AUG.MIN_SIZES, cfg.TEST.SOFT_NMS.ENABLED = True, tuple(min_sizes), soft_nms
    return cfg


def test_wrapper_takes_several_sizes_only_with_the_switch(tmp_path):
    from detectron2_centernet_amd.data.catalog import register_synthetic
    from detectron2_centernet_amd.modeling import CenterNetWithTTA, build_model
    cfg = _cfg(tmp_path)
    register_synthetic(cfg.DATASETS.TRAIN[0], num_classes=80)
    model = build_model(cfg)
    nine = (400, 500, 600, 700, 800, 900, 1000, 1100, 1200)
    with pytest.raises(NotImplementedError, match="multi-scale merging") as e:
        CenterNetWithTTA(_cfg(tmp_path, min_sizes=nine), model)
    assert "TEST.SOFT_NMS.ENABLED" in str(e.value)       # the refusal names the switch
    with pytest.raises(AssertionError, match="CenterNet"):
        CenterNetWithTTA(_cfg(tmp_path, min_sizes=nine, soft_nms=True), torch.nn.Conv2d(3, 3, 1))
    tta = CenterNetWithTTA(_cfg(tmp_path, min_sizes=nine, soft_nms=True), model)
    assert tta.soft_nms and len(tta.passes) == 9 and tta.resize is None and tta.flip is True
    assert [one.resize.short_edge_length[0] for one in tta.passes] == list(nine)
    assert all(type(one) is CenterNetWithTTA and not one.soft_nms and one.flip is True for one in tta.passes)
    assert (tta.sigma, tta.min_score, tta.max_det) == (0.5, 0.001, 100)
    assert tuple(tta.cfg.TEST.AUG.MIN_SIZES) == nine
    one = CenterNetWithTTA(_cfg(tmp_path, min_sizes=(64,), soft_nms=True), model)
    assert one.soft_nms and len(one.passes) == 1 and one.resize is one.passes[0].resize is not None
    none = CenterNetWithTTA(_cfg(tmp_path, soft_nms=True), model)
    assert len(none.passes) == 1 and none.passes[0].resize is None and none.resize is None
    off = CenterNetWithTTA(_cfg(tmp_path, min_sizes=(64,)), model)
    assert off.soft_nms is False and off.passes == [] and off.resize is not None
    # every size states its own target, in the original frame
    tta = CenterNetWithTTA(_cfg(tmp_path, min_sizes=(64, 96), soft_nms=True), model)
    img = torch.zeros(3, 32, 48, dtype=torch.uint8)
    raw = np.zeros((32, 48, 3), dtype=np.uint8)
    for one, hw in zip(tta.passes, ((64, 96), (96, 144))):
        out = one._inputs([{"image": img}])
        assert tuple(out[0]["image"].shape) == (3,) + hw and (out[0]["height"], out[0]["width"]) == (32, 48)
        out = one._inputs([{"image_raw": raw}])
        assert out[0]["resize_hw"] == hw and (out[0]["height"], out[0]["width"]) == (32, 48)
    # training mode is refused when called
    with pytest.raises(RuntimeError, match="inference-time"):
        tta([{"image": img}])
    # on the CPU the merge is refused like every op
    model.eval()
    with pytest.raises(NotImplementedError):
        tta([{"image": img}])


def test_op_has_no_cpu_implementation():
    from detectron2_centernet_amd import ops
    p = (torch.zeros(1, 2, 4), torch.zeros(1, 2), torch.zeros(1, 2, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(NotImplementedError):
        ops.soft_nms_merge([p], 3, 0.5, 0.001, 10)


# ------------------------------------------------------------------------------------------------ the entry point
def test_new_symbol_and_abi_version():
    L = _lib.lib()
    assert L.ctdet_abi_version() == 8
    raw = C.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "ctdet_soft_nms_merge")
    assert "ctdet_soft_nms_merge" in _lib.SIGNATURES
    header = open(os.path.join(os.path.dirname(HERE), "include", "ctdet_hip.h")).read()
    assert "ctdet_soft_nms_merge(" in header and "typedef struct ctdet_softnms_pass" in header
    assert "#define CTDET_SOFTNMS_MAX_PASSES 16\n" in header
    assert "#define CTDET_SOFTNMS_MAX_CANDIDATES 2048\n" in header
    assert C.sizeof(_lib.SoftNmsPass) == 40


def _call(widths, B=2, classes=80, sigma=0.5, min_score=0.001, max_det=100, table=True):
    t = (_lib.SoftNmsPass * max(len(widths), 1))()
    for i, K in enumerate(widths):
        t[i].boxes = t[i].scores = t[i].classes = t[i].counts = BASE
        t[i].K = K
    p = C.c_void_p(BASE)
    return _lib.lib().ctdet_soft_nms_merge(t if table else None, len(widths), B, classes, sigma, min_score, max_det, p, p, p, p, p,
                                           None)


def test_entry_point_in_a_dry_run():
    L = _lib.lib()
    assert L.ctdet_set_label_mode(2) == 0
    try:
        assert _call([100] * 5) == 0, L.ctdet_last_error()
        assert L.ctdet_last_kernel_label().decode() == \
            "sn_cell_kernel<wave per (image,class)> + sn_rank_kernel<workgroup per image>: 5 passes, 500 candidates"
        assert _call([128] * 16) == 0, L.ctdet_last_error()                # the limits themselves are accepted
        assert L.ctdet_last_kernel_label().decode().endswith("16 passes, 2048 candidates")
        assert _call([100, 0, 7]) == 0 and _call([3], B=0) == 0
        for bad, word in (
                (dict(widths=[10] * 17), b"17 passes"),
                (dict(widths=[]), b"0 passes"),
                (dict(widths=[128] * 15 + [129]), b"2049 candidates"),
                (dict(widths=[2049]), b"2049 candidates"),
                (dict(widths=[10, -1]), b"width -1"),
                (dict(widths=[10], max_det=0), b"max_det=0"),
                (dict(widths=[10], max_det=-3), b"max_det=-3"),
                (dict(widths=[10], sigma=0.0), b"sigma=0"),
                (dict(widths=[10], sigma=-0.5), b"sigma=-0.5"),
                (dict(widths=[10], sigma=float("nan")), b"sigma="),
                (dict(widths=[10], classes=0), b"classes"),
                (dict(widths=[10], B=-1), b"B=-1"),
                (dict(widths=[10], table=False), b"null pass table")):
            assert _call(**bad) == -22, bad
            err = L.ctdet_last_error()
            assert err.startswith(b"soft_nms_merge:") and word in err, (bad, err)
    finally:
        L.ctdet_set_label_mode(0)
