"""Host side of CenterNet's fix_res / keep_res test input (INPUT.AFFINE.TEST_MODE): the config key and its
refusals, data.warp.test_params at its known answers, the keep_res warp as an exact copy, the box round trip, the two kinds of
test record, the numpy oracle of the unwarp kernel against a float64 evaluation and a hand-derived case, and the new entry point
of the C ABI.  No GPU: the kernel is compared in test_unwarp_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

import unwarp_cases as UC
from detectron2_centernet_amd import _lib, ops
from detectron2_centernet_amd.config import get_cfg
from detectron2_centernet_amd.data import TrafficLightDatasetMapper
from detectron2_centernet_amd.data import warp as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(mode="fix_res", out=(64, 64), raw=False):
    cfg = get_cfg()
    cfg.INPUT.AFFINE.TEST_MODE, cfg.INPUT.AFFINE.OUTPUT_SIZE, cfg.INPUT.DEVICE_RESIZE = mode, out, raw
    return cfg


# ------------------------------------------------------------------------------------------------- config and parameters
def test_config_default_and_refusals():
    a = get_cfg().INPUT.AFFINE
    assert a.TEST_MODE == "" and a.ENABLED is False
    assert W.TEST_MODES == ("", "fix_res", "keep_res")
    with pytest.raises(ValueError, match=r"INPUT\.AFFINE\.TEST_MODE 'letterbox'"):
        TrafficLightDatasetMapper(_cfg("letterbox"), is_train=False)
    with pytest.raises(ValueError, match=r"INPUT\.AFFINE\.TEST_MODE 'letterbox'"):
        W.test_params(10, 10, "letterbox", (64, 64), 32)
    cfg = _cfg("keep_res")
    cfg.MODEL.CENTERNET.SIZE_DIVISIBILITY = 24
    with pytest.raises(ValueError, match=r"SIZE_DIVISIBILITY.*power of two, got 24"):
        TrafficLightDatasetMapper(cfg, is_train=False)
    with pytest.raises(ValueError, match="power of two"):
        W.test_params(10, 10, "keep_res", None, 0)
    with pytest.raises(ValueError, match=r"INPUT\.AFFINE\.OUTPUT_SIZE \(64, 72\)"):
        TrafficLightDatasetMapper(_cfg("fix_res", (64, 72)), is_train=False)
    # the key is independent of ENABLED and the training mapper ignores it, bad values included
    for mode in ("fix_res", "keep_res", "letterbox"):
        m = TrafficLightDatasetMapper(_cfg(mode), is_train=True)
        assert m.test_mode == "" and type(m.augmentation[0]).__name__ == "ResizeShortestEdge"
    cfg = _cfg("fix_res")
    cfg.INPUT.AFFINE.ENABLED = True
    assert TrafficLightDatasetMapper(cfg, is_train=False).test_mode == "fix_res"
    assert TrafficLightDatasetMapper(_cfg(""), is_train=False).test_mode == ""


def test_test_params_known_answers():
    # the two answers worked in DESIGN.md 7.13: a 640 x 480 (w x h) source
    M, oh, ow = W.test_params(480, 640, "fix_res", (512, 512), 32)
    assert M.dtype == np.float64 and M.tolist() == [[1.25, 0.0, 0.0], [0.0, 1.25, -80.0]] and (oh, ow) == (512, 512)
    M, oh, ow = W.test_params(480, 640, "keep_res", (512, 512), 32)
    assert M.tolist() == [[1.0, 0.0, -16.0], [0.0, 1.0, -16.0]] and (oh, ow) == (512, 672)      # 640 is a multiple of 32 and is padded
    # an odd-sized source, 75 x 51 (w x h): fix_res a = 75 / 64, centre (37.5, 25.5); keep_res centre (37, 25), out 64 x 96
    M, oh, ow = W.test_params(51, 75, "fix_res", (64, 64), 32)
    a = 75 / 64
    assert M.tolist() == [[a, 0.0, 37.5 - a * 32], [0.0, a, 25.5 - a * 32]] and M[0, 2] == 0.0 and M[1, 2] == -12.0
    M, oh, ow = W.test_params(51, 75, "keep_res", None, 32)
    assert M.tolist() == [[1.0, 0.0, 37.0 - 48.0], [0.0, 1.0, 25.0 - 32.0]] and (oh, ow) == (64, 96)
    M, oh, ow = W.test_params(51, 75, "keep_res", None, 8)
    assert (oh, ow) == (56, 80) and M.tolist() == [[1.0, 0.0, -3.0], [0.0, 1.0, -3.0]]
    # a non-square fix_res output: the window lands on the output's WIDTH
    M, oh, ow = W.test_params(60, 80, "fix_res", (64, 128), 32)
    assert M.tolist() == [[0.625, 0.0, 0.0], [0.0, 0.625, 10.0]] and (oh, ow) == (64, 128)
    # built on inverse_matrix, never flipped
    assert np.array_equal(W.test_params(51, 75, "fix_res", (64, 64), 32)[0], W.inverse_matrix(75.0, 37.5, 25.5, False, 75, 64, 64))
    p = W.unwarp_params(W.test_params(480, 640, "fix_res", (512, 512), 32)[0], (480, 640))
    assert p.dtype == np.float32 and p.tolist() == [1.25, 1.25, 0.0, -80.0, 640.0, 480.0]
    with pytest.raises(AssertionError, match="axis-aligned"):
        W.unwarp_params([[1, 0.1, 0], [0, 1, 0]], (4, 4))


@pytest.mark.parametrize("hw", [(50, 70), (64, 96), (33, 31), (1, 1)])
def test_keep_res_warp_is_an_exact_copy(hw):
    h, w = hw
    img = np.random.RandomState(h * 100 + w).randint(1, 256, (h, w, 3)).astype(np.uint8)      # no zero byte in the source
    M, oh, ow = W.test_params(h, w, "keep_res", None, 32)
    assert oh % 32 == 0 and ow % 32 == 0 and oh > h and ow > w and oh - h <= 32 and ow - w <= 32
    tx, ty = int(M[0, 2]), int(M[1, 2])
    assert (tx, ty) == (w // 2 - ow // 2, h // 2 - oh // 2) and tx <= 0 and ty <= 0
    out = W.warp_affine_u8_reference(img, M, oh, ow)
    assert np.array_equal(out[-ty:-ty + h, -tx:-tx + w], img)
    frame = out.copy()
    frame[-ty:-ty + h, -tx:-tx + w] = 0
    assert not frame.any()


@pytest.mark.parametrize("mode", ["fix_res", "keep_res"])
def test_box_round_trip(mode):
    """the unwarp is the inverse of the training box rule forward_coords(., M, False, w), in float64"""
    rng = np.random.RandomState(3)
    for h, w in ((480, 640), (51, 75), (70, 50)):
        M, oh, ow = W.test_params(h, w, mode, (64, 64), 32)
        p = np.array([M[0, 0], M[1, 1], M[0, 2], M[1, 2]])
        assert np.array_equal(W.unwarp_params(M, (h, w))[:4], p.astype(np.float32))
        pts = rng.uniform(-5, 70, (20, 2))                           # points of the network input
        src = pts * p[:2] + p[2:]                                    # ... unwarped
        back = W.forward_coords(src, M, False, w)
        assert np.abs(back - pts).max() <= 1e-12 * 70
        corners = W.forward_coords([[0, 0], [w, h]], M, False, w)      # the content rectangle lies inside the network frame
        assert (corners >= -1e-9).all() and corners[1, 0] <= ow + 1e-9 and corners[1, 1] <= oh + 1e-9


# -------------------------------------------------------------------------------------------------------------- records
def _write_images(root, sizes):
    rng = np.random.RandomState(7)
    recs = []
    for i, (h, w) in enumerate(sizes):
        path = os.path.join(str(root), f"im{i}.png")
        Image.fromarray(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(path)
        recs.append({"file_name": path, "image_id": i, "height": h, "width": w,
                     "annotations": [{"bbox": [w // 4, h // 4, w // 3, h // 3], "bbox_mode": 1, "category_id": 1, "iscrowd": 0}]})
    return recs


@pytest.mark.parametrize("mode", ["fix_res", "keep_res"])
def test_host_and_raw_records(tmp_path, mode):
    recs = _write_images(tmp_path, [(60, 80), (70, 50), (51, 75)])
    host_mapper = TrafficLightDatasetMapper(_cfg(mode, raw=False), is_train=False)
    raw_mapper = TrafficLightDatasetMapper(_cfg(mode, raw=True), is_train=False)
    before = [dict(r) for r in recs]
    for rec in recs:
        h, w = rec["height"], rec["width"]
        host, raw = host_mapper(rec), raw_mapper(rec)
        M, oh, ow = W.test_params(h, w, mode, (64, 64), 32)
        for r in (host, raw):
            assert isinstance(r["warp"], torch.Tensor) and r["warp"].dtype == torch.float64
            assert np.array_equal(r["warp"].numpy(), W.pack_warp(M, False)) and (r["height"], r["width"]) == (h, w)
            assert "annotations" not in r and "instances" not in r
        assert torch.equal(host["warp"], raw["warp"])
        assert "image" not in raw and "image_raw" not in host and "resize_hw" not in host
        assert tuple(raw["resize_hw"]) == (oh, ow) and raw["image_raw"].shape == (h, w, 3) and raw["image_raw"].dtype == np.uint8
        assert host["image"].dtype == torch.uint8 and tuple(host["image"].shape) == (3, oh, ow)
        if mode == "fix_res":
            assert (oh, ow) == (64, 64)
        want = W.warp_affine_u8_reference(raw["image_raw"], M, oh, ow)
        assert np.array_equal(host["image"].numpy().transpose(1, 2, 0), want) and want.any()
    assert recs == before      # the caller's dicts are never modified


def test_default_mode_leaves_the_test_mapper_as_it_was(tmp_path):
    rec = _write_images(tmp_path, [(60, 80)])[0]
    cfg = get_cfg()
    cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = 48, 100
    out = TrafficLightDatasetMapper(cfg, is_train=False)(rec)
    assert "warp" not in out and tuple(out["image"].shape) == (3, 48, 64)
    cfg.INPUT.DEVICE_RESIZE = True
    out = TrafficLightDatasetMapper(cfg, is_train=False)(rec)
    assert "warp" not in out and tuple(out["resize_hw"]) == (48, 64)


# --------------------------------------------------------------------------------------------------------------- oracle
def test_oracle_hand_derived_case():
    """640 x 480 under fix_res 512 x 512: a = 1.25, ty = -80; the box (0, 64, 512, 448) of the network input is the whole image"""
    p = W.unwarp_params(W.test_params(480, 640, "fix_res", (512, 512), 32)[0], (480, 640))
    b, s, c = W.unwarp_boxes_reference([[0, 64, 512, 448], [256, 256, 384, 320], [-8, 0, 520, 512], [0, 0, 512, 60]],
                                       [0.9, 0.8, 0.7, 0.6], [4, 5, 6, 7], 100, 0.5, p)
    assert b.dtype == np.float32 and b.tolist() == [[0, 0, 640, 480], [320, 240, 480, 320], [0, 0, 640, 480]]      # row 3: y in (-80, -5)
    assert s.tolist() == [np.float32(0.9), np.float32(0.8), np.float32(0.7)] and c.tolist() == [4, 5, 6]
    assert [len(W.unwarp_boxes_reference([[0, 64, 512, 448]] * 3, [0.9] * 3, [1, 2, 3], md, 0.5, p)[1]) for md in (0, 2, 3, 9)] == [0, 2, 3, 3]
    assert len(W.unwarp_boxes_reference([[0, 64, 512, 448]], [0.5], [1], 1, 0.5, p)[1]) == 0       # score == thresh is dropped
    assert "inverse of the training box rule" in W.unwarp_boxes_reference.__doc__ and "forward_coords" in W.unwarp_boxes_reference.__doc__


@pytest.mark.parametrize("case", UC.CASES, ids=UC.CASE_IDS)
def test_oracle_against_float64(case):
    """every kept row against the float64 evaluation of the same map and clip.  Bound, one rounding per operation with
    u = 2^-24: |f32(x s) - x s| <= u |x s| and |f32(q + t) - (q + t)| <= u |q + t| for q = f32(x s), so the error before the
    clip is at most u (|x s| + |q + t|) <= u (2 |x s| + |t|) (1 + u); the clip to [0, hi] does not enlarge a difference"""
    inp, ref = UC.inputs(case), UC.reference(case)
    u = 2.0 ** -24
    for b in range(case.B):
        boxes, scores, classes = ref[b]
        p = inp["params"][b].astype(np.float64)
        s, t, hi = p[[0, 1, 0, 1]], p[[2, 3, 2, 3]], p[[4, 5, 4, 5]]
        x = inp["boxes"][b][classes].astype(np.float64)      # the class is the row's number
        with np.errstate(invalid="ignore"):
            want = np.clip(x * s + t, 0.0, hi)
            bound = u * (2 * np.abs(x * s) + np.abs(t)) * (1 + u)
        finite = np.isfinite(x)
        assert (np.abs(boxes.astype(np.float64) - want)[finite] <= bound[finite]).all(), case.name
        assert np.array_equal(boxes[~finite], want[~finite].astype(np.float32))      # an infinite corner sits on the frame
        assert np.array_equal(scores, inp["scores"][b][classes]) and (np.diff(classes) > 0).all()
        assert len(classes) <= min(case.K, case.max_det) and (classes < case.max_det).all()
        assert (boxes >= 0).all() and (boxes <= hi.astype(np.float32)).all() and not np.isnan(scores).any()


# ------------------------------------------------------------------------------------------------------------- refusals
def test_tta_refusals():
    from detectron2_centernet_amd.modeling import CenterNetWithTTA
    cfg = _cfg("fix_res")
    cfg.TEST.AUG.ENABLED, cfg.TEST.AUG.FLIP, cfg.TEST.AUG.MIN_SIZES = True, True, (512,)
    with pytest.raises(NotImplementedError, match=r"TEST\.AUG\.MIN_SIZES=\(512,\) with INPUT\.AFFINE\.TEST_MODE='fix_res'"):
        CenterNetWithTTA(cfg, None)
    cfg.TEST.AUG.MIN_SIZES = (400, 512)
    cfg.TEST.SOFT_NMS.ENABLED = True
    with pytest.raises(NotImplementedError, match=r"TEST\.AUG\.MIN_SIZES=\(400, 512\) with INPUT\.AFFINE\.TEST_MODE"):
        CenterNetWithTTA(cfg, None)
    cfg.TEST.AUG.MIN_SIZES = ()
    with pytest.raises(NotImplementedError, match=r"TEST\.SOFT_NMS\.ENABLED with INPUT\.AFFINE\.TEST_MODE='fix_res'"):
        CenterNetWithTTA(cfg, None)
    # the flip test alone passes the check and reaches the wrapper's own assertion on the model
    cfg.TEST.SOFT_NMS.ENABLED = False
    with pytest.raises(AssertionError, match="CenterNet meta-architecture"):
        CenterNetWithTTA(cfg, None)


def test_predictor_refuses_a_bad_mode_before_building_the_model():
    from detectron2_centernet_amd.engine import DefaultPredictor
    with pytest.raises(ValueError, match=r"INPUT\.AFFINE\.TEST_MODE 'letterbox'"):
        DefaultPredictor(_cfg("letterbox"))
    cfg = _cfg("keep_res")
    cfg.MODEL.CENTERNET.SIZE_DIVISIBILITY = 48
    with pytest.raises(ValueError, match="power of two, got 48"):
        DefaultPredictor(cfg)


def test_wrapper_refusals_without_a_gpu():
    z = torch.zeros(1, 2, 4)
    with pytest.raises(Exception, match="cuda|CUDA|device"):
        ops.postprocess_affine(z, torch.zeros(1, 2), torch.zeros(1, 2, dtype=torch.int32), 2, 0.1, torch.zeros(1, 6))


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_library_symbol_and_declarations():
    header = open(os.path.join(ROOT, "include", "ctdet_hip.h")).read()
    name = "ctdet_postprocess_affine"
    decls = re.findall(r"int32_t\s+" + name + r"\s*\(([^;]*)\);", header)
    assert len(decls) == 1 and len(decls[0].split(",")) == 13 and "img_params6" in decls[0]      # declared once
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, name) and name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 13
    assert _lib.SIGNATURES[name] == _lib.SIGNATURES["ctdet_postprocess"]
    assert _lib.lib().ctdet_abi_version() == 8
    mk = open(os.path.join(ROOT, "detectron2-centernet_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bunwarp\.hip\b", mk, re.M) and re.search(r"^FLAGS_unwarp\s*:=\s*-ffp-contract=off\b", mk, re.M)
    assert not re.search(r"^FLAGS_decode", mk, re.M)
    src = open(os.path.join(ROOT, "detectron2-centernet_amd", "csrc", "unwarp.hip")).read()
    assert "#define UNWARP_PARAMS 6" in src and "dec_postprocess_affine_kernel" in src


def test_entry_point_checks_its_arguments_and_names_its_kernel():
    """label mode 2 (dry run): the entry point checks, names the kernel and returns before the launch, so host buffers stand in"""
    L = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.c_void_p(ctypes.addressof(buf))
    null = ctypes.c_void_p(0)

    def call(B=1, K=4, **over):
        args = dict(boxes=p, scores=p, classes=p, params=p, ob=p, os=p, oc=p, counts=p)
        args.update(over)
        return L.ctdet_postprocess_affine(args["boxes"], args["scores"], args["classes"], B, K, 4, 0.5, args["params"], args["ob"],
                                          args["os"], args["oc"], args["counts"], None)
    assert L.ctdet_set_label_mode(2) == 0
    try:
        assert call() == 0 and L.ctdet_last_kernel_label().decode() == "dec_postprocess_affine_kernel"
        assert call(B=0) == 0                                                   # an empty batch launches nothing
        for K in (0, -3):
            assert call(K=K) == -22 and b"postprocess_affine" in L.ctdet_last_error() and b"K=" in L.ctdet_last_error()
        assert call(B=-1) == -22
        for arg in ("boxes", "scores", "classes", "params", "ob", "os", "oc", "counts"):
            assert call(**{arg: null}) == -22 and b"postprocess_affine: null pointer" in L.ctdet_last_error(), arg
    finally:
        L.ctdet_set_label_mode(0)
