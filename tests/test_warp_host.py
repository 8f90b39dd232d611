"""Host side of CenterNet's random scale-and-crop training input (INPUT.AFFINE, data/warp.py): the warp arithmetic at its
known answers and against a scalar per-pixel restatement, the sampler's draws, the box rule, the two kinds of training
record from one seed, and the new entry point of the C ABI.  No GPU: the kernel is compared in test_warp_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

import warp_cases as WC
from detectron2_centernet_amd import _lib, ops
from detectron2_centernet_amd.config import get_cfg
from detectron2_centernet_amd.data import TrafficLightDatasetMapper, dataset_mapper
from detectron2_centernet_amd.data import detection_utils as du
from detectron2_centernet_amd.data import transforms as T
from detectron2_centernet_amd.data import warp as W
from detectron2_centernet_amd.structures import BoxMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENT = [[1, 0, 0], [0, 1, 0]]


# ---------------------------------------------------------------------------------------------------------------- bytes
def test_identity_returns_the_source():
    img = WC.make_image(12, 20, seed=1)
    assert np.array_equal(W.warp_affine_u8_reference(img, IDENT, 12, 20), img)


def test_shift_returns_the_shifted_source_with_zero_borders():
    img = WC.make_image(9, 11, seed=2)
    got = W.warp_affine_u8_reference(img, [[1, 0, 3], [0, 1, -2]], 9, 11)
    want = np.zeros_like(img)
    want[2:, :8] = img[:7, 3:]      # destination (x, y) reads source (x + 3, y - 2)
    assert np.array_equal(got, want)


def test_diag_33_over_32_visits_every_phase_pair():
    ax, bx, x0, y0 = (t.astype(np.int64) for t in W.warp_tables([[33 / 32, 0, 0], [0, 33 / 32, 0]], 32, 32))
    X, Y = (x0[:, None] + ax[None, :]) >> 5, (y0[:, None] + bx[None, :]) >> 5
    assert len({(int(fx), int(fy)) for fx, fy in zip((X & 31).ravel(), (Y & 31).ravel())}) == 1024


def test_half_scale_row_known_answer():
    row = np.array([0, 100, 200], dtype=np.uint8).reshape(1, 3, 1)
    got = W.warp_affine_u8_reference(row, [[0.5, 0, 0], [0, 1, 0]], 1, 6)
    assert got.reshape(-1).tolist() == [0, 50, 100, 150, 200, 100]


def test_a_map_entirely_outside_gives_zeros():
    img = np.full((9, 9, 3), 255, dtype=np.uint8)
    assert not W.warp_affine_u8_reference(img, [[1, 0, 500.0], [0, 1, -300.0]], 8, 8).any()


def test_flipped_identity_is_the_mirrored_source():
    img = WC.make_image(7, 13, seed=3)
    assert np.array_equal(W.warp_affine_u8_reference(img, IDENT, 7, 13, flip=True), img[:, ::-1])


@pytest.mark.parametrize("case", list(WC.case_inputs()), ids=WC.CASE_IDS)
def test_vectorised_reference_equals_the_scalar_restatement(case):
    name, img, M, flip, (oh, ow) = case
    got = W.warp_affine_u8_reference(img, M, oh, ow, flip)
    want = WC.warp_scalar(img, M, oh, ow, flip)
    assert got.dtype == np.uint8 and got.shape == want.shape == (oh, ow, 3)
    assert np.array_equal(got, want), f"{name}: {int((got != want).sum())} bytes differ"


def test_cases_cover_what_they_claim():
    src = open(os.path.join(ROOT, "detectron2-centernet_amd", "csrc", "warp.hip")).read()
    assert int(re.search(r"#define WARP_TW (\d+)", src).group(1)) == WC.COL_TILE == ops.WARP_TW
    assert int(re.search(r"#define WARP_RB (\d+)", src).group(1)) == WC.ROW_TILE == ops.WARP_RB
    by = {c[0]: c for c in WC.CASES}
    assert by["borders"][1:3] == ((5, 7), (8, 8)) and by["seams"][2] == (9, 65) and by["all_phases"][2] == (32, 32)
    assert by["downscale"][3][0][0] == by["downscale"][3][1][1] == 3.5
    for name, img, M, flip, (oh, ow) in WC.case_inputs():
        ax, bx, x0, y0 = (t.astype(np.int64) for t in W.warp_tables(M, oh, ow))
        sx, sy = (x0[:, None] + ax[None, :]) >> 10, (y0[:, None] + bx[None, :]) >> 10
        H, Wd = img.shape[:2]
        if name == "borders":      # taps one before and one past the source on both axes, and pixels with no tap inside
            assert sx.min() < -1 and sy.min() < -1 and (sx == -1).any() and (sy == -1).any()
            assert (sx == Wd - 1).any() and (sy == H - 1).any() and sx.max() >= Wd and sy.max() >= H
        if name == "rotation":
            assert all(len(set(np.diff(t).tolist())) > 1 or np.diff(t)[0] != 0 for t in (ax, bx, x0, y0))
            assert bx.any() and len(set(x0.tolist())) > 1
        if name in ("outside", "int32_limit"):
            assert not W.warp_affine_u8_reference(img, M, oh, ow, flip).any()
        if name == "int32_limit":
            assert int(x0[0]) == int(ax[1]) == 2 ** 31 - 1 and ((int(x0[0]) + int(ax[1])) & 0xFFFFFFFF) - 2 ** 32 == -2
    assert len({hw for hw, _, _ in WC.BATCH}) == 3 and any(f for _, _, f in WC.BATCH)


def test_limits_are_refused():
    with pytest.raises(ValueError, match="int32"):
        W.warp_tables([[1, 0, 2.2e6], [0, 1, 0]], 4, 4)
    with pytest.raises(ValueError, match="16384"):
        W.warp_affine_u8_reference(np.zeros((1, 16385, 3), np.uint8), IDENT, 2, 2)
    W.warp_affine_u8_reference(np.zeros((1, 16384, 3), np.uint8), IDENT, 2, 2)
    if not torch.cuda.is_available():
        with pytest.raises(NotImplementedError, match="no CPU implementation"):
            ops.warp_affine_u8([torch.zeros(3, 4, 4, dtype=torch.uint8)], [(IDENT, False)], (4, 4))
    assert ops.warp_affine_u8([], [], (4, 4)) == []


# -------------------------------------------------------------------------------------------------------------- sampler
def test_border():
    assert WC.BORDER_VALUES == {64: 16, 100: 32, 255: 64, 256: 64, 257: 128, 480: 128}
    for size, want in WC.BORDER_VALUES.items():
        assert W.border(128, size) == want, size
    assert W.border(128, 1) == 0 and W.border(0, 5) == 0


def test_config_defaults():
    a = get_cfg().INPUT.AFFINE
    assert a.ENABLED is False and tuple(a.OUTPUT_SIZE) == (512, 512) and a.BORDER == 128 and a.FLIP_PROB == 0.5
    assert tuple(a.SCALES) == (0.6, 0.7, 0.8, 0.9, 1.0, 1.1, 1.2, 1.3)      # the literals, not np.arange's floats


def _affine_cfg(device_augment=False, out=(64, 64), fmt="BGR"):
    cfg = get_cfg()
    cfg.INPUT.AFFINE.ENABLED = True
    cfg.INPUT.AFFINE.OUTPUT_SIZE = out
    cfg.INPUT.FORMAT = fmt
    cfg.INPUT.DEVICE_AUGMENT = device_augment
    return cfg


@pytest.mark.parametrize("hw", WC.SAMPLER_SIZES, ids=[f"{h}x{w}" for h, w in WC.SAMPLER_SIZES])
def test_draws_come_in_the_stated_order_and_centres_keep_the_border(hw):
    h, w = hw
    aug = T.RandomAffineCrop(_affine_cfg())
    scales = get_cfg().INPUT.AFFINE.SCALES
    bw, bh = W.border(128, w), W.border(128, h)
    np.random.seed(99)
    got = [aug.draw(h, w) for _ in range(200)]
    state = np.random.get_state()
    np.random.seed(99)
    for s, cx, cy, flip in got:
        k = np.random.randint(len(scales))
        assert s == max(h, w) * scales[k]
        assert cx == np.random.randint(bw, w - bw) and cy == np.random.randint(bh, h - bh)
        assert flip == (np.random.uniform(0, 1) < 0.5)
        assert bw <= cx < w - bw and bh <= cy < h - bh
    after = np.random.get_state()
    assert np.array_equal(state[1], after[1]) and state[2:] == after[2:]      # four draws per sample, no other
    assert len({g[0] for g in got}) == len(scales) and {g[3] for g in got} == {True, False}
    tenth = (w - 2 * bw) / 10      # the whole range is used: 200 draws reach its first and its last tenth
    assert min(g[1] for g in got) < bw + tenth and max(g[1] for g in got) >= w - bw - tenth


def test_inverse_matrix():
    M = W.inverse_matrix(128.0, 50, 40, False, 100, 64, 32)      # a = s / out_w = 4
    assert M.dtype == np.float64 and M.tolist() == [[4.0, 0.0, 50 - 64.0], [0.0, 4.0, 40 - 128.0]]
    assert W.inverse_matrix(128.0, 50, 40, True, 100, 64, 32).tolist() == [[4.0, 0.0, 49 - 64.0], [0.0, 4.0, 40 - 128.0]]
    with pytest.raises(ValueError, match="SIZE_DIVISIBILITY"):
        T.RandomAffineCrop(_affine_cfg(out=(64, 70)))


# ---------------------------------------------------------------------------------------------------------------- boxes
def _boxes_through(t, boxes, hw):
    annos = [du.transform_instance_annotations({"bbox": list(b), "bbox_mode": BoxMode.XYXY_ABS, "category_id": i}, t, hw)
             for i, b in enumerate(boxes)]
    inst = du.filter_empty_instances(du.annotations_to_instances(annos, hw))
    return inst.gt_boxes.tensor.tolist(), inst.gt_classes.tolist()


def test_box_known_answers():
    img = np.zeros((80, 100, 3), np.uint8)
    aug = T.RandomAffineCrop(_affine_cfg())
    # s = 128 -> a = 2: the window covers the whole source; plain, then flipped (x1' = 99 - x2, x2' = 99 - x1)
    t = aug.transform_of((128.0, 50, 40, False), img)
    assert isinstance(t, T.AffineTransform) and t.Minv.tolist() == [[2.0, 0.0, -14.0], [0.0, 2.0, -24.0]]
    assert _boxes_through(t, [(20, 10, 60, 50)], (64, 64)) == ([[17.0, 17.0, 37.0, 37.0]], [0])
    t = aug.transform_of((128.0, 50, 40, True), img)
    assert t.flip and t.Minv.tolist() == [[2.0, 0.0, -15.0], [0.0, 2.0, -24.0]]
    assert _boxes_through(t, [(20, 10, 60, 50)], (64, 64)) == ([[27.0, 17.0, 47.0, 37.0]], [0])
    # s = 64 -> a = 1: the window is source columns 18 .. 82, rows 8 .. 72: one box cut by the frame, one outside and dropped
    t = aug.transform_of((64.0, 50, 40, False), img)
    assert _boxes_through(t, [(10, 20, 40, 60), (0, 0, 15, 7), (30, 30, 40, 40)], (64, 64)) == (
        [[0.0, 12.0, 22.0, 52.0], [12.0, 22.0, 22.0, 32.0]], [0, 2])
    # the image and the boxes move together: a marked source pixel lands where its coordinate maps
    img[40, 60] = 255
    out = aug.transform_of((64.0, 50, 40, True), img).apply_image(img)
    x, y = aug.transform_of((64.0, 50, 40, True), img).apply_coords(np.array([[60.0, 40.0]]))[0]
    assert (x, y) == (99 - 60 - 49 + 32, 32) and out[int(y), int(x)].tolist() == [255] * 3 and int(out.astype(int).sum()) == 3 * 255


# -------------------------------------------------------------------------------------------------------------- records
def _write_images(root, sizes):
    rng = np.random.RandomState(7)
    recs = []
    for i, (h, w) in enumerate(sizes):
        path = os.path.join(str(root), f"im{i}.png")
        Image.fromarray(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(path)
        recs.append({"file_name": path, "image_id": i, "height": h, "width": w,
                     "annotations": [{"bbox": [w // 4, h // 4, w // 3, h // 3], "bbox_mode": 1, "category_id": 1, "iscrowd": 0},
                                     {"bbox": [w // 2, h // 2, w // 4, h // 5], "bbox_mode": 1, "category_id": 0, "iscrowd": 0},
                                     {"bbox": [2, 2, 8, 8], "bbox_mode": 1, "category_id": 2, "iscrowd": 1}]})
    return recs


@pytest.mark.parametrize("prob", [1.0, None], ids=["all_on", "p0.15"])
def test_host_and_raw_records_come_from_the_same_draws(tmp_path, monkeypatch, prob):
    if prob is not None:
        monkeypatch.setattr(dataset_mapper, "_JITTER_PROB", prob)
    recs = _write_images(tmp_path, [(48, 80), (100, 60), (70, 255)])
    seq = [recs[i % 3] for i in range(12)]
    raw_mapper = TrafficLightDatasetMapper(_affine_cfg(True), is_train=True)
    host_mapper = TrafficLightDatasetMapper(_affine_cfg(False), is_train=True)
    captured = []
    real = host_mapper._image

    def spy(record):
        pixels, transforms = real(record)
        captured.append(transforms)
        return pixels, transforms

    host_mapper._image = spy
    np.random.seed(4321)
    raw_out = [raw_mapper(r) for r in seq]
    raw_state = np.random.get_state()
    np.random.seed(4321)
    host_out = [host_mapper(r) for r in seq]
    host_state = np.random.get_state()
    assert raw_state[0] == host_state[0] and np.array_equal(raw_state[1], host_state[1]) and raw_state[2:] == host_state[2:]
    from test_jitter_host import _host_spec
    flips = 0
    for raw, host, tfms, rec in zip(raw_out, host_out, captured, seq):
        aff = tfms.transforms[0]
        assert isinstance(aff, T.AffineTransform)
        warp = raw["warp"]
        assert isinstance(warp, torch.Tensor) and warp.dtype == torch.float64 and tuple(warp.shape) == (2, 4)
        M, flip = W.unpack_warp(warp)
        assert np.array_equal(M, aff.Minv) and flip == aff.flip and M[0, 0] == M[1, 1] and M[0, 1] == M[1, 0] == 0
        flips += flip
        assert tuple(raw["resize_hw"]) == (64, 64) == tuple(host["image"].shape[-2:]) and host["image"].dtype == torch.uint8
        assert tuple(raw["image_raw"].shape) == (rec["height"], rec["width"], 3) and "image" not in raw
        assert np.array_equal(raw["jitter"].numpy(), _host_spec(tfms)[0])
        ri, hi = raw["instances"], host["instances"]
        assert ri.image_size == hi.image_size == (64, 64)
        assert torch.equal(ri.gt_boxes.tensor, hi.gt_boxes.tensor) and torch.equal(ri.gt_classes, hi.gt_classes)
        # the host image is the reference warp of the raw one, then the jitters
        warped = W.warp_affine_u8_reference(raw["image_raw"].numpy(), M, 64, 64, flip)
        want = T.TransformList(tfms.transforms[1:]).apply_image(warped)
        assert np.array_equal(host["image"].numpy(), want.transpose(2, 0, 1))
    assert 0 < flips < len(seq)


def test_disabled_pipeline_is_the_resize_and_the_four_jitters(tmp_path):
    for train_cfg in (get_cfg(), _affine_cfg()):
        train_cfg.INPUT.AFFINE.ENABLED = False
        pipe = dataset_mapper.bulb_traffic_light_augmentation(train_cfg, True)
        assert isinstance(pipe[0], T.ResizeShortestEdge) and len(pipe) == 5
        assert [type(p.aug).__name__ for p in pipe[1:]] == ["RandomContrast", "RandomBrightness", "RandomSaturation", "RandomLighting"]
    on = dataset_mapper.bulb_traffic_light_augmentation(_affine_cfg(), True)
    assert isinstance(on[0], T.RandomAffineCrop) and len(on) == 5 and all(isinstance(p, T.RandomApply) for p in on[1:])
    # the test-time mapper ignores the keys; INPUT.CROP stays refused
    test_pipe = dataset_mapper.bulb_traffic_light_augmentation(_affine_cfg(), False)
    assert len(test_pipe) == 1 and isinstance(test_pipe[0], T.ResizeShortestEdge)
    rec = _write_images(tmp_path, [(48, 80)])[0]
    out = TrafficLightDatasetMapper(_affine_cfg(True), is_train=False)(rec)
    assert "image" in out and "warp" not in out and "image_raw" not in out
    from detectron2_centernet_amd.config import CfgNode as CN
    crop = _affine_cfg()
    crop.INPUT.CROP = CN()
    crop.INPUT.CROP.ENABLED = True
    with pytest.raises(NotImplementedError, match="INPUT.CROP"):
        TrafficLightDatasetMapper(crop, is_train=True)


# ------------------------------------------------------------------------------------------------------------------ ABI
def test_entry_point_and_descriptor():
    header = open(os.path.join(ROOT, "include", "ctdet_hip.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    name = "ctdet_warp_affine_u8_batch"
    m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*)\);", header)
    assert m and len(m.group(1).split(",")) == 5
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 5 and hasattr(raw, name)
    assert _lib.lib().ctdet_abi_version() == 8
    body = re.search(r"typedef struct ctdet_warp_desc \{(.*?)\} ctdet_warp_desc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip().lstrip("*") for decl in body.split(";") if decl.strip()
              for f in re.sub(r"^\s*(const\s+)?\w+\*?\s", "", decl.strip()).split(",")]
    assert fields == [f[0] for f in _lib.WarpDesc._fields_] == list(ops.WARP_DESC_DTYPE.names)
    assert ctypes.sizeof(_lib.WarpDesc) == ops.WARP_DESC_DTYPE.itemsize == 104
    for f in ops.WARP_DESC_DTYPE.names:
        assert getattr(_lib.WarpDesc, f).offset == ops.WARP_DESC_DTYPE.fields[f][1], f
    mk = open(os.path.join(ROOT, "detectron2-centernet_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bwarp\.hip\b", mk, re.M)
    # refused, with a message, before anything is launched (the pointers are never read: any non-null value will do)
    l, p = _lib.lib(), ctypes.c_void_p(1 << 20)
    assert l.ctdet_warp_affine_u8_batch(None, 1, 1, p, None) == -22 and b"null" in l.ctdet_last_error()
    assert l.ctdet_warp_affine_u8_batch(p, 1, 1, None, None) == -22 and b"null" in l.ctdet_last_error()
    assert l.ctdet_warp_affine_u8_batch(p, -1, 0, p, None) == -22 and b"n=-1" in l.ctdet_last_error()
    assert l.ctdet_warp_affine_u8_batch(p, 3, 2, p, None) == -22 and b"not the sum" in l.ctdet_last_error()
    assert l.ctdet_warp_affine_u8_batch(p, 0, 0, p, None) == 0      # n = 0: nothing is launched
