"""Host side of the device colour jitter (INPUT.DEVICE_AUGMENT): the per-byte restatement of the jitters' arithmetic
(data/jitter.py) against the chain of host BlendTransforms, byte for byte; the raw records of the training mapper and the
random draws it makes against the host mapper's; the two new entry points of the C ABI.  No GPU: the kernel is compared in
test_jitter_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

import jitter_cases as JC
from detectron2_centernet_amd import _lib, ops
from detectron2_centernet_amd.config import get_cfg
from detectron2_centernet_amd.data import TrafficLightDatasetMapper, dataset_mapper
from detectron2_centernet_amd.data import transforms as T
from detectron2_centernet_amd.data.jitter import JITTER_ORDER, colour_jitter_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = list(JC.all_cases())


def test_restatement_equals_the_host_chain_byte_for_byte():
    bad = {}
    for cid, img, params in CASES:
        want = JC.host_chain(img, params)
        got = colour_jitter_reference(img, JC.spec_of(params))
        assert got.shape == want.shape == img.shape and got.dtype == np.uint8
        n = int((got != want).sum())
        if n:
            bad[cid] = n
    assert len(CASES) == len(JC.SIZES) * len(JC.IMAGES) * len(JC.PARAMS) == 4 * 4 * 15
    assert not bad, f"mismatching bytes per case {bad}"


def test_cases_cover_what_they_claim():
    src = open(os.path.join(ROOT, "detectron2-centernet_amd", "csrc", "jitter.hip")).read()
    assert int(re.search(r"#define JITTER_TW (\d+)", src).group(1)) == JC.TILE_W == ops.JITTER_TW
    assert int(re.search(r"#define JITTER_TH (\d+)", src).group(1)) == JC.TILE_H == ops.JITTER_TH
    assert [s[1] for s in JC.SIZES] == [(1, 1), (1, JC.TILE_W + 1), (JC.TILE_H + 1, 3), (37, 53)]
    assert 3 * JC.SUM_SIZE[0] * JC.SUM_SIZE[1] * 255 > 2 ** 32
    white, black = JC.make_image("white", 5, 3), JC.make_image("black", 5, 3)
    rnd = JC.make_image("random", 37, 53)
    # brightness at weight 1.0 is the identity; above 1 white stays clipped at 255
    assert np.array_equal(JC.host_chain(rnd, JC.PARAMS["brightness_1.0"]), rnd)
    assert (JC.host_chain(white, JC.PARAMS["brightness_1.2"]) == 255).all()
    assert (JC.host_chain(white, JC.PARAMS["contrast_1.2"]) == 255).all()
    assert not np.array_equal(JC.host_chain(rnd, JC.PARAMS["contrast_0.8"]), rnd)
    assert not np.array_equal(JC.host_chain(rnd, JC.PARAMS["saturation_1.2"]), rnd)
    # lighting: offsets of a few tenths -- on black a negative one clips at 0, a positive one truncates back to 0; on other
    # bytes the truncation is what the transform does
    assert (JC.LIGHT_POS > 0).all() and (JC.LIGHT_POS < 1).all() and (JC.LIGHT_NEG < 0).all() and (JC.LIGHT_NEG > -1).all()
    assert (JC.host_chain(black, JC.PARAMS["light_pos"]) == 0).all() and (JC.host_chain(black, JC.PARAMS["light_neg"]) == 0).all()
    assert np.array_equal(JC.host_chain(white, JC.PARAMS["light_neg"]), np.full_like(white, 254))
    assert np.array_equal(JC.host_chain(rnd, JC.PARAMS["none"]), rnd)


def _write_images(root, sizes):
    rng = np.random.RandomState(7)
    recs = []
    for i, (h, w) in enumerate(sizes):
        arr = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        arr[0, 0] = (200, 100, 50)      # RGB marker pixel
        path = os.path.join(str(root), f"im{i}.png")
        Image.fromarray(arr).save(path)
        recs.append({"file_name": path, "image_id": i, "height": h, "width": w,
                     "annotations": [{"bbox": [1, 1, 15, 12], "bbox_mode": 1, "category_id": 1, "iscrowd": 0},
                                     {"bbox": [10, 20, 30, 9], "bbox_mode": 1, "category_id": 0, "iscrowd": 0},
                                     {"bbox": [2, 2, 8, 8], "bbox_mode": 1, "category_id": 2, "iscrowd": 1}]})
    return recs, rng


def _cfg(device_augment, sizes=(48, 64), fmt="BGR"):
    cfg = get_cfg()
    cfg.INPUT.MIN_SIZE_TRAIN, cfg.INPUT.MIN_SIZE_TRAIN_SAMPLING, cfg.INPUT.MAX_SIZE_TRAIN = sizes, "choice", 100
    cfg.INPUT.FORMAT = fmt
    cfg.INPUT.DEVICE_AUGMENT = device_augment
    return cfg


def _host_spec(transforms):
    """the jitter parameters of a host record's transform list: (drawn, src_weight, dst_weight) per blend, lighting's
    offsets; which blend is which follows from its src_image"""
    spec = np.zeros((4, 4))
    blends = [t for t in transforms.transforms if isinstance(t, T.BlendTransform)]
    for b in blends:
        src = np.asarray(b.src_image)
        if src.ndim == 3:
            t = 2
        elif src.size == 3:
            t = 3
        else:
            t = 1 if isinstance(b.src_image, int) else 0      # brightness blends with the literal 0, contrast with a mean
        assert spec[t, 0] == 0
        spec[t, 0] = 1
        spec[t, 1:] = tuple(src) if t == 3 else (b.src_weight, b.dst_weight, 0.0)
    return spec, len(blends)


def _run_both(tmp_path, prob, n_records, monkeypatch):
    if prob is not None:
        monkeypatch.setattr(dataset_mapper, "_JITTER_PROB", prob)      # before construction
    recs, _ = _write_images(tmp_path, [(60, 90), (70, 50), (64, 64)])
    seq = [recs[i % len(recs)] for i in range(n_records)]
    raw_mapper = TrafficLightDatasetMapper(_cfg(True), is_train=True)
    host_mapper = TrafficLightDatasetMapper(_cfg(False), is_train=True)
    captured = []
    real = host_mapper._image

    def spy(record):
        pixels, transforms = real(record)
        captured.append(transforms)
        return pixels, transforms

    host_mapper._image = spy
    np.random.seed(1234)
    raw_out = [raw_mapper(r) for r in seq]
    raw_state = np.random.get_state()
    np.random.seed(1234)
    host_out = [host_mapper(r) for r in seq]
    host_state = np.random.get_state()
    assert raw_state[0] == host_state[0] and np.array_equal(raw_state[1], host_state[1]) and raw_state[2:] == host_state[2:]
    drawn = np.zeros(4, dtype=int)
    none_drawn = 0
    for raw, host, tfms in zip(raw_out, host_out, captured):
        assert tuple(raw["resize_hw"]) == tuple(host["image"].shape[-2:])
        want, nblends = _host_spec(tfms)
        got = raw["jitter"]
        assert isinstance(got, torch.Tensor) and got.dtype == torch.float64 and tuple(got.shape) == (4, 4)
        assert np.array_equal(got.numpy(), want), (got, want)           # exactly equal: the same float64 values
        assert int(want[:, 0].sum()) == nblends
        drawn += want[:, 0].astype(int)
        none_drawn += nblends == 0
        ri, hi = raw["instances"], host["instances"]
        assert ri.image_size == hi.image_size == tuple(raw["resize_hw"]) and len(ri) == len(hi) == 2      # the crowd box is gone
        assert torch.equal(ri.gt_boxes.tensor, hi.gt_boxes.tensor) and torch.equal(ri.gt_classes, hi.gt_classes)
        assert "annotations" not in raw and "image" not in raw
    return drawn, none_drawn, len(seq)


def test_mapper_draws_equal_the_host_mappers_with_every_jitter_on(tmp_path, monkeypatch):
    drawn, none_drawn, n = _run_both(tmp_path, 1.0, 4, monkeypatch)
    assert (drawn == n).all() and none_drawn == 0


def test_mapper_draws_equal_the_host_mappers_at_the_pipelines_probability(tmp_path, monkeypatch):
    assert dataset_mapper._JITTER_PROB == 0.15
    drawn, none_drawn, n = _run_both(tmp_path, None, 60, monkeypatch)
    print(f"records per transform {drawn.tolist()}, records with none {none_drawn} of {n}")
    assert (drawn >= 1).all() and none_drawn >= 1 and (drawn < n).all()


@pytest.mark.parametrize("fmt", ["BGR", "RGB"])
def test_raw_training_record(tmp_path, fmt):
    assert get_cfg().INPUT.DEVICE_AUGMENT is False
    recs, _ = _write_images(tmp_path, [(60, 90)])
    raw = TrafficLightDatasetMapper(_cfg(True, fmt=fmt), is_train=True)(recs[0])
    img = raw["image_raw"]
    assert isinstance(img, torch.Tensor) and img.dtype == torch.uint8 and tuple(img.shape) == (60, 90, 3) and img.is_contiguous()
    pixels = np.asarray(Image.open(recs[0]["file_name"]).convert("RGB"))
    assert np.array_equal(img.numpy(), pixels[:, :, ::-1] if fmt == "BGR" else pixels)      # channel order INPUT.FORMAT
    assert img[0, 0].tolist() == ([50, 100, 200] if fmt == "BGR" else [200, 100, 50])
    assert "image" not in raw and "annotations" not in raw and "annotations" in recs[0]
    assert set(raw) >= {"image_raw", "resize_hw", "jitter", "instances", "height", "width"}
    # the test-time mapper ignores the key
    test = TrafficLightDatasetMapper(_cfg(True, fmt=fmt), is_train=False)(recs[0])
    assert "image" in test and "image_raw" not in test and "jitter" not in test


def test_a_reordered_pipeline_is_refused_by_name(monkeypatch):
    assert tuple(a.__name__ for a, _ in dataset_mapper._COLOUR_JITTER) == JITTER_ORDER
    j = dataset_mapper._COLOUR_JITTER
    monkeypatch.setattr(dataset_mapper, "_COLOUR_JITTER", (j[1], j[0], j[2], j[3]))
    with pytest.raises(NotImplementedError, match="_COLOUR_JITTER"):
        TrafficLightDatasetMapper(_cfg(True), is_train=True)
    TrafficLightDatasetMapper(_cfg(False), is_train=True)       # the host pipeline takes any order
    TrafficLightDatasetMapper(_cfg(True), is_train=False)


def test_entry_points_and_descriptor():
    header = open(os.path.join(ROOT, "include", "ctdet_hip.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("ctdet_byte_sum_u8_batch", 5), ("ctdet_colour_jitter_u8_batch", 6)):
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*)\);", header)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs and hasattr(raw, name)
    assert _lib.lib().ctdet_abi_version() == 8
    body = re.search(r"typedef struct ctdet_jitter_desc \{(.*?)\} ctdet_jitter_desc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.sub(r"\[\d+\]", "", f).strip().lstrip("*") for decl in body.split(";") if decl.strip()
              for f in re.sub(r"^\s*(const\s+)?\w+\*?\s", "", decl.strip()).split(",")]
    assert fields == [f[0] for f in _lib.JitterDesc._fields_] == list(ops.JITTER_DESC_DTYPE.names)
    assert ctypes.sizeof(_lib.JitterDesc) == ops.JITTER_DESC_DTYPE.itemsize == 136
    for f in ops.JITTER_DESC_DTYPE.names:
        assert getattr(_lib.JitterDesc, f).offset == ops.JITTER_DESC_DTYPE.fields[f][1], f
    mk = open(os.path.join(ROOT, "detectron2-centernet_amd", "csrc", "Makefile")).read()
    assert "jitter.hip" in mk and re.search(r"FLAGS_jitter\s*:=\s*-ffp-contract=off", mk)      # no fused multiply-add
    # refused or finished before anything is launched
    l = _lib.lib()
    assert l.ctdet_colour_jitter_u8_batch(None, 0, 0, None, 0, None) == 0          # nothing drawn: nothing launched
    assert l.ctdet_colour_jitter_u8_batch(None, 1, 1, None, 0, None) == -22 and b"null" in l.ctdet_last_error()
    assert l.ctdet_colour_jitter_u8_batch(None, -1, 0, None, 0, None) == -22
    assert l.ctdet_byte_sum_u8_batch(None, 1, None, 1, None) == -22
    assert l.ctdet_byte_sum_u8_batch(None, 0, None, 0, None) == 0
