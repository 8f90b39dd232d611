"""Host side of the device resize (INPUT.DEVICE_RESIZE): the integer restatement of Pillow's 8-bit bilinear resample and its
coefficient tables (data/resample.py) against Pillow itself, bit for bit; the raw records of the test-time mapper; the
inference sampler / loader; the two new entry points of the C ABI.  No GPU: the kernel is compared in test_resize_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest
from PIL import Image

import resize_cases as RC
from detectron2_centernet_amd import _lib, ops
from detectron2_centernet_amd.config import get_cfg
from detectron2_centernet_amd.data import (DatasetCatalog, InferenceSampler, TrafficLightDatasetMapper,
                                           build_detection_test_loader)
from detectron2_centernet_amd.data import resample
from detectron2_centernet_amd.data import transforms as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = list(RC.all_inputs())


@pytest.mark.parametrize("image,new", [pytest.param(img, new, id=cid) for cid, img, new in INPUTS])
def test_reference_equals_pillow_bit_for_bit(image, new):
    H, W = image.shape[:2]
    want = T.ResizeTransform(H, W, new[0], new[1]).apply_image(image)      # PIL.Image.resize(..., BILINEAR)
    got = resample.resize_u8_reference(image, new[0], new[1])
    assert got.shape == want.shape == (new[0], new[1], 3) and got.dtype == np.uint8
    assert int((got != want).sum()) == 0
    if (image == 255).all():
        assert (want == 255).all() and (got == 255).all()      # the coefficient sums round to 2**22


def test_cases_cover_what_they_claim():
    names = {c[0]: c for c in RC.CASES}
    assert len(RC.CASES) == 9 and len(INPUTS) == 27
    assert names["partial_tile"][2][1] == RC.COL_TILE + 1
    src = open(os.path.join(ROOT, "detectron2-centernet_amd", "csrc", "resize.hip")).read()
    assert int(re.search(r"#define RESIZE_TW (\d+)", src).group(1)) == RC.COL_TILE == ops.RESIZE_TW
    assert int(re.search(r"#define RESIZE_RB (\d+)", src).group(1)) == ops.RESIZE_RB
    assert names["one_row"][1][1] == names["one_row"][2][1] and names["v_skipped"][1][0] == names["v_skipped"][2][0]
    H, new_h = names["long_span"][1][0], names["long_span"][2][0]
    assert resample.bilinear_tables(H, new_h)[0][:, 1].max() > 400       # taps of one output row: far beyond any tile


@pytest.mark.parametrize("in_size,out_size", sorted({(c[1][a], c[2][a]) for c in RC.CASES for a in (0, 1)}))
def test_tables(in_size, out_size):
    bounds, coeffs = resample.bilinear_tables(in_size, out_size)
    ksize = 2 * int(np.ceil(max(in_size / out_size, 1.0))) + 1
    assert bounds.shape == (out_size, 2) and coeffs.shape == (out_size, ksize)
    assert bounds.dtype == np.int32 and coeffs.dtype == np.int32
    first, count = bounds[:, 0].astype(np.int64), bounds[:, 1].astype(np.int64)
    assert (first >= 0).all() and (count >= 1).all() and (count <= ksize).all() and (first + count <= in_size).all()
    assert (coeffs >= 0).all()                                             # bilinear has no negative weights
    assert (np.abs(coeffs.sum(axis=1, dtype=np.int64) - (1 << 22)) <= ksize).all()
    taps = np.arange(ksize)[None, :]
    assert (coeffs[taps >= count[:, None]] == 0).all()                     # zero padded behind the taps
    assert resample.bilinear_tables(in_size, out_size)[1] is coeffs        # cached per (in, out)
    with pytest.raises(ValueError):
        coeffs[0, 0] = 1                                                   # and shared: read only


def test_identity_tables_are_the_identity():
    """a pass whose size does not change is skipped; the tables of such a pass would give the same bytes (weight 2**22 on
    the pixel itself), so a caller that runs it anyway is not wrong"""
    bounds, coeffs = resample.bilinear_tables(9, 9)
    assert (bounds[:, 0] == np.arange(9)).all() and (coeffs[:, 0] == 1 << 22).all() and (coeffs[:, 1:] == 0).all()


def _write_images(root, sizes):
    rng = np.random.RandomState(3)
    recs = []
    for i, (h, w) in enumerate(sizes):
        arr = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        arr[0, 0] = (200, 100, 50)      # RGB marker pixel
        path = os.path.join(str(root), f"im{i}.png")
        Image.fromarray(arr).save(path)
        recs.append({"file_name": path, "image_id": i, "height": h, "width": w,
                     "annotations": [{"bbox": [1, 1, 5, 5], "bbox_mode": 1, "category_id": 0, "iscrowd": 0}]})
    return recs


def _cfg(test_size=40, max_size=1333, fmt="BGR", device_resize=True):
    cfg = get_cfg()
    cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST, cfg.INPUT.FORMAT = test_size, max_size, fmt
    cfg.INPUT.DEVICE_RESIZE = device_resize
    return cfg


@pytest.mark.parametrize("fmt", ["BGR", "RGB"])
@pytest.mark.parametrize("test_size,max_size", [(40, 1333), (80, 100)])
def test_mapper_emits_raw_records(tmp_path, fmt, test_size, max_size):
    assert get_cfg().INPUT.DEVICE_RESIZE is False
    recs = _write_images(tmp_path, [(60, 90), (70, 50)])
    for rec in recs:
        raw = TrafficLightDatasetMapper(_cfg(test_size, max_size, fmt), is_train=False)(rec)
        host = TrafficLightDatasetMapper(_cfg(test_size, max_size, fmt, device_resize=False), is_train=False)(rec)
        assert "image" not in raw and "annotations" not in raw and "instances" not in raw and "annotations" in rec
        assert (raw["height"], raw["width"]) == (host["height"], host["width"]) == (rec["height"], rec["width"])
        img = raw["image_raw"]
        assert isinstance(img, np.ndarray) and img.dtype == np.uint8 and img.shape == (rec["height"], rec["width"], 3)
        assert img[0, 0].tolist() == ([50, 100, 200] if fmt == "BGR" else [200, 100, 50])      # channel order INPUT.FORMAT
        assert tuple(raw["resize_hw"]) == tuple(host["image"].shape[-2:])
        # the raw record resized by the restatement IS the host record
        got = resample.resize_u8_reference(img, *raw["resize_hw"])
        assert np.array_equal(got.transpose(2, 0, 1), host["image"].numpy())


def test_training_mapper_refuses_the_key():
    with pytest.raises(NotImplementedError, match="INPUT.DEVICE_RESIZE"):
        TrafficLightDatasetMapper(_cfg(), is_train=True)
    TrafficLightDatasetMapper(_cfg(device_resize=False), is_train=True)


def test_test_loader_yields_every_record_once_in_order(tmp_path):
    name = "resize_host_loader"
    recs = _write_images(tmp_path, [(30 + i, 40) for i in range(7)])
    if name not in DatasetCatalog:
        DatasetCatalog.register(name, lambda: recs)
    cfg = _cfg()
    cfg.TEST.BATCH_SIZE = 2
    assert list(InferenceSampler(7, 0, 2)) == [0, 2, 4, 6] and list(InferenceSampler(7, 1, 2)) == [1, 3, 5]
    assert len(InferenceSampler(7, 1, 2)) == 3
    seen = []
    for rank in (0, 1):
        loader = build_detection_test_loader(cfg, name, rank=rank, world_size=2, num_workers=0)
        batches = list(loader)
        assert all(isinstance(b, list) for b in batches)                      # the trivial collator
        assert [len(b) for b in batches] == ([2, 2] if rank == 0 else [2, 1])   # TEST.BATCH_SIZE, last one shorter
        ids = [r["image_id"] for b in batches for r in b]
        assert ids == sorted(ids)
        assert all("image_raw" in r and "resize_hw" in r for b in batches for r in b)      # the default mapper, from cfg
        seen += ids
    assert sorted(seen) == list(range(7))
    one = list(build_detection_test_loader(cfg, name, mapper=lambda d: d["image_id"], num_workers=0))
    assert one == [[0, 1], [2, 3], [4, 5], [6]]
    DatasetCatalog.remove(name)


def test_entry_points_are_declared_once():
    header = open(os.path.join(ROOT, "include", "ctdet_hip.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("ctdet_resize_bilinear_u8", 3), ("ctdet_resize_bilinear_u8_batch", 5)):
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*)\);", header)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs and hasattr(raw, name)
    assert _lib.lib().ctdet_abi_version() == 8
    # the descriptor: the header's fields in the header's order, in the ctypes mirror and in the numpy record
    body = re.search(r"typedef struct ctdet_resize_desc \{(.*?)\} ctdet_resize_desc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip().lstrip("*") for decl in body.split(";") if decl.strip()
              for f in re.sub(r"^\s*(const\s+)?\w+\*?\s", "", decl.strip()).split(",")]
    assert fields == [f[0] for f in _lib.ResizeDesc._fields_] == list(ops.RESIZE_DESC_DTYPE.names)
    assert ctypes.sizeof(_lib.ResizeDesc) == ops.RESIZE_DESC_DTYPE.itemsize == 112
    for f, _ in _lib.ResizeDesc._fields_:
        assert getattr(_lib.ResizeDesc, f).offset == ops.RESIZE_DESC_DTYPE.fields[f][1], f
    mk = open(os.path.join(ROOT, "detectron2-centernet_amd", "csrc", "Makefile")).read()
    assert "resize.hip" in mk and "FLAGS_resize" not in mk
    # refused before anything is launched: null pointers, a skipped pass whose size changes
    l = _lib.lib()
    d = _lib.ResizeDesc(src=1 << 20, dst=1 << 21, H=4, W=4, new_h=4, new_w=5, kh=0, kv=0)
    assert l.ctdet_resize_bilinear_u8(ctypes.byref(d), None, None) == -22 and b"skipped" in l.ctdet_last_error()
    assert l.ctdet_resize_bilinear_u8(None, None, None) == -22
    assert l.ctdet_resize_bilinear_u8_batch(None, 1, 1, None, None) == -22
