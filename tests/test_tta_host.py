"""Flip test-time augmentation (TEST.AUG), the parts that need no GPU: the config surface against the reference's defaults
(detectron2/config/defaults.py:634-638), the new entry points of the shared library (argument checks through the label dry
run, where nothing is launched and host addresses stand in for device pointers), the wrapper's refusals, and the definition
of "mirror the network input" against the oracle's preprocess."""
import ctypes as C
import glob
import os
import shutil

import numpy as np
import pytest
import torch

from detectron2_centernet_amd import _lib
from detectron2_centernet_amd._lib import DlaBaseDesc
from oracle import ctdet_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
_BUF = C.create_string_buffer(64)
BASE = (C.addressof(_BUF) + 15) & ~15       # a 16-byte aligned address to stand in for every device pointer


def test_test_aug_defaults_are_the_references():
    from detectron2_centernet_amd.config import get_cfg
    aug = get_cfg().TEST.AUG
    assert aug.ENABLED is False
    assert tuple(aug.MIN_SIZES) == (400, 500, 600, 700, 800, 900, 1000, 1100, 1200)
    assert aug.MAX_SIZE == 4000
    assert aug.FLIP is True
    assert sorted(aug.keys()) == ["ENABLED", "FLIP", "MAX_SIZE", "MIN_SIZES"]


def test_test_aug_keys_can_be_set():
    """a reference command line / yaml that switches TTA on (fails with `Non-existent config key` without TEST.AUG)"""
    from detectron2_centernet_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_list(["TEST.AUG.ENABLED", True])
    assert cfg.TEST.AUG.ENABLED is True
    cfg.merge_from_list(["TEST.AUG.MIN_SIZES", (512,), "TEST.AUG.MAX_SIZE", 1333, "TEST.AUG.FLIP", False])
    assert tuple(cfg.TEST.AUG.MIN_SIZES) == (512,) and cfg.TEST.AUG.MAX_SIZE == 1333 and cfg.TEST.AUG.FLIP is False


def test_test_aug_from_yaml(tmp_path):
    from detectron2_centernet_amd.config import get_cfg
    (tmp_path / "tta.yaml").write_text("TEST:\n  AUG:\n    ENABLED: True\n    MIN_SIZES: (608,)\nVERSION: 2\n")
    cfg = get_cfg()
    cfg.merge_from_file(str(tmp_path / "tta.yaml"))
    assert cfg.TEST.AUG.ENABLED is True and tuple(cfg.TEST.AUG.MIN_SIZES) == (608,) and cfg.TEST.AUG.FLIP is True


def test_golden_yamls_still_load(tmp_path):
    from detectron2_centernet_amd.config import get_cfg
    names = sorted(glob.glob(os.path.join(GOLDEN, "g16_configs", "*.yaml")) + glob.glob(os.path.join(GOLDEN, "g17_configs", "*.yaml")))
    assert len(names) >= 6
    for n in names:      # the g17 files name their base relative to themselves: one directory holds them all
        shutil.copy(n, tmp_path / os.path.basename(n))
    for n in names:
        cfg = get_cfg()
        cfg.merge_from_file(str(tmp_path / os.path.basename(n)))
        assert cfg.TEST.AUG.ENABLED is False and cfg.TEST.AUG.FLIP is True, n
        if os.path.basename(n) != "Base-CenterNet.yaml":
            assert cfg.MODEL.META_ARCHITECTURE == "CenterNet", n


def test_new_symbols_and_abi_version():
    L = _lib.lib()
    assert L.ctdet_abi_version() == 8
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("ctdet_decode_flip", "ctdet_preprocess_mirror", "ctdet_dla_base_mirror_fwd", "ctdet_dla_base_x3_mirror_fwd"):
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES
    header = open(os.path.join(os.path.dirname(HERE), "include", "ctdet_hip.h")).read()
    for name in ("ctdet_decode_flip(", "ctdet_preprocess_mirror(", "ctdet_dla_base_mirror_fwd(", "ctdet_dla_base_x3_mirror_fwd("):
        assert name in header, name
    # the flip decode takes ctdet_decode's arguments
    assert _lib.SIGNATURES["ctdet_decode_flip"] == _lib.SIGNATURES["ctdet_decode"]


def _base_desc(B=4, H=33, W=45, Hp=64, Wp=64, img_dtype=_lib.U8):
    d = DlaBaseDesc()
    d.B, d.H, d.W, d.Hp, d.Wp, d.img_dtype = B, H, W, Hp, Wp, img_dtype
    d.img_batch_stride = 3 * H * W
    for i in range(3):
        d.mean[i], d.std[i] = 0.4, 0.25
    d.out_stride = d.pool_stride = 32
    return d


def _base_call(fn, d, mirror_from):
    p = C.c_void_p(BASE)
    return getattr(_lib.lib(), fn)(C.byref(d), mirror_from, *([p] * 12), None)


@pytest.mark.parametrize("fn,label", [
    ("ctdet_dla_base_mirror_fwd", "dla_base_fused_kernel<u8|f32 -> 32ch,f16,mirror>"),
    ("ctdet_dla_base_x3_mirror_fwd", "dla_base_x3_kernel<u8|f32 -> 32ch,f16x3,mirror>"),
])
def test_mirrored_base_entry_points_in_a_dry_run(fn, label):
    L = _lib.lib()
    assert L.ctdet_set_label_mode(2) == 0
    try:
        for img_dtype in (_lib.U8, _lib.F32):
            for mirror_from in (0, 2, 4):      # every image mirrored / a flip-test batch / none
                assert _base_call(fn, _base_desc(img_dtype=img_dtype), mirror_from) == 0, L.ctdet_last_error()
                assert L.ctdet_last_kernel_label().decode() == label
        for bad in (-1, 5, 1 << 20):
            assert _base_call(fn, _base_desc(), bad) != 0
            assert b"mirror_from" in L.ctdet_last_error()
        # what the plain entry points reject, these reject too (padded size not a multiple of the tile)
        assert _base_call(fn, _base_desc(Hp=40, Wp=48, H=33, W=45), 2) != 0
        # and the plain entry points keep their labels
        p = C.c_void_p(BASE)
        assert L.ctdet_dla_base_fwd(C.byref(_base_desc()), *([p] * 12), None) == 0
        assert L.ctdet_last_kernel_label().decode() == "dla_base_fused_kernel<u8|f32 -> 32ch,f16>"
        assert L.ctdet_dla_base_x3_fwd(C.byref(_base_desc()), *([p] * 12), None) == 0
        assert L.ctdet_last_kernel_label().decode() == "dla_base_x3_kernel<u8|f32 -> 32ch,f16x3>"
    finally:
        L.ctdet_set_label_mode(0)


def test_preprocess_mirror_rejects_bad_mirror_from():
    L = _lib.lib()
    p = C.c_void_p(BASE)
    m = (C.c_float * 3)(0.4, 0.4, 0.4)
    for bad in (-1, 3):
        rc = L.ctdet_preprocess_mirror(p, _lib.U8, p, _lib.F16, 2, 33, 45, 64, 64, 3 * 33 * 45, m, m, 8, 0, bad, None)
        assert rc != 0 and b"mirror_from" in L.ctdet_last_error()


def _cfg(tmp_path, min_sizes=(), flip=True):
    from detectron2_centernet_amd.config import get_cfg
    for n in ("Base-CenterNet.yaml", "ctdet_dla_34_1x.yaml"):
        shutil.copy(os.path.join(GOLDEN, "g16_configs", n), tmp_path / n)
    cfg = get_cfg()
    cfg.merge_from_file(str(tmp_path / "ctdet_dla_34_1x.yaml"))
    cfg.MODEL.DEVICE = "cpu"
    cfg.TEST.AUG.ENABLED, cfg.TEST.AUG.MIN_SIZES, cfg.TEST.AUG.FLIP = True, tuple(min_sizes), flip
    return cfg


def test_wrapper_refusals(tmp_path):
    from detectron2_centernet_amd import modeling
    from detectron2_centernet_amd.data.catalog import register_synthetic
    from detectron2_centernet_amd.modeling import CenterNetWithTTA, build_model
    assert "CenterNetWithTTA" in modeling.__all__
    cfg = _cfg(tmp_path)
    register_synthetic(cfg.DATASETS.TRAIN[0], num_classes=80)
    model = build_model(cfg)
    # something that is not this project's CenterNet
    with pytest.raises(AssertionError, match="CenterNet"):
        CenterNetWithTTA(cfg, torch.nn.Conv2d(3, 3, 1))
    # more than one test size: multi-scale merging, named
    with pytest.raises(NotImplementedError, match="multi-scale merging"):
        CenterNetWithTTA(_cfg(tmp_path, min_sizes=(400, 500)), model)
    with pytest.raises(NotImplementedError, match="multi-scale merging"):
        CenterNetWithTTA(_cfg(tmp_path, min_sizes=(400, 500, 600, 700, 800, 900, 1000, 1100, 1200)), model)
    # one size or none are accepted; training mode is refused when called
    tta = CenterNetWithTTA(_cfg(tmp_path, min_sizes=(64,)), model)
    assert tta.flip is True and tta.resize is not None
    assert CenterNetWithTTA(_cfg(tmp_path, flip=False), model).flip is False
    model.train()
    with pytest.raises(RuntimeError, match="inference-time"):
        tta([{"image": torch.zeros(3, 64, 64, dtype=torch.uint8)}])
    with pytest.raises(RuntimeError, match="inference-time"):
        tta.forward_async([{"image": torch.zeros(3, 64, 64, dtype=torch.uint8)}])


def test_wrapper_resizes_to_the_one_test_size(tmp_path):
    from detectron2_centernet_amd.data.catalog import register_synthetic
    from detectron2_centernet_amd.modeling import CenterNetWithTTA, build_model
    cfg = _cfg(tmp_path, min_sizes=(64,))
    cfg.TEST.AUG.MAX_SIZE = 100
    register_synthetic(cfg.DATASETS.TRAIN[0], num_classes=80)
    tta = CenterNetWithTTA(cfg, build_model(cfg))
    g = torch.Generator().manual_seed(0)
    a = torch.randint(0, 256, (3, 32, 48), generator=g, dtype=torch.uint8)
    b = torch.randint(0, 256, (3, 64, 80), generator=g, dtype=torch.uint8)
    c = torch.randint(0, 256, (3, 40, 120), generator=g, dtype=torch.uint8)
    out = tta._inputs([{"image": a}, {"image": b, "height": 128, "width": 160}, {"image": c}])
    assert tuple(out[0]["image"].shape) == (3, 64, 96) and (out[0]["height"], out[0]["width"]) == (32, 48)
    assert out[1]["image"] is b and (out[1]["height"], out[1]["width"]) == (128, 160)      # already at the test size
    assert tuple(out[2]["image"].shape) == (3, 33, 100) and (out[2]["height"], out[2]["width"]) == (40, 120)   # MAX_SIZE caps
    assert out[0]["image"].dtype == torch.uint8


def test_mirrored_network_input_definition():
    """the mirror is taken on the NETWORK INPUT (normalised, zero padded right / bottom to the size divisibility): column x
    of the mirrored tensor is source column Wp-1-x, zero where that is >= W -- restated in numpy, against the oracle"""
    g = torch.Generator().manual_seed(3)
    H, W, div = 33, 45, 32
    img = torch.randint(0, 256, (3, H, W), generator=g, dtype=torch.uint8)
    mean, std = [0.408, 0.447, 0.470], [0.289, 0.274, 0.278]
    x, sizes = O.preprocess([img], mean, std, div)
    want = x.flip(3)[0].numpy()
    Hp, Wp = (H + div - 1) // div * div, (W + div - 1) // div * div
    assert x.shape == (1, 3, Hp, Wp) and (Hp, Wp) == (64, 64)
    src = img.numpy().astype(np.float32)
    m = np.asarray(mean, dtype=np.float32).reshape(3, 1, 1)
    s = np.asarray(std, dtype=np.float32).reshape(3, 1, 1)
    norm = ((src / np.float32(255.0)) - m) / s
    got = np.zeros((3, Hp, Wp), dtype=np.float32)
    for xo in range(Wp):
        xs = Wp - 1 - xo
        if xs < W:
            got[:, :H, xo] = norm[:, :, xs]
    assert np.array_equal(got, want)
    assert not got[:, :, :Wp - W].any() and got[:, :H, Wp - W:].any()      # the zero padding sits on the left
