"""CPU tests of the deformable ResNet backbone (MODEL.RESNETS.DEFORM_ON_PER_STAGE) and the DCNv1 layer API: model
construction from the reference's ctdet_res_50_1x config, the state-dict layout against the reference's own deformable
ResNet-50 (tests/golden/g18_*, made by tests/golden/make_g18.py), the configurations that are refused, and the ABI's mask
mode."""
import inspect
import os
import re
import shutil

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEFORM = [False, True, True, True]


def _cfg(tmp_path, **resnets):
    from detectron2_centernet_amd.config import get_cfg

    shutil.copy(os.path.join(GOLDEN, "g16_configs", "Base-CenterNet.yaml"), tmp_path / "Base-CenterNet.yaml")
    shutil.copy(os.path.join(GOLDEN, "g16_configs", "ctdet_res_50_1x.yaml"), tmp_path / "ctdet_res_50_1x.yaml")
    cfg = get_cfg()
    cfg.merge_from_file(str(tmp_path / "ctdet_res_50_1x.yaml"))
    cfg.MODEL.DEVICE = "cpu"
    for k, v in resnets.items():
        setattr(cfg.MODEL.RESNETS, k, v)
    return cfg


def _build(cfg):
    from detectron2_centernet_amd.data.catalog import register_synthetic
    from detectron2_centernet_amd.modeling import build_model

    register_synthetic(cfg.DATASETS.TRAIN[0], num_classes=80)
    return build_model(cfg)


def _keys(model):
    sd = model.state_dict()
    return sorted(f"{k} {tuple(v.shape)}" for k, v in sd.items() if k.startswith(("backbone.", "deconv_layers.")))


def _golden_keys(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return sorted(line.strip() for line in f if line.strip())


@pytest.mark.parametrize("modulated,golden", [(False, "g18_resnet50_dconv_state_dict_keys.txt"),
                                              (True, "g18_resnet50_mdconv_state_dict_keys.txt")])
def test_deform_resnet50_builds_with_reference_layout(tmp_path, modulated, golden):
    from detectron2_centernet_amd.layers import DeformConv, ModulatedDeformConv
    from detectron2_centernet_amd.modeling.backbone.resnet import BottleneckBlock, DeformBottleneckBlock

    cfg = _cfg(tmp_path, DEFORM_ON_PER_STAGE=DEFORM, DEFORM_MODULATED=modulated)
    model = _build(cfg)
    bb = model.backbone
    assert all(type(b) is BottleneckBlock for b in bb.res2)
    for blk in (*bb.res3, *bb.res4):
        assert type(blk) is DeformBottleneckBlock
        assert type(blk.conv2) is (ModulatedDeformConv if modulated else DeformConv)
        assert blk.conv2.bias is None and blk.conv2.norm is not None
        off = blk.conv2_offset
        assert off.weight.shape == (27 if modulated else 18, blk.conv1.out_channels, 3, 3)
        assert off.bias is not None
        assert torch.count_nonzero(off.weight) == 0 and torch.count_nonzero(off.bias) == 0
    assert _keys(model) == _golden_keys(golden)


def test_deform_key_lists_differ_from_plain_r50_only_by_offsets():
    plain = set(_golden_keys("g9_resnet50_state_dict_keys.txt"))
    for name, nch in (("g18_resnet50_dconv_state_dict_keys.txt", 18), ("g18_resnet50_mdconv_state_dict_keys.txt", 27)):
        extra = set(_golden_keys(name)) - plain
        assert extra and all(re.match(r"backbone\.res[34]\.\d+\.conv2_offset\.(weight|bias) ", k) for k in extra), extra
        assert all(f"({nch}," in k for k in extra)
        assert plain - set(_golden_keys(name)) == set()


def test_r18_with_deform_raises_reference_assertion(tmp_path):
    from detectron2_centernet_amd.config import get_cfg

    cfg = _cfg(tmp_path, DEPTH=18, RES2_OUT_CHANNELS=64, DEFORM_ON_PER_STAGE=DEFORM)
    assert isinstance(cfg, type(get_cfg()))
    with pytest.raises(AssertionError, match="DEFORM_ON_PER_STAGE unsupported for R18/R34"):
        _build(cfg)


@pytest.mark.parametrize("kw,msg", [(dict(DEFORM_NUM_GROUPS=2), "DEFORM_NUM_GROUPS"),
                                    (dict(STRIDE_IN_1X1=False), "stride 2")])
def test_unsupported_deform_forms_raise(tmp_path, kw, msg):
    cfg = _cfg(tmp_path, DEFORM_ON_PER_STAGE=DEFORM, **kw)
    with pytest.raises(NotImplementedError, match=msg):
        _build(cfg)


def test_stride_in_1x1_false_without_deform_still_builds(tmp_path):
    _build(_cfg(tmp_path, STRIDE_IN_1X1=False))


def test_deform_conv_api_matches_reference():
    from detectron2_centernet_amd.layers import DeformConv, deform_conv

    params = list(inspect.signature(deform_conv).parameters)
    assert params == ["input", "offset", "weight", "stride", "padding", "dilation", "groups", "deformable_groups",
                      "im2col_step"]
    d = inspect.signature(deform_conv).parameters
    assert (d["stride"].default, d["padding"].default, d["dilation"].default, d["groups"].default,
            d["deformable_groups"].default, d["im2col_step"].default) == (1, 0, 1, 1, 1, 64)
    assert list(inspect.signature(DeformConv).parameters) == [
        "in_channels", "out_channels", "kernel_size", "stride", "padding", "dilation", "groups", "deformable_groups", "bias",
        "norm", "activation"]
    m = DeformConv(8, 16, 3, padding=1, norm=torch.nn.Identity())
    assert [k for k, _ in m.named_parameters()] == ["weight"] and m.bias is None
    assert m.weight.shape == (16, 8, 3, 3)
    with pytest.raises(AssertionError):
        DeformConv(8, 16, 3, bias=True)
    x, off = torch.randn(1, 8, 5, 5), torch.zeros(1, 18, 5, 5)
    with pytest.raises(NotImplementedError, match="Deformable Conv is not supported on CPUs!"):
        deform_conv(x, off, m.weight, 1, 1)
    with pytest.raises(NotImplementedError, match="Deformable Conv is not supported on CPUs!"):
        m(x, off)
    with pytest.raises(ValueError, match="Expected 4D tensor"):
        deform_conv(x[0], off, m.weight)


def test_mask_mode_in_header_and_bindings():
    from detectron2_centernet_amd import _lib, ops

    header = open(os.path.join(ROOT, "include", "ctdet_hip.h")).read()
    modes = dict((n, int(v)) for n, v in re.findall(r"CTDET_DCN_MASK_(\w+) = (\d+)", header))
    assert modes == {"LOGIT": 0, "PROB": 1, "NONE": 2}
    assert (_lib.DCN_MASK_LOGIT, _lib.DCN_MASK_PROB, _lib.DCN_MASK_NONE) == (0, 1, 2)
    assert ops.DCN_MASK_NONE == modes["NONE"]
    l = _lib.lib()
    assert l.ctdet_abi_version() == 8
    for name in ("ctdet_dcnv2_fwd", "ctdet_dcnv2_fwd_cols", "ctdet_dcn_cols", "ctdet_dcn_col2im_coord", "ctdet_dcn_col2im_fused"):
        assert name in _lib.SIGNATURES
    # an unknown mode is refused before any device work
    assert l.ctdet_dcn_cols(1, 64, 1, 20, 1, 1, 8, 8, 64, 3, 0, None) != 0
    assert b"mask mode 3" in l.ctdet_last_error()
