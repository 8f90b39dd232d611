"""CPU tests of the depthwise VoVNet-19 bodies (`V-19-slim-dw-eSE`, `V-19-dw-eSE`): construction from the VoVNet config with
CONV_BODY swapped, the state-dict layout against the reference's own modules (tests/golden/g19_*, made by
tests/golden/make_g19.py), the test-side f64 reference (tests/vovnet_dw_ref.py) against the reference's stage outputs, and
the depthwise 3x3 entry points' argument checks."""
import os

import numpy as np
import pytest
import torch

import vovnet_dw_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BODIES = [("V-19-slim-dw-eSE", "slim", "g19_vovnet19_slim_dw_state_dict_keys.txt", 191, 384),
          ("V-19-dw-eSE", "dw", "g19_vovnet19_dw_state_dict_keys.txt", 192, 768)]


def _build(tmp_path, body):
    from detectron2_centernet_amd.config import get_cfg
    from detectron2_centernet_amd.data.catalog import register_synthetic
    from detectron2_centernet_amd.modeling import build_model

    cfg = get_cfg()
    cfg.merge_from_file(R.write_cfg(tmp_path, body))
    cfg.MODEL.DEVICE = "cpu"
    register_synthetic("bulb_train", num_classes=80)
    return build_model(cfg)


def _golden_keys(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return sorted(line.strip() for line in f if line.strip())


@pytest.mark.parametrize("body,tag,keys,seed,stage4", BODIES)
def test_dw_vovnet_builds_with_reference_layout(tmp_path, body, tag, keys, seed, stage4):
    from detectron2_centernet_amd.modeling.backbone.vovnet import _OSA_module

    model = _build(tmp_path, body)
    assert model.backbone_type == "vovnet"
    sd = model.state_dict()
    got = sorted(f"{k} {tuple(v.shape)}" for k, v in sd.items() if k.startswith("backbone."))
    assert got == _golden_keys(keys)
    # the deconv layers read stage4
    assert model.backbone.output_shape()["stage4"].channels == stage4
    assert sd["deconv_layers.0.weight"].shape[0] == stage4
    # module names and order of the reference (dw conv, pw conv, pw norm, pw relu; reduction before the layers)
    names = [n for n, _ in model.backbone.stem.named_children()]
    assert names == ["stem_1/conv", "stem_1/norm", "stem_1/relu", "stem_2/dw_conv3x3", "stem_2/pw_conv1x1", "stem_2/pw_norm",
                     "stem_2/pw_relu", "stem_3/dw_conv3x3", "stem_3/pw_conv1x1", "stem_3/pw_norm", "stem_3/pw_relu"]
    assert getattr(model.backbone.stem, "stem_3/dw_conv3x3").stride == (2, 2)
    osa = model.backbone.stage3.OSA3_1
    assert isinstance(osa, _OSA_module) and osa.depthwise and osa.isReduced
    assert [n for n, _ in osa.named_children()][:2] == ["conv_reduction", "layers"]
    dw = getattr(osa.layers[0], "OSA3_1_0/dw_conv3x3")
    assert dw.groups == dw.in_channels == dw.out_channels and dw.bias is None
    # FREEZE_AT 2 of the config: stem and stage2 frozen, the rest trainable
    frozen = {n for n, p in model.named_parameters() if not p.requires_grad}
    assert any(n.startswith("backbone.stem.stem_2/dw") for n in frozen)
    assert not any(n.startswith("backbone.stage3") and "dw_conv3x3" in n for n in frozen)


@pytest.mark.parametrize("body,tag,keys,seed,stage4", BODIES)
def test_f64_helper_matches_reference_module(body, tag, keys, seed, stage4):
    """the test-side f64 reference of the dw backbone reproduces the reference module's stage outputs (G19) from the same
    weights: max |delta| / max |ref| <= 1e-5 per stage"""
    g = np.load(os.path.join(GOLDEN, "g19_vovnet19_dw.npz"))
    shapes = {}
    for line in open(os.path.join(GOLDEN, keys)):
        k, shp = line.strip().split(" ", 1)
        shapes[k] = eval(shp)
    # make_g19 filled the module's own state dict, whose keys carry no "backbone." prefix (the weights are keyed by name)
    sd = R.dw_state_dict({k[len("backbone."):]: torch.zeros(s) for k, s in shapes.items()}, seed=seed)
    sd = {"backbone." + k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        outs = R.features(sd, torch.from_numpy(g["x"]).double(), body)
    for s in ("stage2", "stage3", "stage4", "stage5"):
        ref = torch.from_numpy(g[f"{tag}_{s}"]).double()
        assert outs[s].shape == ref.shape, (s, outs[s].shape, ref.shape)
        assert ref.abs().max() > 0.1 and ref.std() > 1e-2      # a live signal, not a collapsed map
        err = ((outs[s] - ref).abs().max() / ref.abs().max()).item()
        assert err <= 1e-5, (body, s, err)


def test_dwconv_abi_declared_and_validates_arguments():
    from detectron2_centernet_amd import _lib

    header = open(os.path.join(ROOT, "include", "ctdet_hip.h")).read()
    for name in ("ctdet_dwconv3x3_fwd", "ctdet_dwconv3x3_wgrad", "ctdet_dwconv3x3_wgrad_workspace_bytes"):
        assert name + "(" in header and name in _lib.SIGNATURES
    l = _lib.lib()
    assert l.ctdet_abi_version() == 8
    F16, F32 = _lib.F16, _lib.F32
    p = 1 << 20           # any 16-byte-aligned address: every call below must be refused before it is used
    # stride outside {1, 2}
    assert l.ctdet_dwconv3x3_fwd(p, 64, p, p, 64, 1, 8, 8, 64, 3, 0, F32, None) != 0
    assert b"stride 3" in l.ctdet_last_error()
    # channels not a multiple of the vector width (4 for f32, 8 for f16)
    assert l.ctdet_dwconv3x3_fwd(p, 68, p, p, 68, 1, 8, 8, 66, 1, 0, F32, None) != 0
    assert b"multiple of 4" in l.ctdet_last_error()
    assert l.ctdet_dwconv3x3_fwd(p, 68, p, p, 68, 1, 8, 8, 68, 1, 0, F16, None) != 0
    assert b"multiple of 8" in l.ctdet_last_error()
    # a pixel stride that is narrower than C or breaks the vector alignment
    assert l.ctdet_dwconv3x3_fwd(p, 60, p, p, 64, 1, 8, 8, 64, 1, 0, F32, None) != 0
    assert b"pixel stride 60" in l.ctdet_last_error()
    # misaligned pointer
    assert l.ctdet_dwconv3x3_fwd(p + 4, 64, p, p, 64, 1, 8, 8, 64, 1, 0, F32, None) != 0
    assert b"aligned" in l.ctdet_last_error()
    # null pointers
    assert l.ctdet_dwconv3x3_fwd(None, 64, p, p, 64, 1, 8, 8, 64, 1, 0, F32, None) != 0
    assert b"null" in l.ctdet_last_error()
    assert l.ctdet_dwconv3x3_wgrad(p, 64, None, 64, p, p, 1.0, 0, 1, 8, 8, 64, 1, F32, None) != 0
    assert b"null" in l.ctdet_last_error()
    assert l.ctdet_dwconv3x3_wgrad(p, 64, p, 64, None, p, 1.0, 0, 1, 8, 8, 64, 1, F32, None) != 0
    assert b"workspace" in l.ctdet_last_error()
    # the stride-2 backward is not built: refused with a message
    assert l.ctdet_dwconv3x3_wgrad(p, 64, p, 64, p, p, 1.0, 0, 1, 8, 8, 64, 2, F32, None) != 0
    assert b"stride 2" in l.ctdet_last_error()
    assert l.ctdet_dwconv3x3_wgrad(p, 64, p, 64, p, p, 1.0, 0, 1, 8, 8, 64, 3, F16, None) != 0
    assert b"stride 3" in l.ctdet_last_error()
    # workspace: one f32 [9][C] slot per workgroup, at least one for a non-empty problem, at most 1024
    ws = l.ctdet_dwconv3x3_wgrad_workspace_bytes(2, 33, 47, 96, F32)
    assert ws > 0 and ws % (9 * 96 * 4) == 0
    assert l.ctdet_dwconv3x3_wgrad_workspace_bytes(64, 256, 256, 64, F16) == 1024 * 9 * 64 * 4
    assert l.ctdet_dwconv3x3_wgrad_workspace_bytes(1, 8, 8, 66, F32) == 0


def test_dwconv_ops_refuse_cpu_tensors():
    import detectron2_centernet_amd.ops as ops
    from detectron2_centernet_amd import ops_train

    x = torch.zeros(1, 8, 8, 64)
    w = torch.zeros(64, 1, 3, 3)
    with pytest.raises(NotImplementedError):
        ops.dwconv3x3(x, w, 1)
    with pytest.raises(NotImplementedError):
        ops_train.dwconv3x3_wgrad(x, x)
    with pytest.raises(NotImplementedError):
        ops_train.DwConv3x3Fn.apply(x, w, 1)
