"""Test-side f64 reference of the depthwise VoVNet bodies (`V-19-slim-dw-eSE`, `V-19-dw-eSE`), written with
torch.nn.functional from a state dict whose keys are the reference module's.  Pinned to the reference's own `VoVNet` by
tests/golden/g19_vovnet19_dw.npz (tests/test_vovnet_dw_host.py); composed with the oracle's deconv layers, heads and losses
by the GPU tests.  Also: the deterministic weights of those tests (`dw_state_dict`) and the yaml of the dw configs."""
import os
import sys
import zlib

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from weights import fill_state_dict  # noqa: E402

SPECS = {
    "V-19-slim-dw-eSE": dict(stem=64, stage_ch=[64, 80, 96, 112], out_ch=[112, 256, 384, 512], layers=3, blocks=[1, 1, 1, 1]),
    "V-19-dw-eSE": dict(stem=64, stage_ch=[128, 160, 192, 224], out_ch=[256, 512, 768, 1024], layers=3, blocks=[1, 1, 1, 1]),
}

# ctdet_vovnet2_19_slim_1x.yaml with MODEL.VOVNET.CONV_BODY swapped for a depthwise body
YAML = """
_BASE_: "./Base-CenterNet.yaml"
MODEL:
  BACKBONE:
    NAME: "build_vovnet_backbone"
  WEIGHTS: "/autox-sz/users/chenxiaoniu/models/vovnet19_ese_slim_detectron2.pth"
  VOVNET:
    OUT_FEATURES: ["stage2", "stage3", "stage4", "stage5"]
    CONV_BODY: "{body}"
  CENTERNET:
    HEAD_CONV: 64
    FOCAL_LOSS_ALPHA: [1]
DATASETS:
  TRAIN: ("bulb_train",)
  TEST: ("bulb_val",)
INPUT:
  FORMAT: "RGB"
  MIN_SIZE_TRAIN: (640, 672, 704, 736, 768, 800)
SOLVER:
  IMS_PER_BATCH: 24
  BASE_LR: 2.5e-4
VERSION: 2
"""
BASE = """
MODEL:
  META_ARCHITECTURE: "CenterNet"
  PIXEL_MEAN: [0.408, 0.447, 0.470]
  PIXEL_STD: [0.289, 0.274, 0.278]
VERSION: 2
"""


def write_cfg(tmp_path, body):
    """the yaml pair in tmp_path; returns the config file's path"""
    (tmp_path / "Base-CenterNet.yaml").write_text(BASE)
    p = tmp_path / "ctdet_vovnet2_19_slim_dw_1x.yaml"
    p.write_text(YAML.format(body=body))
    return str(p)


def dw_state_dict(sd, seed):
    """weights.fill_state_dict, with the depthwise layers' FrozenBatchNorm scales (`/pw_norm.weight`, which the shared filler
    takes for a bias) drawn like the other VoVNet norm scales, from [0.75, 1.25): keeps activations at unit scale through
    the stack"""
    out = fill_state_dict(sd, seed)
    for k in out:
        if k.endswith("/pw_norm.weight"):
            g = torch.Generator().manual_seed((zlib.crc32(k.encode()) + seed + 1) % (2 ** 31))
            out[k] = (torch.rand(out[k].shape, generator=g) * 0.5 + 0.75).to(out[k].dtype)
    return out


def frozen_bn(sd, p, x, eps=1e-5):
    scale = sd[p + ".weight"] / torch.sqrt(sd[p + ".running_var"] + eps)
    shift = sd[p + ".bias"] - sd[p + ".running_mean"] * scale
    return x * scale[None, :, None, None] + shift[None, :, None, None]


def conv_norm_relu(sd, name, x, stride=1, pad=1):
    """(name/conv, name/norm, name/relu)"""
    return F.relu(frozen_bn(sd, name + "/norm", F.conv2d(x, sd[name + "/conv.weight"], None, stride, pad)))


def dw_pw(sd, name, x, stride=1):
    """(name/dw_conv3x3, name/pw_conv1x1, name/pw_norm, name/pw_relu): nothing between the two convs"""
    w = sd[name + "/dw_conv3x3.weight"]
    y = F.conv2d(x, w, None, stride, 1, 1, w.shape[0])
    y = F.conv2d(y, sd[name + "/pw_conv1x1.weight"])
    return F.relu(frozen_bn(sd, name + "/pw_norm", y))


def osa(sd, p, name, x, layers, identity):
    """one depthwise OSA module: optional 1x1 reduction, dw layers, concat of [x un-reduced, layer outputs], 1x1, eSE"""
    outs = [x]
    red = f"{p}.conv_reduction.{name}_reduction_0"
    if red + "/conv.weight" in sd:
        x = conv_norm_relu(sd, red, x, 1, 0)
    for i in range(layers):
        x = dw_pw(sd, f"{p}.layers.{i}.{name}_{i}", x)
        outs.append(x)
    xt = conv_norm_relu(sd, f"{p}.concat.{name}_concat", torch.cat(outs, 1), 1, 0)
    s = F.conv2d(xt.mean((2, 3), keepdim=True), sd[p + ".ese.fc.weight"], sd[p + ".ese.fc.bias"])
    xt = xt * (F.relu6(s + 3.0) / 6.0)
    return xt + outs[0] if identity else xt


def features(sd, x, body, p="backbone"):
    """stem (3x3 s2 conv, dw s1, dw s2) + stage2..5 -> dict of the stage outputs"""
    spec = SPECS[body]
    x = conv_norm_relu(sd, p + ".stem.stem_1", x, 2)
    x = dw_pw(sd, p + ".stem.stem_2", x, 1)
    x = dw_pw(sd, p + ".stem.stem_3", x, 2)
    outs = {}
    for si in range(4):
        stage = si + 2
        if stage != 2:
            x = F.max_pool2d(x, kernel_size=3, stride=2, ceil_mode=True)
        for bi in range(spec["blocks"][si]):
            name = f"OSA{stage}_{bi + 1}"
            x = osa(sd, f"{p}.stage{stage}.{name}", name, x, spec["layers"], identity=bi > 0)
        outs[f"stage{stage}"] = x
    return outs


def centernet_forward(sd, images_nchw, body, training=False):
    """stage4 -> the oracle's deconv layers -> the oracle's heads (centernet.py:140-154 for a VoVNet backbone)"""
    from oracle import model_ref as MR
    y = MR.deconv_layers(sd, "deconv_layers", features(sd, images_nchw, body)["stage4"], training)
    return MR.centernet_heads(MR.Net(sd), y)
