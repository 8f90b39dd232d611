"""G19: the reference's depthwise VoVNet-19 bodies (run with the reference checkout at make_golden.REF, on the CPU).

  * g19_vovnet19_dw.npz: an odd-sized input (2 x 3 x 70 x 100: the ceil-mode stage pooling matters) and the stage2..5 outputs
    of the reference's own `VoVNet` for CONV_BODY "V-19-slim-dw-eSE" (keys slim_stage2 ..) and "V-19-dw-eSE" (dw_stage2 ..),
    NORM "FrozenBN", FREEZE_AT 0, weights from tests/vovnet_dw_ref.dw_state_dict (weights.fill_state_dict, depthwise norm
    scales drawn like the other norm scales) with seeds 191 / 192.
  * g19_vovnet19_slim_dw_state_dict_keys.txt / g19_vovnet19_dw_state_dict_keys.txt: key and shape list of each body --
    G12's format.

make_golden.py's stubbing of the reference's imports is reused unchanged."""
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as G  # noqa: E402
from vovnet_dw_ref import dw_state_dict  # noqa: E402

BODIES = (("V-19-slim-dw-eSE", "slim", "g19_vovnet19_slim_dw_state_dict_keys.txt", 191),
          ("V-19-dw-eSE", "dw", "g19_vovnet19_dw_state_dict_keys.txt", 192))


def main():
    G.install()
    load = G.load
    layers = sys.modules["detectron2.layers"]
    layers.ShapeSpec = load("detectron2.layers.shape_spec").ShapeSpec
    wrappers = load("detectron2.layers.wrappers")
    for n in ("Conv2d", "ConvTranspose2d", "BatchNorm2d", "cat", "interpolate", "Linear", "nonzero_tuple"):
        setattr(layers, n, getattr(wrappers, n))
    bn_mod = load("detectron2.layers.batch_norm")
    for n in ("FrozenBatchNorm2d", "get_norm", "NaiveSyncBatchNorm"):
        setattr(layers, n, getattr(bn_mod, n))
    bb = sys.modules["detectron2.modeling.backbone"]
    build_mod = load("detectron2.modeling.backbone.build")
    bb.Backbone = load("detectron2.modeling.backbone.backbone").Backbone
    bb.BACKBONE_REGISTRY, bb.build_backbone = build_mod.BACKBONE_REGISTRY, build_mod.build_backbone
    vov = load("detectron2.modeling.backbone.vovnet")

    gg = torch.Generator().manual_seed(1900)
    x = torch.randn(2, 3, 70, 100, generator=gg)
    arrays = {"x": x.numpy()}
    for body, tag, fname, seed in BODIES:
        cfg = NS(MODEL=NS(VOVNET=NS(NORM="FrozenBN", CONV_BODY=body), BACKBONE=NS(FREEZE_AT=0)))
        torch.manual_seed(seed)
        net = vov.VoVNet(cfg, 3, out_features=["stage2", "stage3", "stage4", "stage5"]).eval()
        sd = net.state_dict()
        net.load_state_dict(dw_state_dict({k: v for k, v in sd.items()}, seed=seed))
        with torch.no_grad():
            outs = net(x)
        for k, v in outs.items():
            arrays[f"{tag}_{k}"] = v.numpy()
        with open(os.path.join(HERE, fname), "w") as f:
            for k in sorted(sd.keys()):
                f.write(f"backbone.{k} {tuple(sd[k].shape)}\n")
    np.savez_compressed(os.path.join(HERE, "g19_vovnet19_dw.npz"), **arrays)
    print("G19 written to", HERE)


if __name__ == "__main__":
    main()
