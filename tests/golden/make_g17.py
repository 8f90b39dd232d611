"""G17: the SyncBN / WarmupCosineLR configs of the reference (run with the reference checkout at make_golden.REF, on the CPU).

  * g17_configs/: the reference's ctdet_res_18_bot_1x, ctdet_res_18_larger_bot_1x and ctdet_res_34_larger_bot_1x config
    files, byte for byte (their _BASE_ is G16's Base-CenterNet.yaml);
  * g17_resnet18_syncbn_state_dict_keys.txt: key and shape list of the reference's ResNet-18 built with norm="SyncBN" and
    freeze(2) (FrozenBN in stem / res2 after `convert_frozen_batchnorm`, SyncBatchNorm with num_batches_tracked in
    res3 / res4), plus CenterNet's deconv layers -- G10's format.

make_golden.py's stubbing of the reference's imports is reused unchanged."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as G  # noqa: E402


def main():
    G.install()
    load = G.load
    layers = sys.modules["detectron2.layers"]
    shape_spec = load("detectron2.layers.shape_spec")
    layers.ShapeSpec = shape_spec.ShapeSpec
    wrappers = load("detectron2.layers.wrappers")
    for n in ("Conv2d", "ConvTranspose2d", "BatchNorm2d", "cat", "interpolate", "Linear", "nonzero_tuple"):
        setattr(layers, n, getattr(wrappers, n))
    bn_mod = load("detectron2.layers.batch_norm")
    for n in ("FrozenBatchNorm2d", "get_norm", "NaiveSyncBatchNorm"):
        setattr(layers, n, getattr(bn_mod, n))
    blocks = load("detectron2.layers.blocks")
    layers.CNNBlockBase = blocks.CNNBlockBase
    deform = load("detectron2.layers.deform_conv")
    layers.ModulatedDeformConv, layers.DeformConv = deform.ModulatedDeformConv, deform.DeformConv
    layers.DeformConvV2 = deform.DeformConvV2
    st = sys.modules["detectron2.structures"]
    boxes = load("detectron2.structures.boxes")
    st.Boxes, st.BoxMode = boxes.Boxes, boxes.BoxMode
    st.Instances = load("detectron2.structures.instances").Instances
    st.ImageList = load("detectron2.structures.image_list").ImageList
    bb = sys.modules["detectron2.modeling.backbone"]
    build_mod = load("detectron2.modeling.backbone.build")
    bb.Backbone = load("detectron2.modeling.backbone.backbone").Backbone
    bb.BACKBONE_REGISTRY, bb.build_backbone = build_mod.BACKBONE_REGISTRY, build_mod.build_backbone
    dla = load("detectron2.modeling.backbone.dla")
    bb.DLAUp, bb.IDAUp = dla.DLAUp, dla.IDAUp
    load("detectron2.data.catalog")
    load("detectron2.data.detection_utils")
    sys.modules["detectron2.modeling"].postprocessing = load("detectron2.modeling.postprocessing")
    sys.modules["detectron2.modeling.meta_arch"].build = load("detectron2.modeling.meta_arch.build")
    cn = load("detectron2.modeling.meta_arch.centernet")
    resnet = load("detectron2.modeling.backbone.resnet")

    # ResNet-18 res4 with norm "SyncBN", FREEZE_AT 2 (the ctdet_res_18_bot_1x backbone), + the deconv layers
    torch.manual_seed(17)
    stem = resnet.BasicStem(in_channels=3, out_channels=64, norm="SyncBN")
    stages, cin, cout = [], 64, 64
    for idx, nblk in enumerate([2, 2, 2]):
        first_stride = 1 if idx == 0 else 2
        stages.append(resnet.ResNet.make_stage(block_class=resnet.BasicBlock, num_blocks=nblk,
                                               stride_per_block=[first_stride] + [1] * (nblk - 1), in_channels=cin,
                                               out_channels=cout, norm="SyncBN"))
        cin, cout = cout, cout * 2
    r18 = resnet.ResNet(stem, stages, out_features=["res4"]).freeze(2)
    assert isinstance(r18.res3[0].conv1.norm, torch.nn.SyncBatchNorm)
    assert type(r18.res2[0].conv1.norm).__name__ == "FrozenBatchNorm2d"
    deconv = cn.CenterNet._make_deconv_layer(None, 256, 2, [256, 256], [4, 4])
    with open(os.path.join(HERE, "g17_resnet18_syncbn_state_dict_keys.txt"), "w") as f:
        for k in sorted(r18.state_dict().keys()):
            f.write(f"backbone.{k} {tuple(r18.state_dict()[k].shape)}\n")
        for k in sorted(deconv.state_dict().keys()):
            f.write(f"deconv_layers.{k} {tuple(deconv.state_dict()[k].shape)}\n")

    cfg_src = os.path.join(G.REF, "projects", "CenterNet", "configs", "COCO-Detection")
    cfg_dst = os.path.join(HERE, "g17_configs")
    os.makedirs(cfg_dst, exist_ok=True)
    for name in ("ctdet_res_18_bot_1x.yaml", "ctdet_res_18_larger_bot_1x.yaml", "ctdet_res_34_larger_bot_1x.yaml"):
        with open(os.path.join(cfg_src, name), "rb") as fi, open(os.path.join(cfg_dst, name), "wb") as fo:
            fo.write(fi.read())
    print("G17 written to", HERE)


if __name__ == "__main__":
    main()
