"""G18: the reference's deformable ResNet-50 (run with the reference checkout at make_golden.REF, on the CPU).

  * g18_resnet50_dconv_state_dict_keys.txt / g18_resnet50_mdconv_state_dict_keys.txt: key and shape list of the reference's
    ResNet-50 (res4, norm "FrozenBN", freeze(2): the ctdet_res_50_1x backbone) with DEFORM_ON_PER_STAGE
    [False, True, True, True] -- DeformBottleneckBlock in res3 / res4, built as build_resnet_backbone builds it
    (resnet.py:609-642) -- with DEFORM_MODULATED False (DeformConv, 18-channel conv2_offset) and True (ModulatedDeformConv,
    27 channels), plus CenterNet's deconv layers -- G10's format.

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

    for modulated, fname in ((False, "g18_resnet50_dconv_state_dict_keys.txt"), (True, "g18_resnet50_mdconv_state_dict_keys.txt")):
        torch.manual_seed(18)
        stem = resnet.BasicStem(in_channels=3, out_channels=64, norm="FrozenBN")
        stages, cin, cout, bott = [], 64, 256, 64
        for idx, (nblk, deform) in enumerate(zip([3, 4, 6], [False, True, True])):
            first_stride = 1 if idx == 0 else 2
            kw = dict(num_blocks=nblk, stride_per_block=[first_stride] + [1] * (nblk - 1), in_channels=cin, out_channels=cout,
                      norm="FrozenBN", bottleneck_channels=bott, stride_in_1x1=True, dilation=1, num_groups=1)
            if deform:
                kw.update(block_class=resnet.DeformBottleneckBlock, deform_modulated=modulated, deform_num_groups=1)
            else:
                kw.update(block_class=resnet.BottleneckBlock)
            stages.append(resnet.ResNet.make_stage(**kw))
            cin, cout, bott = cout, cout * 2, bott * 2
        r50 = resnet.ResNet(stem, stages, out_features=["res4"]).freeze(2)
        assert type(r50.res3[0]).__name__ == "DeformBottleneckBlock"
        deconv = cn.CenterNet._make_deconv_layer(None, 1024, 2, [256, 256], [4, 4])
        with open(os.path.join(HERE, fname), "w") as f:
            for k in sorted(r50.state_dict().keys()):
                f.write(f"backbone.{k} {tuple(r50.state_dict()[k].shape)}\n")
            for k in sorted(deconv.state_dict().keys()):
                f.write(f"deconv_layers.{k} {tuple(deconv.state_dict()[k].shape)}\n")
    print("G18 written to", HERE)


if __name__ == "__main__":
    main()
