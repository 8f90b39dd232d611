from .shape_spec import ShapeSpec
from .deform_conv import DCN, DeformConv, DeformConvV2, ModulatedDeformConv, deform_conv, modulated_deform_conv
from .batch_norm import Conv2d, FrozenBatchNorm2d, get_norm
from . import hipnn

__all__ = ["ShapeSpec", "DCN", "DeformConv", "DeformConvV2", "ModulatedDeformConv", "deform_conv", "modulated_deform_conv",
           "hipnn", "Conv2d",
           "FrozenBatchNorm2d", "get_norm"]
