from .build import FlatAdam, FlatSGD, adam_state_from_torch, build_model_ema, build_optimizer, param_groups
from .ema import ModelEMA
from .lr_scheduler import (WarmupCosineLR, WarmupMultiStepLR, build_lr_scheduler, warmup_cosine_factor,
                           warmup_multistep_factor)

__all__ = ["FlatSGD", "FlatAdam", "adam_state_from_torch", "build_optimizer", "build_model_ema", "ModelEMA", "param_groups",
           "WarmupMultiStepLR",
           "WarmupCosineLR", "build_lr_scheduler", "warmup_multistep_factor", "warmup_cosine_factor"]
