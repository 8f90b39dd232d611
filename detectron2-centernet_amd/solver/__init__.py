from .build import FlatAdam, FlatSGD, adam_state_from_torch, build_optimizer, param_groups
from .lr_scheduler import (WarmupCosineLR, WarmupMultiStepLR, build_lr_scheduler, warmup_cosine_factor,
                           warmup_multistep_factor)

__all__ = ["FlatSGD", "FlatAdam", "adam_state_from_torch", "build_optimizer", "param_groups", "WarmupMultiStepLR",
           "WarmupCosineLR", "build_lr_scheduler", "warmup_multistep_factor", "warmup_cosine_factor"]
