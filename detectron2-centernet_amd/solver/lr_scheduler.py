"""WarmupMultiStepLR and WarmupCosineLR (detectron2/solver/lr_scheduler.py:16-87, warm-up factor :90-116) and the choice
between them by SOLVER.LR_SCHEDULER_NAME (detectron2/solver/build.py:140-165)."""
import math
from bisect import bisect_right


def _warmup_factor(it, warmup_factor, warmup_iters, warmup_method):
    if it >= warmup_iters:
        w = 1.0
    elif warmup_method == "constant":
        w = warmup_factor
    elif warmup_method == "linear":
        alpha = it / warmup_iters
        w = warmup_factor * (1 - alpha) + alpha
    else:
        raise ValueError(f"Unknown warmup method: {warmup_method}")
    return w


def warmup_multistep_factor(it, milestones, gamma, warmup_factor, warmup_iters, warmup_method="linear"):
    return _warmup_factor(it, warmup_factor, warmup_iters, warmup_method) * gamma ** bisect_right(list(milestones), it)


def warmup_cosine_factor(it, max_iters, warmup_factor, warmup_iters, warmup_method="linear"):
    """the half cosine over [0, max_iters] multiplied by the warm-up factor (lr_scheduler.py:71-84)"""
    return _warmup_factor(it, warmup_factor, warmup_iters, warmup_method) * 0.5 * (1.0 + math.cos(math.pi * it / max_iters))


class WarmupMultiStepLR:
    """scheduler over a flat optimizer (FlatSGD / FlatAdam): `step()` advances one iteration and writes the new learning rates."""

    def __init__(self, optimizer, milestones, gamma=0.1, warmup_factor=0.001, warmup_iters=1000, warmup_method="linear",
                 last_epoch=-1):
        if not list(milestones) == sorted(milestones):
            raise ValueError(f"Milestones should be a list of increasing integers. Got {milestones}")
        self.optimizer, self.milestones, self.gamma = optimizer, list(milestones), gamma
        self.warmup_factor, self.warmup_iters, self.warmup_method = warmup_factor, warmup_iters, warmup_method
        self.last_epoch = last_epoch
        self.step()

    def get_factor(self):
        return warmup_multistep_factor(self.last_epoch, self.milestones, self.gamma, self.warmup_factor,
                                       self.warmup_iters, self.warmup_method)

    def step(self):
        self.last_epoch += 1
        self.optimizer.set_lr_factor(self.get_factor())

    def state_dict(self):
        return {"last_epoch": self.last_epoch}

    def load_state_dict(self, sd):
        self.last_epoch = sd["last_epoch"]
        self.optimizer.set_lr_factor(self.get_factor())


class WarmupCosineLR(WarmupMultiStepLR):
    """lr_scheduler.py:52-87 over a flat optimizer (MAX_ITER iterations)"""

    def __init__(self, optimizer, max_iters, warmup_factor=0.001, warmup_iters=1000, warmup_method="linear", last_epoch=-1):
        self.optimizer, self.max_iters = optimizer, max_iters
        self.warmup_factor, self.warmup_iters, self.warmup_method = warmup_factor, warmup_iters, warmup_method
        self.last_epoch = last_epoch
        self.step()

    def get_factor(self):
        return warmup_cosine_factor(self.last_epoch, self.max_iters, self.warmup_factor, self.warmup_iters, self.warmup_method)


def build_lr_scheduler(cfg, optimizer):
    """solver/build.py:140-165"""
    name = cfg.SOLVER.LR_SCHEDULER_NAME
    if name == "WarmupMultiStepLR":
        return WarmupMultiStepLR(optimizer, cfg.SOLVER.STEPS, cfg.SOLVER.GAMMA, warmup_factor=cfg.SOLVER.WARMUP_FACTOR,
                                 warmup_iters=cfg.SOLVER.WARMUP_ITERS, warmup_method=cfg.SOLVER.WARMUP_METHOD)
    if name == "WarmupCosineLR":
        return WarmupCosineLR(optimizer, cfg.SOLVER.MAX_ITER, warmup_factor=cfg.SOLVER.WARMUP_FACTOR,
                              warmup_iters=cfg.SOLVER.WARMUP_ITERS, warmup_method=cfg.SOLVER.WARMUP_METHOD)
    raise ValueError(f"Unknown LR scheduler: {name}")
