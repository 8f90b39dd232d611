from . import hooks
from .defaults import DefaultPredictor, DefaultTrainer, default_argument_parser, default_setup
from .hooks import CallbackHook, EvalHook, IterationTimer, LRScheduler, PeriodicCheckpointer, PeriodicWriter, PreciseBN
from .launch import launch
from .metric_ring import MetricRing
from .train_loop import HookBase, SimpleTrainer, TrainerBase

__all__ = ["DefaultPredictor", "DefaultTrainer", "default_argument_parser", "default_setup", "SimpleTrainer", "TrainerBase",
           "HookBase", "MetricRing", "hooks", "CallbackHook", "EvalHook", "IterationTimer", "LRScheduler",
           "PeriodicCheckpointer", "PeriodicWriter", "PreciseBN", "launch"]
