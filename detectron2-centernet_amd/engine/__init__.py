from .defaults import DefaultPredictor
from .launch import launch
from .train_loop import SimpleTrainer

__all__ = ["DefaultPredictor", "SimpleTrainer", "launch"]
