from .events import (CommonMetricPrinter, EventStorage, EventWriter, HistoryBuffer, JSONWriter, TensorboardXWriter,
                     get_event_storage)
from .logger import setup_logger

__all__ = ["CommonMetricPrinter", "EventStorage", "EventWriter", "HistoryBuffer", "JSONWriter", "TensorboardXWriter",
           "get_event_storage", "setup_logger"]
