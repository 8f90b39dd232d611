"""Scalar event storage and its writers (reference: detectron2/utils/events.py, with fvcore's HistoryBuffer, which is absent
here, restated small).  Scalars only: images and histograms are not kept.

What differs from the reference: `EventStorage._put_scalar_at` files a value under the iteration it BELONGS to instead of the
storage's current one.  The trainer's device-side metric ring (engine/metric_ring.py) delivers the losses of up to 64 steps at
once; written through it, the histories hold entry for entry what the reference's per-step path records."""
import datetime
import json
import logging
import os
import time
from collections import defaultdict
from contextlib import contextmanager

import numpy as np
import torch

__all__ = ["get_event_storage", "HistoryBuffer", "EventWriter", "JSONWriter", "TensorboardXWriter", "CommonMetricPrinter",
           "EventStorage"]

_CURRENT_STORAGE_STACK = []


def get_event_storage():
    """the EventStorage of the innermost `with EventStorage(...)` block"""
    assert len(_CURRENT_STORAGE_STACK), "get_event_storage() has to be called inside a 'with EventStorage(...)' context!"
    return _CURRENT_STORAGE_STACK[-1]


class HistoryBuffer:
    """(value, iteration) pairs of one scalar, the newest `max_length` of them, and the average over all of them"""

    def __init__(self, max_length=1000000):
        self._max_length = max_length
        self._data = []
        self._count = 0
        self._global_avg = 0.0

    def update(self, value, iteration=None):
        if iteration is None:
            iteration = self._count
        if len(self._data) == self._max_length:
            self._data.pop(0)
        self._data.append((value, iteration))
        self._count += 1
        self._global_avg += (value - self._global_avg) / self._count

    def latest(self):
        return self._data[-1][0]

    def median(self, window_size):
        return float(np.median([x[0] for x in self._data[-window_size:]]))

    def avg(self, window_size):
        return float(np.mean([x[0] for x in self._data[-window_size:]]))

    def global_avg(self):
        return self._global_avg

    def values(self):
        return self._data


class EventWriter:
    """takes what it wants from the current EventStorage when `write()` is called"""

    def write(self):
        raise NotImplementedError

    def close(self):
        pass


class JSONWriter(EventWriter):
    """one json object per line: for every iteration that holds a scalar's latest value not written yet, those scalars
    (median-smoothed over `window_size` where the scalar's hint says so) and "iteration", keys sorted.  Appends to the file."""

    def __init__(self, json_file, window_size=20):
        self._file_handle = open(json_file, "a")
        self._window_size = window_size
        self._last_write = -1

    def write(self):
        storage = get_event_storage()
        to_save = defaultdict(dict)
        for k, (v, itr) in storage.latest_with_smoothing_hint(self._window_size).items():
            if itr <= self._last_write:      # written before
                continue
            to_save[itr][k] = v
        if not to_save:
            return
        self._last_write = max(to_save)
        for itr, scalars in to_save.items():
            scalars["iteration"] = itr
            self._file_handle.write(json.dumps(scalars, sort_keys=True) + "\n")
        self._file_handle.flush()
        try:
            os.fsync(self._file_handle.fileno())
        except (AttributeError, OSError):
            pass

    def close(self):
        self._file_handle.close()


def tensorboard_available():
    try:
        from torch.utils.tensorboard import SummaryWriter  # noqa: F401
    except Exception:  # noqa: BLE001 -- the import fails in several ways when the tensorboard package is absent
        return False
    return True


class TensorboardXWriter(EventWriter):
    """all scalars to a tensorboard event file (needs `torch.utils.tensorboard`; scalars only)"""

    def __init__(self, log_dir, window_size=20, **kwargs):
        from torch.utils.tensorboard import SummaryWriter

        self._window_size = window_size
        self._writer = SummaryWriter(log_dir, **kwargs)
        self._last_write = -1

    def write(self):
        storage = get_event_storage()
        new_last_write = self._last_write
        for k, (v, itr) in storage.latest_with_smoothing_hint(self._window_size).items():
            if itr > self._last_write:
                self._writer.add_scalar(k, v, itr)
                new_last_write = max(new_last_write, itr)
        self._last_write = new_last_write

    def close(self):
        if hasattr(self, "_writer"):
            self._writer.close()


class CommonMetricPrinter(EventWriter):
    """the one log line of a training run: eta, iteration, every `*loss*` history's median(20), time, data_time, lr, memory"""

    def __init__(self, max_iter):
        self.logger = logging.getLogger(__name__)
        self._max_iter = max_iter
        self._last_write = None

    def write(self):
        storage = get_event_storage()
        iteration = storage.iter
        try:
            data_time = storage.history("data_time").avg(20)
        except KeyError:           # not there in the first iterations (warm-up), or without a SimpleTrainer
            data_time = None
        eta_string = None
        try:
            iter_time = storage.history("time").global_avg()
            eta_seconds = storage.history("time").median(1000) * (self._max_iter - iteration)
            storage.put_scalar("eta_seconds", eta_seconds, smoothing_hint=False)
            eta_string = str(datetime.timedelta(seconds=int(eta_seconds)))
        except KeyError:
            iter_time = None
            if self._last_write is not None:      # an estimate from the wall clock between two writes
                estimate_iter_time = (time.perf_counter() - self._last_write[1]) / (iteration - self._last_write[0])
                eta_seconds = estimate_iter_time * (self._max_iter - iteration)
                eta_string = str(datetime.timedelta(seconds=int(eta_seconds)))
            self._last_write = (iteration, time.perf_counter())
        try:
            lr = "{:.5g}".format(storage.history("lr").latest())
        except KeyError:
            lr = "N/A"
        max_mem_mb = torch.cuda.max_memory_allocated() / 1024.0 / 1024.0 if torch.cuda.is_available() else None
        self.logger.info(" {eta}iter: {iter}  {losses}  {time}{data_time}lr: {lr}  {memory}".format(
            eta=f"eta: {eta_string}  " if eta_string else "",
            iter=iteration,
            losses="  ".join(["{}: {:.4g}".format(k, v.median(20)) for k, v in storage.histories().items() if "loss" in k]),
            time="time: {:.4f}  ".format(iter_time) if iter_time is not None else "",
            data_time="data_time: {:.4f}  ".format(data_time) if data_time is not None else "",
            lr=lr,
            memory="max_mem: {:.0f}M".format(max_mem_mb) if max_mem_mb is not None else ""))


class EventStorage:
    """named scalar histories of a training run, each value filed under an iteration"""

    def __init__(self, start_iter=0):
        self._history = defaultdict(HistoryBuffer)
        self._smoothing_hints = {}
        self._latest_scalars = {}
        self._iter = start_iter
        self._current_prefix = ""

    def put_scalar(self, name, value, smoothing_hint=True):
        """smoothing_hint: whether a writer should smooth this (noisy) scalar; one hint per name"""
        self._put_scalar_at(name, value, self._iter, smoothing_hint)

    def _put_scalar_at(self, name, value, iteration, smoothing_hint=True):
        """file `value` under `iteration` (not after a later entry of the same name: a history stays in iteration order)"""
        name = self._current_prefix + name
        history = self._history[name]
        value, iteration = float(value), int(iteration)
        last = self._latest_scalars.get(name)
        assert last is None or iteration >= last[1], \
            "Scalar {} was put at iteration {} after iteration {}!".format(name, iteration, last[1])
        history.update(value, iteration)
        self._latest_scalars[name] = (value, iteration)
        existing_hint = self._smoothing_hints.get(name)
        if existing_hint is not None:
            assert existing_hint == smoothing_hint, "Scalar {} was put with a different smoothing_hint!".format(name)
        else:
            self._smoothing_hints[name] = smoothing_hint

    def put_scalars(self, *, smoothing_hint=True, **kwargs):
        for k, v in kwargs.items():
            self.put_scalar(k, v, smoothing_hint=smoothing_hint)

    def history(self, name):
        ret = self._history.get(name, None)
        if ret is None:
            raise KeyError("No history metric available for {}!".format(name))
        return ret

    def histories(self):
        return self._history

    def latest(self):
        """name -> (latest value, the iteration it was filed under)"""
        return self._latest_scalars

    def latest_with_smoothing_hint(self, window_size=20):
        """like `latest`, the value replaced by the median of the last `window_size` where the scalar's hint is True"""
        result = {}
        for k, (v, itr) in self._latest_scalars.items():
            result[k] = (self._history[k].median(window_size) if self._smoothing_hints[k] else v, itr)
        return result

    def smoothing_hints(self):
        return self._smoothing_hints

    def step(self):
        self._iter += 1

    @property
    def iter(self):
        return self._iter

    @property
    def iteration(self):
        return self._iter

    def __enter__(self):
        _CURRENT_STORAGE_STACK.append(self)
        return self

    def __exit__(self, exc_type, exc_val, exc_tb):
        assert _CURRENT_STORAGE_STACK[-1] == self
        _CURRENT_STORAGE_STACK.pop()

    @contextmanager
    def name_scope(self, name):
        """every scalar put inside the block is prefixed with `name/`"""
        old_prefix = self._current_prefix
        self._current_prefix = name.rstrip("/") + "/"
        try:
            yield
        finally:
            self._current_prefix = old_prefix
