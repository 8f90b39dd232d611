"""The common hooks of a training run (reference: detectron2/engine/hooks.py; fvcore's PeriodicCheckpointer restated).

Two things differ from the reference, both because of how SimpleTrainer works here:

  * The step's metrics wait in a device-side ring (engine/metric_ring.py) until somebody flushes them.  Every hook that
    writes, saves or scores flushes first (`trainer.flush_metrics()`): the writer so that its lines are complete, the
    checkpointer and the evaluation so that nothing is saved or scored from a state whose losses were not finite -- the
    flush is where FloatingPointError is raised, at most one flush period after the step.
  * `LRScheduler` only RECORDS the learning rate.  SimpleTrainer steps its scheduler inside the step (in a captured step the
    update kernel reads the rate from a device table the scheduler writes); a hook that stepped it again would run the
    schedule at double speed.

Not built: AutogradProfiler."""
import contextlib
import datetime
import itertools
import logging
import time

from ..evaluation.testing import flatten_results_dict
from ..utils import comm
from ..utils.events import EventStorage, EventWriter
from .precise_bn import get_bn_modules, update_bn_stats
from .train_loop import HookBase

__all__ = ["CallbackHook", "IterationTimer", "PeriodicWriter", "PeriodicCheckpointer", "LRScheduler", "EvalHook",
           "PreciseBN"]


def _flush(trainer):
    flush = getattr(trainer, "flush_metrics", None)
    if flush is not None:
        flush()


class CallbackHook(HookBase):
    """a hook made of functions that take the trainer"""

    def __init__(self, *, before_train=None, after_train=None, before_step=None, after_step=None):
        self._before_train = before_train
        self._before_step = before_step
        self._after_step = after_step
        self._after_train = after_train

    def before_train(self):
        if self._before_train:
            self._before_train(self.trainer)

    def after_train(self):
        if self._after_train:
            self._after_train(self.trainer)
        # the functions may be closures over the trainer: drop them, so that no reference cycle outlives the run
        del self._before_train, self._after_train
        del self._before_step, self._after_step

    def before_step(self):
        if self._before_step:
            self._before_step(self.trainer)

    def after_step(self):
        if self._after_step:
            self._after_step(self.trainer)


class IterationTimer(HookBase):
    """`time` per iteration, the first `warmup_iter` iterations left out, and the two summary lines at the end of training.

    With a metric ring the step time is the DEVICE time between the HIP events of two steps, filed at the flush: the steps
    are enqueued asynchronously, and a host clock around `run_step` would time the enqueue.  This hook then only tells the
    trainer from which iteration on `time` counts.  Without a ring (a trainer that reads its losses back every step) it
    times the step on the host, as the reference does.  The summary is wall-clock time either way."""

    def __init__(self, warmup_iter=3):
        self._warmup_iter = warmup_iter
        self._start_time = time.perf_counter()
        self._step_start = None
        self._total = 0.0

    def _device_timed(self):
        ring = getattr(self.trainer, "metric_ring", None)
        return ring is not None and not ring.sync_mode

    def before_train(self):
        self._start_time = time.perf_counter()
        self._total = 0.0
        if hasattr(self.trainer, "time_from_iteration"):
            self.trainer.time_from_iteration = self.trainer.start_iter + self._warmup_iter - 1

    def after_train(self):
        logger = logging.getLogger(__name__)
        total_time = time.perf_counter() - self._start_time
        total_time_minus_hooks = self._total
        hook_time = total_time - total_time_minus_hooks
        num_iter = self.trainer.iter + 1 - self.trainer.start_iter - self._warmup_iter
        if num_iter > 0 and total_time_minus_hooks > 0:
            # speed is meaningful only after the warm-up
            logger.info("Overall training speed: {} iterations in {} ({:.4f} s / it)".format(
                num_iter, str(datetime.timedelta(seconds=int(total_time_minus_hooks))), total_time_minus_hooks / num_iter))
        logger.info("Total training time: {} ({} on hooks)".format(
            str(datetime.timedelta(seconds=int(total_time))), str(datetime.timedelta(seconds=int(hook_time)))))

    def before_step(self):
        self._step_start = time.perf_counter()

    def after_step(self):
        sec = time.perf_counter() - self._step_start
        iter_done = self.trainer.iter - self.trainer.start_iter + 1      # +1: this is after_step
        if iter_done >= self._warmup_iter:
            self._total += sec
            if not self._device_timed():
                self.trainer.storage.put_scalars(time=sec)
        else:
            self._start_time = time.perf_counter()
            self._total = 0.0


class PeriodicWriter(HookBase):
    """every `period` iterations and after the last one: flush the trainer's metric ring, then `write()` of every writer"""

    def __init__(self, writers, period=20):
        self._writers = writers
        for w in writers:
            assert isinstance(w, EventWriter), w
        self._period = period

    def after_step(self):
        if (self.trainer.iter + 1) % self._period == 0 or (self.trainer.iter == self.trainer.max_iter - 1):
            _flush(self.trainer)
            for writer in self._writers:
                writer.write()

    def after_train(self):
        for writer in self._writers:
            writer.close()


class PeriodicCheckpointer(HookBase):
    """`model_{iteration:07d}.pth` whenever `iteration + 1` is a multiple of `period`, `model_final.pth` after the last
    iteration, each with `iteration` in it (fvcore's PeriodicCheckpointer as a hook).  The metric ring is flushed first: a
    non-finite loss raises there and no file is written."""

    def __init__(self, checkpointer, period, max_iter=None):
        self.checkpointer = checkpointer
        self.period = int(period)
        self.max_iter = max_iter

    def before_train(self):
        self.max_iter = self.trainer.max_iter

    def step(self, iteration, **kwargs):
        iteration = int(iteration)
        additional_state = {"iteration": iteration}
        additional_state.update(kwargs)
        periodic = self.period > 0 and (iteration + 1) % self.period == 0
        final = self.max_iter is not None and iteration >= self.max_iter - 1
        if not (periodic or final):
            return
        _flush(getattr(self, "trainer", None))
        if periodic:
            self.checkpointer.save("model_{:07d}".format(iteration), **additional_state)
        if final:
            self.checkpointer.save("model_final", **additional_state)

    def save(self, name, **kwargs):
        self.checkpointer.save(name, **kwargs)

    def after_step(self):
        self.step(self.trainer.iter)


class LRScheduler(HookBase):
    """records `lr`, the rate the iteration's update used, every iteration.  It never steps the scheduler: SimpleTrainer does
    that inside the step (see the module docstring)."""

    def __init__(self, optimizer, scheduler=None):
        self._optimizer = optimizer
        self._scheduler = scheduler      # kept for the reference's signature only
        self._lr = None

    def before_step(self):
        self._lr = self._optimizer.lr    # after the step the optimizer already holds the next iteration's rate

    def after_step(self):
        self.trainer.storage.put_scalar("lr", self._optimizer.lr if self._lr is None else self._lr, smoothing_hint=False)


class EvalHook(HookBase):
    """`eval_function()` every `eval_period` iterations and after the last one; its (nested) dict of floats goes into the
    storage flattened, unsmoothed.  Enabled on all ranks or none: it ends in a barrier."""

    def __init__(self, eval_period, eval_function):
        self._period = eval_period
        self._func = eval_function

    def _do_eval(self):
        _flush(self.trainer)           # nothing is scored from a state whose losses were not finite
        results = self._func()
        if results:
            assert isinstance(results, dict), "Eval function must return a dict. Got {} instead.".format(results)
            flattened_results = flatten_results_dict(results)
            for k, v in flattened_results.items():
                try:
                    v = float(v)
                except Exception as e:
                    raise ValueError("[EvalHook] eval_function should return a nested dict of float. "
                                     "Got '{}: {}' instead.".format(k, v)) from e
            self.trainer.storage.put_scalars(**flattened_results, smoothing_hint=False)
        comm.synchronize()             # evaluation takes the ranks different times: start the next iteration together

    def after_step(self):
        next_iter = self.trainer.iter + 1
        is_final = next_iter == self.trainer.max_iter
        if is_final or (self._period > 0 and next_iter % self._period == 0):
            self._do_eval()

    def after_train(self):
        del self._func      # likely a closure over the trainer


class PreciseBN(HookBase):
    """every `period` iterations (0: never during training) and after the last one: the running statistics of the model's
    BatchNorm layers in training mode are recomputed as the true mean and population variance over `num_iter` batches of
    `data_loader` (engine/precise_bn.py::update_bn_stats).  One iterator over the loader stays alive across runs.

    around: a callable returning a context manager that every run happens inside -- DefaultTrainer passes the EMA's
    `swapped`, so that the statistics are measured for, and stored with, the averaged weights."""

    def __init__(self, period, model, data_loader, num_iter, around=None):
        self._logger = logging.getLogger(__name__)
        if len(get_bn_modules(model)) == 0:
            self._logger.info("PreciseBN is disabled because model does not contain BN layers in training mode.")
            self._disabled = True
            return
        self._model = model
        self._data_loader = data_loader
        self._num_iter = num_iter
        self._period = period
        self._around = around
        self._disabled = False
        self._data_iter = None

    def after_step(self):
        next_iter = self.trainer.iter + 1
        is_final = next_iter == self.trainer.max_iter
        if is_final or (self._period > 0 and next_iter % self._period == 0):
            self.update_stats()

    def update_stats(self):
        """update the model with precise statistics; may be called by hand"""
        if self._disabled:
            return
        if self._data_iter is None:
            self._data_iter = iter(self._data_loader)

        def data_loader():
            for num_iter in itertools.count(1):
                if num_iter % 100 == 0:
                    self._logger.info("Running precise-BN ... {}/{} iterations.".format(num_iter, self._num_iter))
                yield next(self._data_iter)      # this way the same iterator is reused

        with EventStorage():      # events of these forwards go into a storage that is thrown away
            self._logger.info("Running precise-BN for {} iterations...  ".format(self._num_iter)
                              + "Note that this could produce different statistics every time.")
            with (self._around() if self._around is not None else contextlib.nullcontext()):
                update_bn_stats(self._model, data_loader(), self._num_iter)
