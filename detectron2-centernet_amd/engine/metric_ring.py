"""Per-step training metrics that never stall the step.

The reference's `SimpleTrainer._write_metrics` (train_loop.py:261-290) reads every loss back with `.cpu().item()` and gathers
the dicts of all ranks by pickle, on every step.  Here one tiny HIP launch behind each step (ops_train.metric_push) copies
the step's loss scalars, its data time and its iteration number into a row of a 64-row ring on the device, and keeps the
first iteration whose losses were not finite in one device word.  `flush()` -- called by whatever needs the numbers: the
periodic writer, the checkpoint hook, the evaluation hook -- fetches ring and word in ONE device-to-host copy behind ONE
synchronisation (and, with several ranks, one all-gather in front of it), checks the rows' tags, reduces over the ranks and
returns one record per iteration.  `records_from_rows` is that reduction, a pure function over host arrays.

Step time: one HIP event per step, recorded behind the push; an iteration's `time` is the device time between its event and
the one before it (a host clock around an asynchronous enqueue would measure the launch).  The first step after a flush is
measured from an event `begin_step` records, so the host work of the hook that flushed is not billed to it.

CTDET_METRICS_SYNC=1 (read at construction): the reference's per-step path instead -- read back, gather and check in `push`."""
import os
from collections import OrderedDict

import numpy as np
import torch

from .. import ops_train
from ..utils import comm

RING_ROWS = 64
MAX_SCALARS = ops_train.METRIC_MAX_SCALARS
ROW_FLOATS = MAX_SCALARS + 2
NO_BAD_ITERATION = ops_train.METRIC_NO_BAD_ITERATION
NON_FINITE_MESSAGE = "Loss became infinite or NaN at iteration={}!\nloss_dict = {}"


def records_from_rows(names, rows, iterations):
    """The rank reduction of a flush, on host arrays.

    names: the K loss names, in the order of the step's loss dict.  rows: f32 [world, n, >= K + 2], row j of every rank being
    the ring row of iterations[j]: [tag (int32 bits), K losses, data_time, ...].  Returns n records
    {"iteration", "data_time", "total_loss", "losses": OrderedDict}: the losses averaged over the ranks (in float64, as
    np.mean over the ranks' Python floats is), data_time the maximum over the ranks, total_loss the sum of the averaged losses
    in dict order (train_loop.py:279-290).  A row whose tag is not the expected iteration -- overwritten, never written, out
    of order -- raises RuntimeError."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    K = len(names)
    if rows.ndim != 3 or rows.shape[1] != len(iterations) or rows.shape[2] < K + 2:
        raise ValueError(f"rows {rows.shape} do not hold {len(iterations)} rows of {K} losses per rank")
    tags = rows[:, :, 0].view(np.int32)
    want = np.asarray(list(iterations), dtype=np.int64).reshape(1, -1)
    if rows.shape[1] and not np.array_equal(tags, np.broadcast_to(want, tags.shape)):
        r, j = [int(v[0]) for v in np.nonzero(tags != want)]
        raise RuntimeError(f"metric ring: rank {r} holds tag {int(tags[r, j])} where iteration {int(want[0, j])} was expected "
                           "(a row that was overwritten, never written or pushed out of order)")
    losses = rows[:, :, 1:1 + K].astype(np.float64)
    data_time = rows[:, :, 1 + K].astype(np.float64)
    records = []
    for j, it in enumerate(iterations):
        mean = OrderedDict((k, np.mean([losses[r, j, i] for r in range(rows.shape[0])])) for i, k in enumerate(names))
        records.append({"iteration": int(it), "data_time": float(np.max(data_time[:, j])),
                        "total_loss": float(sum(v for v in mean.values())),
                        "losses": OrderedDict((k, float(v)) for k, v in mean.items())})
    return records


def first_bad_iteration(words):
    """the smallest first-bad word of the ranks, or None while every rank's word is still the sentinel"""
    first = int(np.min(np.asarray(words, dtype=np.int64)))
    return None if first >= NO_BAD_ITERATION else first


def put_records(storage, records, time_from_iteration=None):
    """file the records of a flush in `storage`, each under the iteration it belongs to, in the reference's order: data_time,
    total_loss, the losses (when there is more than one), then the step time.  time_from_iteration: the first iteration
    whose `time` is kept (IterationTimer's warm-up rule); None keeps no time."""
    for rec in records:
        it = rec["iteration"]
        storage._put_scalar_at("data_time", rec["data_time"], it)
        storage._put_scalar_at("total_loss", rec["total_loss"], it)
        if len(rec["losses"]) > 1:
            for k, v in rec["losses"].items():
                storage._put_scalar_at(k, v, it)
        if rec.get("time") is not None and time_from_iteration is not None and it >= time_from_iteration:
            storage._put_scalar_at("time", rec["time"], it)


class MetricRing:
    """push(loss_dict, data_time, iteration) behind every step; flush() -> the records of the iterations pushed since"""

    def __init__(self, device, process_group=None):
        device = torch.device(device)
        if device.type != "cuda":
            raise NotImplementedError("the CenterNet HIP path has no CPU implementation; the metric ring lives on a ROCm device")
        self.device, self.group = device, process_group
        self.sync_mode = os.environ.get("CTDET_METRICS_SYNC", "0") == "1"
        # ring and first-bad word in one buffer, so that one copy fetches both: rows [0, RING_ROWS) the ring, every tag -1;
        # row RING_ROWS starts with the word
        buf = torch.full((RING_ROWS + 1, ROW_FLOATS), -1, dtype=torch.int32, device=device)
        buf[RING_ROWS, 0] = NO_BAD_ITERATION
        self._buf = buf.view(torch.float32)
        self.ring = self._buf[:RING_ROWS]
        self.first_bad = buf[RING_ROWS, :1]
        self._host = None
        # one event more than rows: a pending step's `before` event is the event of the push before it, which may be one
        # push older than the oldest unread row; with RING_ROWS + 1 events, taken in turn, it is re-recorded only by a push
        # that has flushed that step first (at most RING_ROWS steps are ever pending)
        self._events = [torch.cuda.Event(enable_timing=True) for _ in range(RING_ROWS + 1)]
        self._pushes = 0
        self._start = torch.cuda.Event(enable_timing=True)
        self._prev = None
        self._pending = []            # (iteration, event before the step or None, event behind it) of the rows not read yet
        self._backlog = []            # records of a flush that `push` had to make itself
        self.names = None
        self.flushes = 0

    @property
    def world(self):
        import torch.distributed as dist
        return dist.get_world_size(self.group) if dist.is_available() and dist.is_initialized() else 1

    def begin_step(self):
        """in front of a step: the event the step's time is measured from, when the step before it left none (the first
        step, and the first one after a flush)"""
        if self.sync_mode:          # every step ends in a read-back: IterationTimer's host clock measures the step
            return
        if self._prev is None:
            self._start.record()
            self._prev = self._start

    def push(self, loss_dict, data_time, iteration):
        names = tuple(loss_dict.keys())
        if self.names is None:
            if not 1 <= len(names) <= MAX_SCALARS:
                raise ValueError(f"the metric ring holds 1..{MAX_SCALARS} losses per step, got {len(names)}")
            self.names = names
        elif names != self.names:
            raise ValueError(f"the loss dict changed from {self.names} to {names}")
        scalars = [v.detach() for v in loss_dict.values()]
        if any(not t.is_cuda for t in scalars):
            raise NotImplementedError("the CenterNet HIP path has no CPU implementation; tensors must be on a ROCm device")
        if self.sync_mode:
            return self._push_sync(scalars, data_time, iteration)
        if len(self._pending) >= RING_ROWS:       # the row about to be written is still unread
            self._backlog.extend(self._fetch())
        scalars = [t if t.dtype == torch.float32 else t.float() for t in scalars]
        ops_train.metric_push(scalars, data_time, self.ring, self.first_bad, iteration)
        ev = self._events[self._pushes % (RING_ROWS + 1)]
        self._pushes += 1
        ev.record()
        self._pending.append((int(iteration), self._prev, ev))
        self._prev = ev

    def _push_sync(self, scalars, data_time, iteration):
        """the reference's step: a read-back per loss, the check, a gather of the dicts (train_loop.py:253-290)"""
        metrics = OrderedDict((k, t.cpu().item()) for k, t in zip(self.names, scalars))
        if not all(np.isfinite(v) for v in metrics.values()):
            raise FloatingPointError(NON_FINITE_MESSAGE.format(iteration, dict(metrics)))
        metrics["data_time"] = float(data_time)
        every = comm.gather(metrics)
        if not comm.is_main_process():
            return
        dt = float(np.max([m.pop("data_time") for m in every]))
        mean = OrderedDict((k, np.mean([m[k] for m in every])) for k in self.names)
        self._backlog.append({"iteration": int(iteration), "data_time": dt, "total_loss": float(sum(v for v in mean.values())),
                              "losses": OrderedDict((k, float(v)) for k, v in mean.items()), "time": None})

    def flush(self):
        """the records of every iteration pushed since the last flush, oldest first; FloatingPointError when a loss of one of
        them was not finite (the message names the first such iteration and carries its loss dict)"""
        records, self._backlog = self._backlog, []
        if self._pending:
            records.extend(self._fetch())
        self._prev = None       # whoever flushed does host work now: the next step is timed from its own `begin_step`
        return records

    def _fetch(self):
        import torch.distributed as dist
        world = self.world
        src = self._buf
        if world > 1:        # ONE collective per flush (the reference: one pickle gather per step)
            src = torch.empty((world,) + tuple(self._buf.shape), dtype=torch.float32, device=self.device)
            dist.all_gather(list(src.unbind(0)), self._buf, group=self.group)
        if self._host is None or self._host.shape != src.shape:
            self._host = torch.empty(src.shape, dtype=torch.float32, pin_memory=True)
        self._host.copy_(src, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        self.flushes += 1
        host = self._host.numpy().reshape(world, RING_ROWS + 1, ROW_FLOATS)
        pending, self._pending = self._pending, []
        iterations = [p[0] for p in pending]
        rows = host[:, [it % RING_ROWS for it in iterations], :]
        bad = first_bad_iteration(host[:, RING_ROWS, 0].view(np.int32))
        if bad is not None:
            words = host[:, RING_ROWS, 0].view(np.int32)
            r = int(np.argmin(words))
            row = host[r, bad % RING_ROWS]
            tagged = int(row[:1].view(np.int32)[0]) == bad
            loss = {k: float(row[1 + i]) for i, k in enumerate(self.names)} if tagged else "(the row is gone)"
            raise FloatingPointError(NON_FINITE_MESSAGE.format(bad, loss))
        records = records_from_rows(self.names, rows, iterations)
        for rec, (_, before, after) in zip(records, pending):
            rec["time"] = before.elapsed_time(after) * 1e-3 if before is not None else None
        return records
