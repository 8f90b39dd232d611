"""TEST.PRECISE_BN: population BatchNorm statistics, merged by HIP kernels (the reference takes
`get_bn_modules` / `update_bn_stats` from fvcore.nn.precise_bn).

The running statistics training leaves behind are a moving average over weights that kept changing -- and with SOLVER.EMA an
average of such averages, never measured with the weights they are shipped with.  `update_bn_stats` recomputes them from
`num_iters` fresh batches with the weights as they are: per channel the mean and the population variance over ALL rows of all
batches (of all ranks), what current fvcore's `_PopulationVarianceEstimator` gives.

fvcore runs two small torch ops per layer per batch.  Here a batch costs one statistics-only training forward at momentum 1
(`train_step.centernet_stats_forward`: every layer then leaves its batch mean and unbiased batch variance in its running
buffers) and ONE launch, `ops.precise_bn_merge_`, which folds all layers' statistics into an f64 (n, mean, M2) state through a
pointer table by Chan's parallel formula; one more launch, `ops.precise_bn_finish_`, combines the ranks' states and writes the
buffers.  There is no CPU implementation."""
import itertools

import torch

from .. import ops, ops_train
from . import train_step

__all__ = ["get_bn_modules", "update_bn_stats"]


def get_bn_modules(model):
    """the norm layers whose statistics PreciseBN recomputes: in training mode, tracking running statistics, trainable --
    the rule of `solver.ema.covered_buffers` with `m.training` added.  FrozenBatchNorm2d is no torch norm layer and never
    among them."""
    out = []
    for m in model.modules():
        if not isinstance(m, torch.nn.modules.batchnorm._NormBase) or not m.training:
            continue
        if not m.track_running_stats or m.running_mean is None:
            continue
        params = list(m.parameters(recurse=False))
        if params and not any(p.requires_grad for p in params):
            continue
        out.append(m)
    return out


def _group_of(group):
    """(rank, world, group) of the collectives: `group`, else the trainer's SyncBatchNorm group, else WORLD"""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return 0, 1, None
    g = ops_train.SYNC_BN_GROUP if group is None else group
    return dist.get_rank(g), dist.get_world_size(g), g


def _walk_rows(mods, walk):
    """the row count of every covered layer, in `mods` order, from one forward's walk [(module, rows)]"""
    seen = {}
    for m, rows in walk:
        if id(m) in seen:
            raise NotImplementedError("PreciseBN: a BatchNorm layer ran twice in one forward; its running buffers hold the "
                                      "second call's statistics only")
        seen[id(m)] = int(rows)
    missing = [i for i, m in enumerate(mods) if id(m) not in seen]
    if missing:
        raise RuntimeError(f"PreciseBN: covered BatchNorm layer {missing[0]} ({mods[missing[0]]}) was not reached by the "
                           f"statistics forward")
    return [seen[id(m)] for m in mods]


@torch.no_grad()
def update_bn_stats(model, data_loader, num_iters, group=None):
    """running_mean / running_var of every layer of `get_bn_modules(model)` := mean / population variance over the rows of
    `num_iters` batches of `data_loader` (record batches, as `model(batch)` takes them in training), over every rank of
    `group`; num_batches_tracked advances by num_iters.  Nothing else of the model changes.  If the loader ends early or
    anything raises, the statistics (and counters) are put back as they were and the error goes on; the momenta are
    restored in every case."""
    mods = get_bn_modules(model)
    if not mods:
        return
    num_iters = int(num_iters)
    if num_iters < 1:
        raise ValueError(f"PreciseBN: num_iters must be at least 1, got {num_iters}")
    dev = mods[0].running_mean.device
    if dev.type != "cuda":
        raise NotImplementedError("PreciseBN lives in HIP kernels: there is no CPU implementation of it; the model must be on "
                                  "a ROCm device")
    for m in mods:
        for b in (m.running_mean, m.running_var):
            if b.dtype != torch.float32 or not b.is_contiguous() or b.device != dev:
                raise NotImplementedError("PreciseBN: running statistics must be contiguous f32 buffers on one device")
        if m.momentum is None:
            raise NotImplementedError("PreciseBN: a layer with momentum None (cumulative average) is not supported")
    rank, world, group = _group_of(group)

    # the tables: one segment per layer, read and written where the module keeps its buffers
    numels = [m.running_mean.numel() for m in mods]
    starts = [0] + list(itertools.accumulate(numels))
    total = starts[-1]
    mean_ptrs = torch.tensor([m.running_mean.data_ptr() for m in mods], dtype=torch.int64, device=dev)
    var_ptrs = torch.tensor([m.running_var.data_ptr() for m in mods], dtype=torch.int64, device=dev)
    seg_start = torch.tensor(starts, dtype=torch.int64, device=dev)
    max_len = max(numels)
    state = torch.zeros(3, total, dtype=torch.float64, device=dev)
    # SyncBatchNorm at world > 1 leaves GLOBAL batch statistics: the row counts of those layers must be global too
    is_sync = [isinstance(m, torch.nn.SyncBatchNorm) and world > 1 for m in mods]
    sync_mask = torch.tensor(is_sync, dtype=torch.bool, device=dev) if any(is_sync) else None
    rows_cache = {}

    snapshot = [(m.running_mean.clone(), m.running_var.clone(),
                 None if m.num_batches_tracked is None else m.num_batches_tracked.clone()) for m in mods]
    momenta = [m.momentum for m in mods]
    try:
        for m in mods:
            m.momentum = 1.0
        done = 0
        for batch in itertools.islice(data_loader, num_iters):
            train_step._STATS_WALK = walk = []
            try:
                train_step.centernet_stats_forward(model, batch)
            finally:
                train_step._STATS_WALK = None
            rows = tuple(_walk_rows(mods, walk))
            rows_dev = rows_cache.get(rows)
            if rows_dev is None:
                rows_dev = rows_cache[rows] = ops.precise_bn_rows(rows).to(dev)
            if sync_mask is not None:
                import torch.distributed as dist
                summed = rows_dev.clone()
                dist.all_reduce(summed, op=dist.ReduceOp.SUM, group=group)
                rows_dev = torch.where(sync_mask, summed, rows_dev)
            ops.precise_bn_merge_(mean_ptrs, var_ptrs, seg_start, rows, max_len, state, rows_dev=rows_dev)
            done += 1
        if done < num_iters:
            raise RuntimeError(f"PreciseBN: the loader ended after {done} of {num_iters} batches")
        # this rank's state into its slot of a zeroed buffer: the SUM all-reduce is then an exact all-gather (x + 0 = x)
        slots = torch.zeros(world, 3, total, dtype=torch.float64, device=dev)
        slots[rank].copy_(state)
        if world > 1:
            import torch.distributed as dist
            dist.all_reduce(slots, op=dist.ReduceOp.SUM, group=group)
        ops.precise_bn_finish_(mean_ptrs, var_ptrs, seg_start, max_len, slots)
        for m in mods:      # raw-pointer writes: the caches keyed by tensor versions (folded BatchNorm) must see them
            torch.autograd.graph.increment_version(m.running_mean)
            torch.autograd.graph.increment_version(m.running_var)
    except BaseException:
        # a half-run must not leave one batch's momentum-1 statistics in the model
        for m, (mean, var, tracked) in zip(mods, snapshot):
            m.running_mean.copy_(mean)
            m.running_var.copy_(var)
            if tracked is not None:
                m.num_batches_tracked.copy_(tracked)
        raise
    finally:
        for m, mom in zip(mods, momenta):
            m.momentum = mom
