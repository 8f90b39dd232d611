"""SOLVER.EMA: an exponential moving average of the weights, kept and swapped in by HIP kernels.

    e <- e + w * (p - e),   w = 1 - d,   d = min(DECAY, (1 + t) / (10 + t)) under WARMUP, else DECAY

over every trainable parameter -- ONE flat f32 buffer next to the optimizer's `flat_param` -- and over the running statistics
of the norm layers that training writes.  `update()` is three launches behind the optimizer update, inside the captured
single-GPU step; the update count t lives on the device, as Adam's step count does.  For an evaluation the averaged values
are EXCHANGED with the live ones in place (`swapped()`): the captured graphs hold the addresses of `flat_param`, of the
BatchNorm buffers and of the packed conv operands, so nothing may be re-pointed.  There is no CPU implementation of the
update; the naming table and the state dict (`EmaTable`) are plain torch and work anywhere."""
import contextlib

import torch

from .. import ops

STAT_ALIGN = 4      # elements: every statistics segment starts on a float4 boundary of `ema_stats`


def check_decay(decay):
    decay = float(decay)
    if not 0.0 <= decay < 1.0:
        raise ValueError(f"SOLVER.EMA.DECAY must lie in [0, 1), got {decay}")
    return decay


def ema_decay(t, decay, warmup):
    """the decay of update number t (0-based), as ctdet_ema_advance computes it in f64"""
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


def covered_buffers(model):
    """[(state-dict name, buffer)]: running_mean / running_var of the norm layers that track running statistics and are
    trainable.  FrozenBatchNorm2d (not a torch norm layer), a norm layer whose parameters are all frozen, pixel_mean /
    pixel_std never change and are left out; num_batches_tracked is an integer and stays live."""
    out = []
    for mname, m in model.named_modules():
        if not isinstance(m, torch.nn.modules.batchnorm._NormBase) or not m.track_running_stats or m.running_mean is None:
            continue
        params = list(m.parameters(recurse=False))
        if params and not any(p.requires_grad for p in params):
            continue
        for key in ("running_mean", "running_var"):
            out.append((f"{mname}.{key}" if mname else key, getattr(m, key)))
    return out


def stat_layout(numels):
    """offsets of the statistics segments in `ema_stats`, each padded to STAT_ALIGN elements -> (starts, total)"""
    starts, off = [], 0
    for n in numels:
        starts.append(off)
        off += -(-n // STAT_ALIGN) * STAT_ALIGN
    return starts, off


class EmaTable:
    """Which slice of the flat EMA buffers belongs to which state-dict name, and the state dict built from it."""

    def __init__(self, model, params, offsets):
        """params / offsets: the optimizer's parameters and their [(start, numel)] in its flat buffer"""
        names = {id(p): n for n, p in model.named_parameters()}
        unnamed = [i for i, p in enumerate(params) if id(p) not in names]
        if unnamed:
            raise ValueError(f"ModelEMA: optimizer parameters {unnamed} do not belong to the model")
        self.params = [(names[id(p)], off, n, tuple(p.shape)) for p, (off, n) in zip(params, offsets)]
        self.buffers_live = covered_buffers(model)
        starts, self.stats_total = stat_layout([b.numel() for _, b in self.buffers_live])
        self.buffers = [(name, off, b.numel(), tuple(b.shape)) for (name, b), off in zip(self.buffers_live, starts)]

    def pack(self, flat_param, flat_stats, updates, decay):
        def part(flat, entries):
            return {name: flat[off:off + n].detach().to("cpu", torch.float32).reshape(shape).clone()
                    for name, off, n, shape in entries}
        return {"params": part(flat_param, self.params), "buffers": part(flat_stats, self.buffers), "updates": int(updates),
                "decay": float(decay)}

    def unpack(self, sd, flat_param, flat_stats):
        """writes sd's tensors into the flat buffers by name; a missing or mis-shaped entry raises and names it.  Everything
        is checked before anything is written.  Returns the update count."""
        for kind, entries in (("params", self.params), ("buffers", self.buffers)):
            have = sd.get(kind, {})
            for name, _, _, shape in entries:
                if name not in have:
                    raise KeyError(f"EMA state: '{name}' is missing from its \"{kind}\"")
                if tuple(have[name].shape) != shape:
                    raise ValueError(f"EMA state: '{name}' has shape {tuple(have[name].shape)}, the model's is {shape}")
        if "updates" not in sd:
            raise KeyError("EMA state: 'updates' is missing")
        for kind, entries, flat in (("params", self.params, flat_param), ("buffers", self.buffers, flat_stats)):
            for name, off, n, _ in entries:
                flat[off:off + n].copy_(sd[kind][name].reshape(-1).to(flat.device, torch.float32))
        return int(sd["updates"])


class ModelEMA:
    def __init__(self, model, optimizer, decay=0.9998, warmup=True):
        """optimizer: a FlatOptimizer over `model`'s parameters.  The EMA starts as a copy of the live values with an update
        count of 0.  The caller attaches it (`optimizer.ema = ema`): FlatOptimizer._after_update then runs `update()`."""
        self.decay, self.warmup = check_decay(decay), bool(warmup)
        dev = optimizer.flat_param.device
        if dev.type != "cuda":
            raise NotImplementedError("SOLVER.EMA lives in HIP kernels: there is no CPU implementation of it; the model's "
                                      "parameters must be on a ROCm device")
        self.model, self.optimizer = model, optimizer
        self.table = EmaTable(model, optimizer.params, optimizer.offsets)
        self.updates = torch.zeros(1, dtype=torch.int64, device=dev)
        self.weight = torch.zeros(1, dtype=torch.float32, device=dev)      # written by every update's first launch
        # the parameters: one segment, many workgroups
        total = optimizer.flat_param.numel()
        self.ema_param = optimizer.flat_param.clone()
        self._param_ptrs = torch.tensor([optimizer.flat_param.data_ptr()], dtype=torch.int64, device=dev)
        self._param_start = torch.tensor([0, total], dtype=torch.int64, device=dev)
        # the statistics: one segment per buffer, read where the module keeps it.  A segment's length is the distance to the
        # next start, so the padding behind a buffer whose length is no multiple of STAT_ALIGN is a segment of its own, paired
        # with scratch
        self.ema_stats = torch.zeros(self.table.stats_total, dtype=torch.float32, device=dev)
        self._scratch = torch.zeros_like(self.ema_stats)
        ptrs, starts = [], []
        for (_, b), (_, off, n, _) in zip(self.table.buffers_live, self.table.buffers):
            if b.dtype != torch.float32 or not b.is_contiguous() or b.device != dev:
                raise NotImplementedError("ModelEMA: running statistics must be contiguous f32 buffers on the optimizer's device")
            ptrs.append(b.data_ptr())
            starts.append(off)
            if n % STAT_ALIGN:
                ptrs.append(self._scratch.data_ptr() + 4 * (off + n))
                starts.append(off + n)
        self._stat_max = max([b.numel() for _, b in self.table.buffers_live], default=0)
        self._stat_ptrs = torch.tensor(ptrs, dtype=torch.int64, device=dev)
        self._stat_start = torch.tensor(starts + [self.table.stats_total], dtype=torch.int64, device=dev)
        self._gather_stats()

    def _gather_stats(self):
        for (_, b), (_, off, n, _) in zip(self.table.buffers_live, self.table.buffers):
            self.ema_stats[off:off + n].copy_(b.detach().reshape(-1))

    def update(self):
        """launches only (the step is captured into the training graph): the count and the weight (one thread), the
        parameters, the statistics"""
        ops.ema_advance_(self.updates, self.weight, self.decay, self.warmup)
        ops.ema_lerp_segments_(self._param_ptrs, self.ema_param, self._param_start, self.ema_param.numel(), self.weight)
        if self._stat_max:
            ops.ema_lerp_segments_(self._stat_ptrs, self.ema_stats, self._stat_start, self._stat_max, self.weight)

    def reset(self):
        """EMA := live, updates := 0"""
        self.ema_param.copy_(self.optimizer.flat_param)
        self._gather_stats()
        self.updates.zero_()

    def _exchange(self):
        ops.ema_swap_segments_(self._param_ptrs, self.ema_param, self._param_start, self.ema_param.numel())
        if self._stat_max:
            ops.ema_swap_segments_(self._stat_ptrs, self.ema_stats, self._stat_start, self._stat_max)
        # raw-pointer writes: tell autograd and the caches keyed by tensor versions (folded BatchNorm, packed weights) ...
        for p in self.optimizer.params:
            torch.autograd.graph.increment_version(p)
        for _, b in self.table.buffers_live:
            torch.autograd.graph.increment_version(b)
        # ... and refresh the packed f16 / f16x3 operands the captured training step reads: they are not keyed by anything
        # the graph looks at.  After the exchange back this is what keeps the next step from training on EMA operands.
        if getattr(self.optimizer, "_packs", None) is not None:
            self.optimizer._packs.run()

    @contextlib.contextmanager
    def swapped(self):
        """`with ema.swapped(): evaluate(model)` -- the model holds the averaged weights and statistics inside the block (the
        EMA buffers hold the live ones meanwhile) and the live ones again after it, bit for bit, also when the block raises"""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ModelEMA.swapped() inside a stream capture: the exchange belongs to no training graph")
        self._exchange()
        try:
            yield self
        finally:
            self._exchange()

    def state_dict(self):
        """{"params": {name: f32 CPU tensor}, "buffers": {...}, "updates": int, "decay": float}, keyed by the model's
        state-dict names; reading the count waits for the device"""
        return self.table.pack(self.ema_param, self.ema_stats, self.updates.item(), self.decay)

    def load_state_dict(self, sd):
        """by name; `decay` stays what this object was built with (the config's)"""
        self.updates.fill_(self.table.unpack(sd, self.ema_param, self.ema_stats))

    def model_state_dict(self):
        """the model's full state dict with the EMA values substituted: what one ships"""
        out = {k: v.detach().cpu().clone() for k, v in self.model.state_dict().items()}
        sd = self.state_dict()
        out.update(sd["params"])
        out.update(sd["buffers"])
        return out

    @staticmethod
    def load_into_model(model, sd):
        """a checkpoint's "ema" entry into a plain model, for evaluation: its parameters and statistics replace the model's;
        a name the model does not have, or another shape, raises"""
        values = dict(sd["params"])
        values.update(sd["buffers"])
        own = model.state_dict()
        for name, v in values.items():
            if name not in own:
                raise KeyError(f"EMA state: the model has no '{name}'")
            if tuple(own[name].shape) != tuple(v.shape):
                raise ValueError(f"EMA state: '{name}' has shape {tuple(v.shape)}, the model's is {tuple(own[name].shape)}")
        model.load_state_dict(values, strict=False)
        return model
