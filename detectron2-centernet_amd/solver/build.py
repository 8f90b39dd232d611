"""SGD with momentum -- or Adam / AdamW (SOLVER.OPTIMIZER) -- over flat parameter / gradient / state buffers,
updated by the HIP kernels `sgd_runs_kernel` / `adam_runs_kernel`.

Hyper-parameter grouping follows detectron2/solver/build.py:93-137: norm-layer parameters use WEIGHT_DECAY_NORM,
`bias` parameters use BASE_LR*BIAS_LR_FACTOR and WEIGHT_DECAY_BIAS, everything else BASE_LR / WEIGHT_DECAY;
momentum SOLVER.MOMENTUM, SOLVER.NESTEROV, and SOLVER.CLIP_GRADIENTS as solver/build.py:19-90 applies it: every parameter
clipped on its own, by value or by its own 1 / 2 / inf norm, before the update.  Design for MI355X: all parameters live in ONE contiguous f32
buffer ordered by reverse registration (roughly the order backward produces gradients), so (i) ONE kernel launch updates everything (per-run
learning rate / weight decay tables in device memory), (ii) the gradient buffer is directly the RCCL all-reduce operand, cut
into large contiguous buckets (engine/reducer.py).
"""
import math

import torch

from .. import _lib, ops

NORM_TYPES = (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d, torch.nn.BatchNorm3d, torch.nn.SyncBatchNorm,
              torch.nn.GroupNorm, torch.nn.InstanceNorm2d, torch.nn.LayerNorm, torch.nn.LocalResponseNorm)


def param_groups(cfg, model):
    """[(param, lr_factor, weight_decay)] in module order (solver/build.py:100-131)."""
    out, memo = [], set()
    for module in model.modules():
        for key, value in module.named_parameters(recurse=False):
            if not value.requires_grad or value in memo:
                continue
            memo.add(value)
            lr_factor, wd = 1.0, cfg.SOLVER.WEIGHT_DECAY
            if isinstance(module, NORM_TYPES):
                wd = cfg.SOLVER.WEIGHT_DECAY_NORM
            elif key == "bias":
                lr_factor = cfg.SOLVER.BIAS_LR_FACTOR
                wd = cfg.SOLVER.WEIGHT_DECAY_BIAS
            out.append((value, float(lr_factor), float(wd)))
    return out


GRAD_CHUNK = 4096     # elements per partial of the per-parameter norms (16 KB: one float4 per thread and trip, four trips)
_NORM_KINDS = {1.0: _lib.NORM_L1, 2.0: _lib.NORM_L2, math.inf: _lib.NORM_INF}


def grad_chunks(offsets, chunk=GRAD_CHUNK):
    """The chunk table of the per-parameter norm reduction, a pure function of `offsets` = [(start, numel)] (consecutive
    parameters of the flat buffer): chunks of at most `chunk` elements, in buffer order, none across a parameter boundary.
    Returns (chunk_start, chunk_len, param_chunk_end): parameter q owns chunks [param_chunk_end[q-1], param_chunk_end[q])."""
    starts, lens, ends = [], [], []
    for off, n in offsets:
        for a in range(off, off + n, chunk):
            starts.append(a)
            lens.append(min(chunk, off + n - a))
        ends.append(len(starts))
    return starts, lens, ends


def clip_from_cfg(cfg):
    """SOLVER.CLIP_GRADIENTS -> None (disabled) or (clip type, CLIP_VALUE, NORM_TYPE) as FlatSGD(clip=...) takes it"""
    c = cfg.SOLVER.get("CLIP_GRADIENTS", None)
    if c is None or not c.get("ENABLED", False):
        return None
    return (c.CLIP_TYPE, c.CLIP_VALUE, c.get("NORM_TYPE", 2.0))


def _check_clip(clip):
    """(clip type, value[, norm type]) -> (_lib.CLIP_*, value, _lib.NORM_* or 0), refusing what is not built"""
    if clip is None:
        return _lib.CLIP_NONE, 0.0, 0
    kind, value = clip[0], float(clip[1])
    if kind not in ("value", "norm"):      # the reference: GradientClipType(cfg.CLIP_TYPE) raises ValueError
        raise ValueError(f"SOLVER.CLIP_GRADIENTS.CLIP_TYPE: {kind!r} is not a valid gradient clip type ('value', 'norm')")
    if not value > 0.0:
        raise ValueError(f"SOLVER.CLIP_GRADIENTS.CLIP_VALUE must be positive, got {value}")
    if kind == "value":
        return _lib.CLIP_VALUE, value, 0
    try:
        norm = _NORM_KINDS[float(clip[2]) if len(clip) > 2 else 2.0]
    except (KeyError, TypeError, ValueError):
        raise NotImplementedError(f"SOLVER.CLIP_GRADIENTS.NORM_TYPE {clip[2]!r}: the norm kernels are built for 1, 2 and "
                                  "inf") from None
    return _lib.CLIP_NORM, value, norm


class FlatOptimizer:
    """What the flat optimizers share: the parameters re-pointed into ONE f32 buffer in reverse registration order, the
    gradient buffer next to it, the runs of equal (lr factor, weight decay) with their device tables, the learning-rate table
    the schedulers write, the chunk tables and results of per-parameter norm clipping, the zero arena of the weight-gradient
    accumulators and the plan that re-packs the conv weights after a step.  A subclass adds its state buffers and the update."""

    def __init__(self, groups, base_lr, device=None, clip=None, needs_hip=None):
        """groups: [(param, lr_factor, weight_decay)].  Parameters are re-pointed into one flat buffer.
        clip: None, ("value", c) or ("norm", c, p) with p in 1, 2, inf -- each parameter clipped on its own (clip_from_cfg).
        needs_hip: the refusal for parameters that are not on a ROCm device (None: they are accepted); raised before any
        parameter is touched"""
        self.base_lr = float(base_lr)
        self._clip_type, self._clip_value, self._norm_type = _check_clip(clip)
        groups = list(groups)
        if needs_hip and groups and torch.device(device or groups[0][0].device).type != "cuda":
            raise NotImplementedError(needs_hip)
        groups = list(reversed(groups))  # heads first: the order gradients become ready in backward
        # contiguous segments per (lr_factor, wd) would break the backward-order layout; instead keep the order and
        # record maximal runs of equal hyper-parameters (a handful for DLA-34: weights / norm+bias alternate per layer
        # type, so runs are merged by sorting *within* a bucket-sized window only if adjacent).  Simplest exact form:
        # one run per change of (lr_factor, wd).
        self.params = [g[0] for g in groups]
        device = device or self.params[0].device
        total = sum(p.numel() for p in self.params)
        self.flat_param = torch.empty(total, dtype=torch.float32, device=device)
        self.flat_grad = torch.zeros(total, dtype=torch.float32, device=device)
        self.offsets, self.runs = [], []
        off = 0
        for p, lf, wd in groups:
            n = p.numel()
            self.flat_param[off:off + n].copy_(p.data.reshape(-1))
            p.data = self.flat_param[off:off + n].view_as(p.data)
            p.grad = self.flat_grad[off:off + n].view_as(p.data)
            p._ctdet_flat_grad = p.grad      # ops_train.grad_slot: backward kernels accumulate here directly
            if self.runs and self.runs[-1][2] == lf and self.runs[-1][3] == wd:
                self.runs[-1][1] = off + n
            else:
                self.runs.append([off, off + n, lf, wd])
            self.offsets.append((off, n))
            off += n
        self.lr_factors = sorted({r[2] for r in self.runs})
        # device-side tables for the one-launch update: run ends, weight decay, index into the lr table
        self._lr_table = torch.zeros(len(self.lr_factors), dtype=torch.float32, device=device)
        # (norm clipping: one run per parameter, so that the kernel's run lookup also finds the parameter's clip coefficient)
        table = self.runs
        if self._clip_type == _lib.CLIP_NORM:
            table = [[off, off + n, lf, wd] for (off, n), (_, lf, wd) in zip(self.offsets, groups)]
        self._run_end = torch.tensor([r[1] for r in table], dtype=torch.int64, device=device)
        self._run_wd = torch.tensor([r[3] for r in table], dtype=torch.float32, device=device)
        self._run_lr_index = torch.tensor([self.lr_factors.index(r[2]) for r in table], dtype=torch.int32, device=device)
        # per-parameter norm clipping: the chunk table of the norm reduction, and where its results live.
        # `grad_norms` / `clip_coefs` (one entry per parameter, in the order of `self.params`) hold the last step's values;
        # reading them is the caller's synchronisation, step() never waits for them
        self.grad_norms = self.clip_coefs = None
        if self._clip_type == _lib.CLIP_NORM:
            starts, lens, ends = grad_chunks(self.offsets)
            self._chunk_start = torch.tensor(starts, dtype=torch.int64, device=device)
            self._chunk_len = torch.tensor(lens, dtype=torch.int32, device=device)
            self._param_chunk_end = torch.tensor(ends, dtype=torch.int32, device=device)
            self._partials = torch.zeros(len(starts), dtype=torch.float32, device=device)
            self.grad_norms = torch.zeros(len(self.params), dtype=torch.float32, device=device)
            self.clip_coefs = torch.ones(len(self.params), dtype=torch.float32, device=device)
        self.set_lr_factor(1.0)
        # zero-initialised scratch for the atomically accumulated weight gradients (ops_train.ZeroArena): a little larger
        # than the parameter count (channel padding), cleared together with the gradient buffer
        self._arena = self._packs = None
        self.ema = None       # a solver.ema.ModelEMA, attached by its owner: updated behind every step (_after_update)
        if torch.device(device).type == "cuda":
            from .. import ops_train
            self._arena = ops_train.ARENA = ops_train.ZeroArena(int(total * 1.25) + (1 << 20), torch.device(device))
            self._packs = ops.PACK_PLAN = ops.PackPlan(self.flat_param)

    def set_lr_factor(self, f):
        self._sched_factor = float(f)
        for i, lf in enumerate(self.lr_factors):
            self._lr_table[i:i + 1].fill_(self.base_lr * lf * self._sched_factor)

    @property
    def lr(self):
        return self.base_lr * self._sched_factor

    def zero_grad(self):
        self.flat_grad.zero_()
        if self._arena is not None:       # the weight-gradient accumulators of this backward pass: one fill for all of them
            from .. import ops_train
            ops_train.PENDING.clear()     # leftovers of a backward pass that raised ...
            ops_train._END_QUEUED[0] = False   # ... whose end-of-backward callback autograd dropped with it: without this
                                               # reset no later pass would queue the flush of its weight gradients again
            self._arena.begin_step()
        for p, (off, n) in zip(self.params, self.offsets):
            if p.grad is None or p.grad.data_ptr() != self.flat_grad.data_ptr() + 4 * off:
                p.grad = p._ctdet_flat_grad = self.flat_grad[off:off + n].view_as(p.data)

    def _clip_coef_launches(self):
        """norm clipping: the two launches of the per-parameter norms and coefficients, in front of the update"""
        if self._clip_type == _lib.CLIP_NORM:
            ops.grad_chunk_norms_(self.flat_grad, self._chunk_start, self._chunk_len, self._norm_type, self._partials)
            ops.grad_clip_coefs_(self._partials, self._param_chunk_end, self._norm_type, self._clip_value,
                                 self.grad_norms, self.clip_coefs)

    def _after_update(self):
        if self.ema is not None:      # SOLVER.EMA: launches only, so inside the captured single-GPU step
            self.ema.update()
        for p in self.params:  # raw-pointer update: tell autograd / the packed-weight caches the values changed
            torch.autograd.graph.increment_version(p)
        if self._packs is not None:   # the f16 operands of every conv weight the last step used, in one launch
            self._packs.run()


class FlatSGD(FlatOptimizer):
    def __init__(self, groups, base_lr, momentum=0.9, device=None, nesterov=False, clip=None):
        """groups, clip: see FlatOptimizer"""
        self.momentum, self.nesterov = float(momentum), bool(nesterov)
        needs_hip = None
        if self.nesterov or (clip is not None and _check_clip(clip)[0] != _lib.CLIP_NONE):
            needs_hip = ("SOLVER.NESTEROV / SOLVER.CLIP_GRADIENTS live in the HIP update kernel: there is no CPU "
                         "implementation of them; the model's parameters must be on a ROCm device")
        super().__init__(groups, base_lr, device, clip, needs_hip)
        self.flat_mom = torch.zeros_like(self.flat_param)
        self._first = True

    def step(self):
        """launches only (the step is captured into the training graph): the plain update is one kernel; Nesterov and value
        clipping are variants of it; norm clipping puts the two kernels of the per-parameter norms in front.  `flat_grad` is
        read, never written: it keeps what backward (and the all-reduce) produced"""
        if self._clip_type == _lib.CLIP_NONE and not self.nesterov:
            ops.sgd_momentum_runs_(self.flat_param, self.flat_grad, self.flat_mom, self._run_end, self._run_lr_index,
                                   self._run_wd, self._lr_table, self.momentum, self._first)
        else:
            self._clip_coef_launches()
            ops.sgd_momentum_runs_clip_(self.flat_param, self.flat_grad, self.flat_mom, self._run_end, self._run_lr_index,
                                        self._run_wd, self._lr_table, self.momentum, self._first, self.nesterov,
                                        self._clip_type, self._clip_value, self.clip_coefs)
        self._first = False
        self._after_update()

    def state_dict(self):
        return {"momentum": self.flat_mom.clone(), "first": self._first}

    def load_state_dict(self, sd):
        """this optimizer's own state, or the `torch.optim.SGD` state dict a reference checkpoint carries under "optimizer"
        ({"state": {index: {"momentum_buffer": t}}, "param_groups": [{"params": [indices], ...}]}): the reference builds one
        group per parameter in module order (solver/build.py:100-137), the order of `param_groups` here, so buffer i
        belongs to parameter i of that order"""
        if "momentum" in sd:
            self.flat_mom.copy_(sd["momentum"])
            self._first = sd["first"]
            return
        if "state" not in sd or "param_groups" not in sd:
            raise KeyError("optimizer state: neither FlatSGD's {'momentum', 'first'} nor a torch.optim.SGD state dict")
        if any("exp_avg" in st for st in sd["state"].values()):
            raise KeyError("optimizer state: FlatSGD expects 'momentum_buffer' entries (torch.optim.SGD), this one holds "
                           "'exp_avg' (torch.optim.Adam / AdamW: SOLVER.OPTIMIZER)")
        order = [i for g in sd["param_groups"] for i in g["params"]]
        if len(order) != len(self.params):
            raise ValueError(f"optimizer state holds {len(order)} parameters, the model has {len(self.params)} trainable ones")
        # self.params is the reversed module order
        loaded = 0
        for k, idx in enumerate(order):
            st = sd["state"].get(idx, {})
            buf = st.get("momentum_buffer")
            off, n = self.offsets[len(order) - 1 - k]
            if buf is None:
                self.flat_mom[off:off + n].zero_()
                continue
            if buf.numel() != n:
                raise ValueError(f"momentum buffer {idx}: {buf.numel()} elements, parameter has {n}")
            self.flat_mom[off:off + n].copy_(buf.reshape(-1).to(self.flat_mom.device, torch.float32))
            loaded += 1
        self._first = loaded == 0


def adam_state_from_torch(sd, numels, amsgrad=False):
    """A `torch.optim.Adam` / `AdamW` state dict ({"state": {i: {"step", "exp_avg", "exp_avg_sq"[, "max_exp_avg_sq"]}},
    "param_groups": [{"params": [indices], ...}]}, one group per parameter in module order, as FlatSGD.load_state_dict assumes
    for SGD) -> FlatAdam's own {"exp_avg", "exp_avg_sq", ["max_exp_avg_sq"], "step"}: flat f32 CPU buffers in the order of
    `numels`, the element counts of FlatAdam's parameters -- the REVERSED module order.  A pure function (no device).
    `step` (an int or a tensor) must be the same for every parameter that has a state, since the flat step keeps one count;
    a parameter without a state (torch creates it at the parameter's first gradient) gets zeros."""
    if "state" not in sd or "param_groups" not in sd:
        raise KeyError("optimizer state: neither FlatAdam's {'exp_avg', 'exp_avg_sq', 'step'} nor a torch.optim.Adam / AdamW "
                       "state dict")
    order = [i for g in sd["param_groups"] for i in g["params"]]
    numels = list(numels)
    if len(order) != len(numels):
        raise ValueError(f"optimizer state holds {len(order)} parameters, the model has {len(numels)} trainable ones")
    names = ["exp_avg", "exp_avg_sq"] + (["max_exp_avg_sq"] if amsgrad else [])
    pieces, steps = {k: [] for k in names}, set()
    for k in reversed(range(len(order))):           # module index k sits at position len - 1 - k of the flat buffer
        st, n = sd["state"].get(order[k], {}), numels[len(order) - 1 - k]
        if st:
            missing = [key for key in names + ["step"] if key not in st]
            if missing:
                raise KeyError(f"optimizer state of parameter {order[k]}: FlatAdam expects {names + ['step']} "
                               f"(torch.optim.Adam / AdamW{', amsgrad=True' if amsgrad else ''}), {missing} missing; it holds "
                               f"{sorted(st)}")
            steps.add(int(st["step"]))
        for key in names:
            buf = st.get(key) if st else None
            if buf is None:
                buf = torch.zeros(n)
            if buf.numel() != n:
                raise ValueError(f"{key} {order[k]}: {buf.numel()} elements, parameter has {n}")
            pieces[key].append(buf.detach().reshape(-1).to("cpu", torch.float32))
    if len(steps) > 1:
        raise ValueError(f"optimizer state: per-parameter step counts {sorted(steps)}; the flat Adam step keeps one count for "
                         "all parameters")
    out = {key: torch.cat(v) if v else torch.zeros(0) for key, v in pieces.items()}
    out["step"] = steps.pop() if steps else 0
    return out


def _check_adam(betas, eps):
    """torch.optim.Adam's own refusals, in its words"""
    betas = tuple(float(b) for b in betas)
    if len(betas) != 2:
        raise ValueError(f"SOLVER.ADAM.BETAS must hold two values, got {betas}")
    if not float(eps) > 0.0:           # torch's words; torch lets eps == 0 through, the entry point does not
        raise ValueError(f"Invalid epsilon value: {eps}")
    for i, b in enumerate(betas):
        if not 0.0 <= b < 1.0:
            raise ValueError(f"Invalid beta parameter at index {i}: {b}")
    return betas, float(eps)


class FlatAdam(FlatOptimizer):
    """torch.optim.Adam (decoupled=False: weight decay added to the gradient) / AdamW (decoupled=True: p *= 1 - lr * wd),
    optionally AMSGrad, single-tensor order, over the flat buffers: `exp_avg`, `exp_avg_sq`, `max_exp_avg_sq` (None without
    amsgrad) and ONE step count for all parameters, `step_count`, which lives on the device -- the single-GPU training graph
    replays step() without the host, so the kernels advance it.  A parameter whose gradient is zero is still
    stepped (weight decay, decaying moments): the flat buffer has no "grad is None", as in FlatSGD.  SOLVER.MOMENTUM is not
    read.  There is no CPU implementation."""

    def __init__(self, groups, base_lr, betas=(0.9, 0.999), eps=1e-8, decoupled=False, amsgrad=False, clip=None, device=None):
        """groups, clip: see FlatOptimizer"""
        self.betas, self.eps = _check_adam(betas, eps)
        self.decoupled, self.amsgrad = bool(decoupled), bool(amsgrad)
        super().__init__(groups, base_lr, device, clip,
                         needs_hip="SOLVER.OPTIMIZER ADAM / ADAMW live in the HIP update kernel: there is no CPU implementation "
                                   "of them; the model's parameters must be on a ROCm device")
        self.exp_avg = self.flat_mom = torch.zeros_like(self.flat_param)     # flat_mom: the name engine/bench_train.py reads
        self.exp_avg_sq = torch.zeros_like(self.flat_param)
        self.max_exp_avg_sq = torch.zeros_like(self.flat_param) if self.amsgrad else None
        self.step_count = torch.zeros(1, dtype=torch.int64, device=self.flat_param.device)
        self._bias = torch.ones(2, dtype=torch.float32, device=self.flat_param.device)   # written by every step's first launch

    def step(self):
        """launches only: the step count and bias corrections (one thread), [the two kernels of the per-parameter norms],
        the update.  `flat_grad` is read, never written"""
        ops.adam_advance_(self.step_count, self._bias, *self.betas)
        self._clip_coef_launches()
        ops.adam_runs_(self.flat_param, self.flat_grad, self.exp_avg, self.exp_avg_sq, self.max_exp_avg_sq, self._run_end,
                       self._run_lr_index, self._run_wd, self._lr_table, self._bias, self.betas[0], self.betas[1], self.eps,
                       self.decoupled, self.amsgrad, self._clip_type, self._clip_value, self.clip_coefs)
        self._after_update()

    def _state_names(self):
        return ["exp_avg", "exp_avg_sq"] + (["max_exp_avg_sq"] if self.amsgrad else [])

    def state_dict(self):
        """reading the step count waits for the device"""
        sd = {k: getattr(self, k).clone() for k in self._state_names()}
        sd["step"] = int(self.step_count.item())
        return sd

    def load_state_dict(self, sd):
        """this optimizer's own state, or a `torch.optim.Adam` / `AdamW` state dict (adam_state_from_torch)"""
        if "momentum" in sd or any("momentum_buffer" in st for st in sd.get("state", {}).values()):
            raise KeyError(f"optimizer state: FlatAdam expects {self._state_names() + ['step']} or a torch.optim.Adam / AdamW "
                           "state dict, this one is an SGD state (momentum)")
        if "exp_avg" not in sd:
            sd = adam_state_from_torch(sd, [n for _, n in self.offsets], self.amsgrad)
        missing = [k for k in self._state_names() + ["step"] if k not in sd]
        if missing:
            raise KeyError(f"optimizer state: FlatAdam expects {self._state_names() + ['step']}, {missing} missing")
        for k in self._state_names():
            getattr(self, k).copy_(sd[k])
        self.step_count.fill_(int(sd["step"]))


OPTIMIZERS = ("SGD", "ADAM", "ADAMW")


def build_optimizer(cfg, model):
    """solver/build.py:93-137: torch.optim.SGD(momentum, nesterov) behind maybe_add_gradient_clipping; with SOLVER.OPTIMIZER
    ADAM / ADAMW (keys the reference does not have) torch.optim.Adam / AdamW(SOLVER.ADAM.BETAS, EPS, AMSGRAD) behind the same
    clipping.  What the kernels do not implement is refused instead of being silently dropped: a NORM_TYPE other than 1, 2,
    inf, either SGD option or Adam for parameters that are not on a ROCm device, and NESTEROV with Adam (SOLVER.MOMENTUM is
    simply not read there: beta1 takes its place)."""
    name = cfg.SOLVER.get("OPTIMIZER", "SGD")
    if name not in OPTIMIZERS:
        raise ValueError(f"SOLVER.OPTIMIZER: {name!r} is not one of {', '.join(OPTIMIZERS)}")
    if name == "SGD":
        return FlatSGD(param_groups(cfg, model), cfg.SOLVER.BASE_LR, cfg.SOLVER.MOMENTUM,
                       nesterov=cfg.SOLVER.get("NESTEROV", False), clip=clip_from_cfg(cfg))
    if cfg.SOLVER.get("NESTEROV", False):
        raise ValueError(f"SOLVER.NESTEROV: True has no meaning for SOLVER.OPTIMIZER: {name} (Nesterov momentum is an option "
                         "of SGD)")
    adam = cfg.SOLVER.ADAM
    return FlatAdam(param_groups(cfg, model), cfg.SOLVER.BASE_LR, betas=adam.BETAS, eps=adam.EPS, decoupled=name == "ADAMW",
                    amsgrad=adam.AMSGRAD, clip=clip_from_cfg(cfg))


def build_model_ema(cfg, model, optimizer):
    """SOLVER.EMA -> a ModelEMA over `optimizer`'s flat buffer (solver/ema.py), or None when it is disabled.  The caller
    attaches it (`optimizer.ema = ema`) and registers it with the checkpointer"""
    e = cfg.SOLVER.get("EMA", None)
    if e is None or not e.get("ENABLED", False):
        return None
    from .ema import ModelEMA
    return ModelEMA(model, optimizer, decay=e.DECAY, warmup=e.WARMUP)
