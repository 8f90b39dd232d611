"""Case tables, float64 reference and error bound of the flat optimizer-step kernels (csrc/train_ops.hip): sgd_kernel,
sgd_runs_kernel, sgd_runs_clip_kernel<CLIP, NEST>, adam_runs_kernel<CLIP, DECOUPLED, AMSGRAD>, adam_advance_kernel,
grad_chunk_norm_kernel<L1|L2|INF> and grad_clip_coef_kernel<L1|L2|INF>.

The reference is the definition -- the comment blocks above sgd_runs_body and adam_runs_kernel, which are torch's order --
evaluated in a float64 "value with running error bound" (EV): every operation returns the float64 result r and a bound e(r)
on the error of the same operation chain evaluated in f32, u = 2^-24:

    a +- b        e(a) + e(b) + u |r|
    a * b         |a| e(b) + |b| e(a) + e(a) e(b) + u |r|
    a / b         (e(a) + |r| e(b)) / (|b| - e(b)) + u |r|        (|b| > e(b) is asserted)
    sqrt(a)       sqrt(a + e(a)) - sqrt(max(a - e(a), 0)) + u |r|
    maximum       max(e(a), e(b))
    clamp, select, copy: the operand's own bound

The tolerance of an element is 2 e + 2^-149: the factor 2 covers the second-order terms and the one rounding a fused
multiply-add saves (train_ops.hip is built with contraction on, torch's CPU path and numpy are not).  u |r| bounds a
rounding only in the normal range, so every float64 intermediate is asserted to be zero or normal in f32.

The same formulas run in a second arithmetic, F32 (numpy float32, one rounding per operation, nothing fused): the host
test holds that emulation, and torch.optim on the CPU, to the tolerance, and a list of seeded wrong formulas (WRONG) outside
it.  Hyper-parameters reach the formulas per element, np.repeat over the run table -- independent of the kernel's binary
search, so a neighbour run's lr or weight decay leaking across a boundary shows.

Sums (the norm kernels) use the depth of the kernel's fixed summation shape instead: an element that passes through at
most D additions contributes at most D u times the sum of the magnitudes of the terms."""
import math

import numpy as np

U = 2.0 ** -24
F32_MIN_NORMAL = 2.0 ** -126
F32_DENORM = 2.0 ** -149

CLIP_NONE, CLIP_VALUE, CLIP_NORM = 0, 1, 2          # _lib.CLIP_* (the host test asserts they agree)
NORM_L1, NORM_L2, NORM_INF = 1, 2, 3                # _lib.NORM_*
GUARD = 64                                          # sentinel elements on either side of every buffer
SENTINEL = 777.0


def f32(x):
    """x rounded to f32, as a Python float (what `(float)x` gives the launchers)"""
    return float(np.float32(x))


def _normal(r):
    a = np.abs(r)
    bad = (a > 0) & (a < F32_MIN_NORMAL)            # NaN compares false
    assert not bad.any(), "a subnormal f32 intermediate: u |r| is no bound there; choose other inputs"
    return r


class EV:
    """float64 value with a running bound on the f32 evaluation's error"""

    def __init__(self, v, e=None):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.zeros_like(self.v) if e is None else np.asarray(e, dtype=np.float64)

    @staticmethod
    def lift(x):
        return x if isinstance(x, EV) else EV(x)

    def __add__(self, o):
        o = EV.lift(o)
        r = _normal(self.v + o.v)
        return EV(r, self.e + o.e + U * np.abs(r))

    __radd__ = __add__

    def __sub__(self, o):
        o = EV.lift(o)
        r = _normal(self.v - o.v)
        return EV(r, self.e + o.e + U * np.abs(r))

    def __mul__(self, o):
        o = EV.lift(o)
        r = _normal(self.v * o.v)
        return EV(r, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e + U * np.abs(r))

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = EV.lift(o)
        fin = np.isfinite(self.v) & np.isfinite(o.v)
        assert (np.abs(o.v) > o.e)[fin].all(), "a divisor that its own error bound reaches"
        with np.errstate(all="ignore"):
            r = _normal(self.v / o.v)
            return EV(r, (self.e + np.abs(r) * o.e) / (np.abs(o.v) - o.e) + U * np.abs(r))

    def sqrt(self):
        with np.errstate(all="ignore"):
            r = _normal(np.sqrt(self.v))
            return EV(r, np.sqrt(self.v + self.e) - np.sqrt(np.maximum(self.v - self.e, 0.0)) + U * np.abs(r))

    def maximum(self, o):                           # torch.maximum: a NaN on either side stays
        o = EV.lift(o)
        return EV(np.maximum(self.v, o.v), np.maximum(self.e, o.e))

    def clamp(self, c):                             # NaN stays, +-inf become +-c
        return EV(np.clip(self.v, -c, c), self.e)

    def clamp_max(self, c):                         # torch.clamp(x, max=c): NaN stays
        return EV(np.where(self.v > c, c, self.v), self.e)

    @staticmethod
    def where(mask, a, b):
        a, b = EV.lift(a), EV.lift(b)
        return EV(np.where(mask, a.v, b.v), np.where(mask, a.e, b.e))


class F32:
    """the same interface in numpy float32: one rounding per operation, no fused multiply-add"""

    def __init__(self, v):
        self.v = np.asarray(v, dtype=np.float32)

    @staticmethod
    def lift(x):
        return x if isinstance(x, F32) else F32(x)

    def __add__(self, o):
        return F32(self.v + F32.lift(o).v)

    __radd__ = __add__

    def __sub__(self, o):
        return F32(self.v - F32.lift(o).v)

    def __mul__(self, o):
        return F32(self.v * F32.lift(o).v)

    __rmul__ = __mul__

    def __truediv__(self, o):
        with np.errstate(all="ignore"):
            return F32(self.v / F32.lift(o).v)

    def sqrt(self):
        with np.errstate(all="ignore"):
            return F32(np.sqrt(self.v))

    def maximum(self, o):
        return F32(np.maximum(self.v, F32.lift(o).v))

    def clamp(self, c):
        return F32(np.clip(self.v, np.float32(-c), np.float32(c)))

    def clamp_max(self, c):
        return F32(np.where(self.v > np.float32(c), np.float32(c), self.v))

    @staticmethod
    def where(mask, a, b):
        return F32(np.where(mask, F32.lift(a).v, F32.lift(b).v))


def tolerance(ref):
    return 2.0 * ref.e + F32_DENORM


def ratio(got, ref):
    """worst |got - ref| / tolerance over the finite elements of the reference; where the reference is not finite the result
    must be the same non-finite value (exact)"""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.v.shape, (got.shape, ref.v.shape)
    fin = np.isfinite(ref.v)
    assert np.array_equal(np.isnan(got), np.isnan(ref.v)), "NaN where the definition has none, or none where it has one"
    inf = np.isinf(ref.v)
    assert np.array_equal(got[inf], ref.v[inf])
    if not fin.any():
        return 0.0
    return float((np.abs(got - ref.v)[fin] / tolerance(ref)[fin]).max())


# ------------------------------------------------------------------------------------------------------------------------
# the definitions, written once for both arithmetics
# ------------------------------------------------------------------------------------------------------------------------
WRONG_SGD = ("wd_after_momentum", "no_nesterov", "clip_after_wd", "neighbour_lr")
WRONG_ADAM = ("omb2_in_f32", "eps_in_sqrt", "no_running_max", "bias_of_previous_step", "neighbour_lr")
WRONG = WRONG_SGD + WRONG_ADAM[:-1]


def _clip(A, G, clip, clip_value, cf):
    if clip == CLIP_VALUE:
        return G.clamp(clip_value)
    if clip == CLIP_NORM:
        return G * A(cf)
    return G


def sgd_update(A, p, g, m, lr, wd, cf, mom, first, nest, clip, clip_value, wrong=None):
    """clip, weight decay (only where wd != 0), momentum (first step: buf = g'), Nesterov look-ahead -- torch.optim.SGD behind
    a per-parameter clipper.  p, g, m: f32 values; lr, wd, cf: per element.  Returns (p, buf)."""
    P, G, LR, WD = A(p), A(g), A(lr), A(wd)
    has_wd = np.asarray(wd) != 0
    if wrong == "clip_after_wd":
        G = _clip(A, A.where(has_wd, G + WD * P, G), clip, clip_value, cf)
    else:
        G = _clip(A, G, clip, clip_value, cf)
        if wrong != "wd_after_momentum":
            G = A.where(has_wd, G + WD * P, G)
    B = G if first else A(mom) * A(m) + G
    if wrong == "wd_after_momentum":
        B = A.where(has_wd, B + WD * P, B)
    if nest and wrong != "no_nesterov":
        return P - LR * (G + A(mom) * B), B
    return P - LR * B, B


def adam_update(A, p, g, m, v, x, lr, wd, cf, bias, beta1, beta2, eps, decoupled, amsgrad, clip, clip_value, wrong=None):
    """torch.optim.Adam / AdamW, single-tensor order; the scalars rounded as launch_adam_runs rounds them; bias = the two f32
    values adam_advance wrote.  Returns (p, m, v, vmax or None)."""
    b1, omb1, b2, omb2, fe = f32(beta1), f32(1.0 - beta1), f32(beta2), f32(1.0 - beta2), f32(eps)
    if wrong == "omb2_in_f32":
        omb2 = float(np.float32(1.0) - np.float32(beta2))
    P, G, M, V, WD = A(p), A(g), A(m), A(v), A(wd)
    G = _clip(A, G, clip, clip_value, cf)
    if decoupled:
        keep = (1.0 - np.asarray(lr, np.float64) * np.asarray(wd, np.float64)).astype(np.float32)   # f64, rounded once
        P = P * A(keep)
    else:
        G = A.where(np.asarray(wd) != 0, G + WD * P, G)
    M = A(b1) * M + A(omb1) * G
    V = A(b2) * V + (A(omb2) * G) * G
    X = None
    VH = V
    if amsgrad:
        X = V if wrong == "no_running_max" else A(x).maximum(V)
        VH = X
    if wrong == "eps_in_sqrt":
        DEN = (VH + A(fe)).sqrt() * A(bias[1])
    else:
        DEN = VH.sqrt() * A(bias[1]) + A(fe)
    STEP = A(lr) * A(bias[0])
    return P - STEP * (M / DEN), M, V, X


def adam_bias(t, beta1, beta2):
    """what adam_advance writes for step t: f64 arithmetic, stored f32"""
    return (f32(1.0 / (1.0 - beta1 ** t)), f32(1.0 / math.sqrt(1.0 - beta2 ** t)))


# ------------------------------------------------------------------------------------------------------------------------
# run tables
# ------------------------------------------------------------------------------------------------------------------------
LR_TABLE = (f32(0.02), 0.0, f32(0.005))             # one of the three learning rates is 0.0
WEIGHT_DECAY = f32(1e-4)
MOMENTUM = f32(0.9)
CLIP_VALUE_AT = f32(0.05)                           # inside the gradients' five decades: both sides of the clamp occur
CLIP_NORM_AT = 1.0
BETAS = (0.9, 0.999)
EPS = 1e-8
WG = 1024                                           # elements of one trip of a workgroup (256 threads x float4)
RUNS_GRID_CAP = 2048                                # launch_sgd_runs / launch_adam_runs
SGD_GRID_CAP = 8192                                 # launch_sgd, 256 elements a workgroup


class RunTable:
    def __init__(self, name, run_len, wd=None):
        self.name = name
        self.run_len = list(run_len)
        self.run_end = list(np.cumsum(self.run_len))
        self.n = int(self.run_end[-1])
        r = np.arange(len(self.run_len))
        self.lr_index = list((r % 3).astype(int))                       # neighbours never share a learning rate
        self.wd = list(wd) if wd is not None else [WEIGHT_DECAY if k % 2 else 0.0 for k in r]   # zero / non-zero alternate

    def per_element(self, values):
        return np.repeat(np.asarray(values, dtype=np.float64), self.run_len)

    def lr(self):
        return self.per_element([LR_TABLE[i] for i in self.lr_index])

    def neighbour_lr(self):
        """the wrong table: the first element of every run takes the lr of the run before it"""
        lr = self.lr()
        out = lr.copy()
        for s in self.run_end[:-1]:
            if 0 < s < self.n:
                out[s] = lr[s - 1]
        return out


# 17 runs, 12202 elements, 12 workgroups of 1024
MAIN = RunTable("main", [0, 1, 2, 3, 4, 5, 7, 8,      # a zero-length first run; the short runs (ends 1 .. 30)
                         993, 1, 1,                   # ends 1023, 1024, 1025
                         0,                           # a zero-length run in the middle
                         2500,                        # 1025 .. 3525: workgroups 1, 2 and 3
                         4571, 3, 4103,               # ends 8096, 8099, 12202 (not a multiple of 4)
                         0])                          # a zero-length last run
LEN1 = RunTable("len1", [1])
LEN3 = RunTable("len3", [2, 1])
SMALL = RunTable("small", [31, 0, 33], wd=[WEIGHT_DECAY, 0.0, 0.0])    # the hand-made Adam inputs, the non-finite cases
# the grid caps: n = 2048 * 1024 + 3 * 1024 + 5 makes `per` 2048 for the run kernels (two trips a thread); sgd_kernel's
# grid-stride loop wraps at 8192 * 256.  Two runs, the boundary no multiple of 4.
CAPPED_N = RUNS_GRID_CAP * WG + 3 * WG + 5
CAPPED = RunTable("capped", [1048579, CAPPED_N - 1048579])
CAPPED_SGD = RunTable("capped_sgd", [1048579, SGD_GRID_CAP * 256 + 5 - 1048579])

SGD_CLIP_VARIANTS = [(CLIP_NONE, True), (CLIP_VALUE, False), (CLIP_VALUE, True), (CLIP_NORM, False), (CLIP_NORM, True)]
ADAM_VARIANTS = [(c, d, a) for c in (CLIP_NONE, CLIP_VALUE, CLIP_NORM) for d in (False, True) for a in (False, True)]


def _inputs(n, seed):
    """f32 values: gradients over five decades, parameters O(1), zeros in g, m and v"""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(n) * 10.0 ** rng.uniform(-4.0, 1.0, n)
    p = rng.standard_normal(n) * 0.5
    m = rng.standard_normal(n) * 0.1
    v = (rng.standard_normal(n) * 0.1) ** 2
    g[rng.random(n) < 0.05] = 0.0
    m[rng.random(n) < 0.05] = 0.0
    v[rng.random(n) < 0.05] = 0.0
    x = v * rng.choice([0.25, 1.0, 4.0], n)          # the running maximum below, at and above v
    return {k: a.astype(np.float32) for k, a in (("p", p), ("g", g), ("m", m), ("v", v), ("x", x))}


def norm_coefs(g, table, clip_value):
    """the coefficient of every run as torch.nn.utils.clip_grad_norm_ derives it when called with that run alone (L2): an
    input of the update kernels, like the gradient"""
    import torch
    out = []
    for r, e in enumerate(table.run_end):
        s = e - table.run_len[r]
        q = torch.zeros(table.run_len[r], requires_grad=True)
        q.grad = torch.from_numpy(g[s:e].copy())
        with np.errstate(all="ignore"):
            total = torch.nn.utils.clip_grad_norm_([q], clip_value, foreach=False)
        out.append(float(torch.clamp(clip_value / (total + 1e-6), max=1.0)))
    return np.asarray(out, dtype=np.float32)


class Case:
    """one launch of one update kernel: its run table, hyper-parameters and inputs, all explicit"""

    def __init__(self, kind, table, seed, first=False, nest=False, clip=CLIP_NONE, decoupled=False, amsgrad=False, t=10,
                 special=None):
        self.kind, self.table, self.seed, self.first, self.nest, self.clip = kind, table, seed, first, nest, clip
        self.decoupled, self.amsgrad, self.t, self.special = decoupled, amsgrad, t, special
        self.name = f"{kind}-{table.name}" + (f"-clip{clip}" if kind in ("sgd_clip", "adam") else "") + \
            ("-nest" if nest else "") + ("-first" if first else "") + ("-w" if decoupled else "") + \
            ("-ams" if amsgrad else "") + (f"-t{t}" if kind == "adam" else "") + (f"-{special}" if special else "")
        self.clip_value = CLIP_VALUE_AT if clip == CLIP_VALUE else (CLIP_NORM_AT if clip == CLIP_NORM else 0.0)
        self._in = None

    def inputs(self):
        if self._in is None:
            n = self.table.n
            d = _inputs(n, self.seed)
            if self.first:
                d["m"] = np.full(n, np.nan, dtype=np.float32)       # a first step never reads the momentum buffer
            if self.special == "adam_edges":
                _adam_edges(d, self)
            if self.special == "nonfinite":
                _nonfinite(d, self)
            if self.kind == "sgd":                                  # the scalar kernel: one lr, one weight decay
                d["lr"], d["wd"] = np.full(n, LR_TABLE[0]), np.full(n, WEIGHT_DECAY)
            else:
                d["lr"], d["wd"] = self.table.lr(), self.table.per_element(self.table.wd)
            d["coefs"] = norm_coefs(d["g"], self.table, self.clip_value) if self.clip == CLIP_NORM else None
            d["cf"] = self.table.per_element(d["coefs"]) if self.clip == CLIP_NORM else None
            self._in = d
        return self._in

    def bias(self, t=None):
        return adam_bias(self.t if t is None else t, *BETAS)

    def evaluate(self, A=EV, wrong=None, bias=None):
        """{name: A} of the buffers the kernel writes"""
        d = self.inputs()
        lr = self.table.neighbour_lr() if wrong == "neighbour_lr" else d["lr"]
        if self.kind == "adam":
            if bias is None:
                bias = self.bias(self.t - 1) if wrong == "bias_of_previous_step" else self.bias()
            P, M, V, X = adam_update(A, d["p"], d["g"], d["m"], d["v"], d["x"], lr, d["wd"], d["cf"], bias, BETAS[0], BETAS[1],
                                     EPS, self.decoupled, self.amsgrad, self.clip, self.clip_value, wrong)
            out = {"p": P, "m": M, "v": V}
            if self.amsgrad:
                out["x"] = X
            return out
        P, B = sgd_update(A, d["p"], d["g"], d["m"], lr, d["wd"], d["cf"], MOMENTUM, self.first, self.nest, self.clip,
                          self.clip_value, wrong)
        return {"p": P, "m": B}

    def zero_expected(self, z):
        """the exact parameter of the all-zero Adam elements z: p * keep for AdamW, p for Adam without weight decay (with it
        the gradient is wd * p, no longer zero: None)"""
        d = self.inputs()
        if self.decoupled:
            keep = (1.0 - d["lr"][z].astype(np.float64) * d["wd"][z].astype(np.float64)).astype(np.float32)
            return d["p"][z] * keep
        return d["p"][z] if not d["wd"][z].any() else None

    def exact_unchanged(self):
        """elements whose parameter the definition leaves bit-equal: lr == 0 and a finite update to multiply it with (AdamW
        too: keep = 1 - 0 * wd = 1)"""
        d = self.inputs()
        return (d["lr"] == 0) & np.isfinite(d["g"]) & np.isfinite(d["v"]) & np.isfinite(d["x"])


def zero_slices():
    """the g = m = v = vmax = 0 elements of the hand-made Adam inputs: the first ZERO_AT of SMALL's two live runs"""
    return [slice(e - l, e - l + ZERO_AT) for l, e in zip(SMALL.run_len, SMALL.run_end) if l]


# hand-made Adam elements (table SMALL), the first ZERO_AT elements of each run
ZERO_AT = 4          # g = m = v = vmax = 0: Adam leaves p, AdamW gives p * keep, both exact
TINY_AT = 8          # v tiny against eps^2 and g = 0: eps is the denominator


def _adam_edges(d, case):
    for r, e in enumerate(case.table.run_end):
        s = e - case.table.run_len[r]
        if case.table.run_len[r] < 20:
            continue
        for k in ("g", "m", "v", "x"):
            d[k][s:s + ZERO_AT] = 0.0
        d["g"][s + ZERO_AT:s + TINY_AT] = 0.0
        d["v"][s + ZERO_AT:s + TINY_AT] = np.float32(1e-22)             # sqrt = 1e-11 against eps = 1e-8
        d["x"][s + ZERO_AT:s + TINY_AT] = np.float32(1e-22)
        d["m"][s + ZERO_AT:s + TINY_AT] = np.float32(1e-10)
        # vmax equal to the new v without any rounding in the way: g = 0, v = vmax = 0, m != 0 (the denominator is eps)
        d["g"][s + TINY_AT:s + TINY_AT + 2] = 0.0
        d["v"][s + TINY_AT:s + TINY_AT + 2] = 0.0
        d["x"][s + TINY_AT:s + TINY_AT + 2] = 0.0
        d["m"][s + TINY_AT:s + TINY_AT + 2] = np.float32(0.25)
        # ... and far above / far below it
        d["v"][s + 10:s + 14] = np.float32(0.01)
        d["g"][s + 10:s + 14] = np.float32(0.3)
        d["x"][s + 10:s + 12] = np.float32(1.0)
        d["x"][s + 12:s + 14] = np.float32(1e-6)


NONFINITE_G = {3: np.nan, 9: np.inf, 17: -np.inf, 40: np.nan, 47: np.inf, 55: -np.inf}   # both runs of SMALL, mixed residues
NONFINITE_V = {21: np.nan}
NONFINITE_X = {26: np.nan, 60: np.nan}


def _nonfinite(d, case):
    for i, val in NONFINITE_G.items():
        d["g"][i] = val
    if case.kind == "adam":
        for i, val in NONFINITE_V.items():
            d["v"][i] = val
        for i, val in NONFINITE_X.items():
            d["x"][i] = val


def update_cases():
    """every instantiation over MAIN, LEN1 and LEN3: 1 + 1 + 5 + 12 = 19 kernels a table"""
    out = []
    for ti, table in enumerate((MAIN, LEN1, LEN3)):
        out.append(Case("sgd", table, 100 + ti))
        out.append(Case("sgd_runs", table, 110 + ti))
        out += [Case("sgd_clip", table, 120 + ti, clip=c, nest=n) for c, n in SGD_CLIP_VARIANTS]
        out += [Case("adam", table, 130 + ti, clip=c, decoupled=d, amsgrad=a) for c, d, a in ADAM_VARIANTS]
    return out


def first_step_cases():
    return [Case("sgd", MAIN, 200, first=True), Case("sgd_runs", MAIN, 201, first=True),
            Case("sgd_clip", MAIN, 202, first=True, clip=CLIP_VALUE, nest=True)]


def adam_edge_cases():
    """the hand-made elements at t = 1 and with the bias of t = 10^6 (exactly [1, 1]), all twelve instantiations"""
    return [Case("adam", SMALL, 300, clip=c, decoupled=d, amsgrad=a, t=t, special="adam_edges")
            for t in (1, 10 ** 6) for c, d, a in ADAM_VARIANTS]


def nonfinite_cases():
    return [Case("sgd_clip", SMALL, 400, clip=CLIP_VALUE, special="nonfinite"),
            Case("sgd_clip", SMALL, 401, clip=CLIP_VALUE, nest=True, special="nonfinite"),
            Case("adam", SMALL, 402, clip=CLIP_VALUE, amsgrad=True, special="nonfinite"),
            Case("adam", SMALL, 403, clip=CLIP_VALUE, decoupled=True, amsgrad=True, special="nonfinite")]


def capped_cases():
    return [Case("sgd_runs", CAPPED, 500), Case("sgd_clip", CAPPED, 501, clip=CLIP_NORM, nest=True),
            Case("adam", CAPPED, 502, clip=CLIP_VALUE, decoupled=True, amsgrad=True), Case("sgd", CAPPED_SGD, 503)]


def finite_small_cases():
    return update_cases() + first_step_cases() + adam_edge_cases()


# ------------------------------------------------------------------------------------------------------------------------
# the norm kernels
# ------------------------------------------------------------------------------------------------------------------------
GRAD_CHUNK = 4096                                   # solver.build.GRAD_CHUNK (asserted by the host test)
# parameter lengths in buffer order: the offsets they produce cover the residues 0 .. 3 mod 4
NORM_PARAM_LENGTHS = [1, 0, 2, 3, 5, 4, 4095, 4096, 4097, 64 * GRAD_CHUNK, 64 * GRAD_CHUNK + 1, 0]
NORM_TYPES = (NORM_L1, NORM_L2, NORM_INF)
# grad_chunk_norm_kernel: a thread adds at most 16 terms of a 4096-element chunk in address order (four trips of a float4; a
# chunk that starts off the 16-byte grid gives thread 0 a fifth, partial trip and as many elements fewer in its first), then 6
# butterfly levels, then the 3 joins of the four waves
CHUNK_DEPTH = 16 + 6 + 3


def norm_offsets():
    out, off = [], 0
    for n in NORM_PARAM_LENGTHS:
        out.append((off, n))
        off += n
    return out


def norm_total():
    return sum(NORM_PARAM_LENGTHS)


def coef_depth(nchunks_of_param):
    """grad_clip_coef_kernel: lane l adds partials l, l + 64, .. serially, then 6 butterfly levels"""
    return -(-nchunks_of_param // 64) + 6


def chunk_partials_ref(g, starts, lens, norm_type):
    """EV of every chunk's partial: sum g^2 (one more rounding per term for the square), sum |g| or max |g| (exact)"""
    g = np.asarray(g, dtype=np.float64)
    v, e = np.zeros(len(starts)), np.zeros(len(starts))
    with np.errstate(all="ignore"):
        for c, (s, l) in enumerate(zip(starts, lens)):
            a = np.abs(g[s:s + l])
            if norm_type == NORM_INF:
                v[c] = np.nan if np.isnan(a).any() else a.max()
            elif norm_type == NORM_L1:
                v[c], e[c] = a.sum(), CHUNK_DEPTH * U * a.sum()
            else:
                v[c], e[c] = (a * a).sum(), (CHUNK_DEPTH + 1) * U * (a * a).sum()
    return EV(v, e)


def coefs_ref(partials, ends, norm_type, clip_value):
    """(norms, coefs) as EV from the partials the first kernel wrote (inputs: exact)"""
    partials = np.asarray(partials, dtype=np.float64)
    nv, ne = np.zeros(len(ends)), np.zeros(len(ends))
    first = 0
    with np.errstate(all="ignore"):
        for q, last in enumerate(ends):
            part = partials[first:last]
            if norm_type == NORM_INF:
                nv[q] = 0.0 if not len(part) else (np.nan if np.isnan(part).any() else part.max())
            else:
                nv[q] = part.sum()
                ne[q] = coef_depth(last - first) * U * np.abs(part).sum()
            first = last
        norm = EV(nv, ne)
        if norm_type == NORM_L2:
            norm = norm.sqrt()
        coef = (EV(np.full(len(ends), f32(clip_value))) / (norm + f32(1e-6))).clamp_max(1.0)
    return norm, coef
