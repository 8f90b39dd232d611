"""Case tables, input builders, float64 references and bounds for the BatchNorm training kernels of csrc/train_bwd.hip:
    chan_reduce_kernel (modes 0 and 1), chan_finalize_kernel (modes 0 and 1), affine_act_kernel, affine_act_rows_kernel,
    bn_bwd_apply_kernel, bn_bwd_apply_rows_kernel, bn_slot_finalize_kernel, bn_sync_fwd_apply_kernel, bn_sync_bwd_apply_kernel
each on f16 and f32 tensors, reached through ops_train.bn_train_fwd / bn_train_bwd (fused) and bn_local_stats / bn_sync_fwd /
bn_local_grad_sums / bn_sync_bwd (split around the SyncBN collectives).  test_bn_host.py holds the tables to their own conditions on
the CPU; test_bn_gpu.py runs the kernels over them.  test_syncbn_gpu.py, test_train_gpu.py and test_train_x3_gpu.py keep what they
held before (large row counts, the autograd functions, whole steps).

Shapes.  Tensors are [1, 1, M, C], C = CV * N (N = 8 f16 / 4 f32 elements of a 16-byte channel vector).  Every M is computed from the
mirrored launch constants as the smallest that takes the branch named next to it; chan_lanes / rows_kernel_split / apply_blocks below
are the launchers' arithmetic and the host test evaluates them for every case.

Inputs.  f16-representable where the tensor is f16.  y: channel 0 is constant over the rows (var = 0, invstd = 1 / sqrt(eps)), channel
1 has mean exactly 0 (rows mirrored in sign), channel 2 of f32 tensors has |mean| / std = 1000 (what chan_reduce_kernel's pivot exists
for; f16 tensors keep the fused kernels' plain sums; the shifted-mean bound is an f32 property), the others have |mean| <= std / 2 and
row 0 -- the pivot of the f32 sums -- within std / 4 of the mean; dz leans to one side per channel and on y - mean, so that the sums of
the backward do not cancel (the ceiling below is relative to them).  Running statistics start from random values, gamma has both signs.
The backward's z is built by hand, not taken from a forward: z[m, c] = Z_SPECIALS[(m + c) % 7] = +0.0, the smallest positive subnormal
of the type, -0.0, NaN, 1, the negative subnormal, -1; the reference applies `z > 0` to the same tensor.  The backward's mean, invstd
and scale are the forward reference rounded to f32 (the numbers a forward hands on), and the backward reference starts from them.

References.  Plain float64 formulas: mean, biased variance (two passes), invstd = 1 / sqrt(var + eps), z = act((y - mean) * invstd *
gamma + beta + res); running_var takes M > 1 ? var * M / (M - 1) : var (the kernels' own definition at M = 1); g = dz * (z > 0),
dbeta = gm * sum g, dgamma = gm * sum g * xhat, dy = scale * (g - sum g / M - xhat * sum g * xhat / M), dres = g.  eps, momentum and
grad_mult enter as the f32 numbers the kernels receive.

Bounds, per element, nothing left out, no max-norm scaling.  U = 2^-24, u_T = 2^-11 for f16 outputs and 0 for f32 outputs.
  * exact (torch.equal): dres, the y = None dy, the dgamma = 0 of the y = None modes, sentinels outside a written slice, the zeroed
    foreign slots and the row count of a slot.
  * a sum of the rank's M rows in chan_reduce_kernel: every term passes through at most
        n = min(M, k + ceil(log2(rows_per_pass)))       k = ceil(M / (blocks * rows_per_pass)) rows of one thread,
    f32 additions (the thread's serial sum, then the LDS tree over the row lanes; an addition of 0 is exact, so never more than M;
    the block partials are added in f64 and add none).  n <= M, the count the rule of pointwise_cases.py would take.
        dm   = sum (y - K) / M          b_dm   = (n + 1) U sum |y - K| / M            (+1: the subtraction; K = y[0] f32, 0 f16)
        var  = sum (y - K)^2 / M - dm^2 b_var  = (n + 3) U sum (y - K)^2 / M + 2 |dm| b_dm + b_dm^2     (+3: y - K twice, the square)
        mean = K + dm                   b_mean = b_dm (+ U |mean| once it is rounded to f32)
        s0   = sum g                    b_s0   = (n + 1) U sum |g|                    (+1: the f32 rounding of the f64 total)
        s1   = sum g xhat               b_s1   = (n + 4) U sum |g xhat|               (+4: y - mean, * invstd, g * xhat, the total)
        dbeta, dgamma = gm * s          b      = gm b_s + U |ref|
  * ranks combined by bn_slot_combine (f64): mean = sum w_r mean_r, var = sum w_r (var_r + (mean_r - mean)^2), w_r = M_r / M, so
        b_mean = sum w_r b_dm_r,   b_var = sum w_r (b_var_r + 2 |mean_r - mean| b_dm_r + b_dm_r^2);   one rank: the lines above.
  * invstd: b_invstd = max |f(var +- b_var) - f(var)| + U invstd, f(v) = 1 / sqrt(max(v, 0) + eps) evaluated, not linearised (at
    var = 0 the slope is 1 / (2 eps^1.5)).   scale = gamma * invstd: b_scale = |gamma| b_invstd + U |scale|.
  * z = T(act(y * scale + (beta - mean * scale) + res)): the statistics' bounds times the element's sensitivity to them, then the
    named roundings (mean * scale, the shift's subtraction, y * scale or its FMA, the add of shift, the add of res: 5) on
    A = |y scale| + |mean scale| + |beta| + |res|:
        b_z = |y - mean| b_scale + |scale| b_mean + b_scale b_mean + 5 U A + u_T |ref| + q
    q = 2^-24, the f16 subnormal quantum, for f16 outputs (BatchNorm outputs pass through 0; q stands for u_T |ref| below 2^-14).
  * running_mean = (1 - momentum) * old + momentum * mean:  b = momentum b_mean + 4 U (|(1 - momentum) old| + |momentum mean|)
    (1 - momentum in f32, two products, one sum); running_var the same with b_var * M / (M - 1) and the f32 rounding of the variance.
  * dy = T(scale * (g - s0 / M - xhat * s1 / M)), A = |scale| (|g| + |s0 / M| + |xhat s1 / M|):
        b_dy = |scale| b_s0 / M + |scale xhat| b_s1 / M + 8 U A + u_T |ref| + q
    (1 / M in f32 on two terms, s0 / M, y - mean, * invstd, s1 / M, xhat * that, two subtractions, * scale: each at most U A; 8
    covers any contraction).  In the split kernels s0, s1 and their bounds are the sums over the ranks.
  * ceiling from test_syncbn_gpu.py: over the channels with |mean| / std <= 10 these bounds divided by max |ref| stay below
    invstd 2e-6, z 2e-6 (f32) / 4e-3 (f16), dy, dgamma, dbeta 2e-5 / 2e-2.  test_bn_host.py asserts it for every case but the
    one- and two-row ones, where max |ref| is taken over a handful of elements (M = 2, f32: 3.7e-6 for z).

Worst err / bound per kernel path, mode and dtype, measured on an MI355X on 2026-10-19 at the commit that adds this file (parent
9620359):
    path and quantity                           f16    f32
    affine_act z                                0.995  0.200
    affine_act_rows z                           0.998  0.209
    bn_bwd_apply dy                             0.993  0.186     (2026-10-20, at the commit that gives the three backward-apply
                                                                  kernels one expression, parent 7976952; before: 0.993  0.172)
    bn_bwd_apply_rows dy                        0.998  0.226
    bn_sync_bwd_apply w1-3 dy                   0.998  0.235
    bn_sync_fwd_apply w1-3 z                    0.998  0.209
    chan_reduce+finalize m0 invstd              0.700  0.700
    chan_reduce+finalize m0 mean                0.065  0.478
    chan_reduce+finalize m0 rm                  0.492  0.541
    chan_reduce+finalize m0 rv                  0.332  0.318
    chan_reduce+finalize m0 scale               0.361  0.772
    chan_reduce+finalize m1 dbeta               0.099  0.154
    chan_reduce+finalize m1 dbias (y=None)      0.011  0.021
    chan_reduce+finalize m1 dgamma              0.118  0.093
    slot_finalize m1 w1-3 dbeta                 0.118  0.189
    slot_finalize m1 w1-3 dgamma                0.172  0.156
    slot_finalize+sync_fwd w1-3 invstd          0.700  0.700
    slot_finalize+sync_fwd w1-3 mean            0.065  0.478
    slot_finalize+sync_fwd w1-3 rm              0.497  0.545
    slot_finalize+sync_fwd w1-3 rv              0.332  0.318
    slot_finalize+sync_fwd w1-3 scale           0.361  0.772
(w1-3: the worst over one, two and three simulated ranks.)  The f16 figures close to 1 are the rounding of the result to f16 (half an
ulp against u_T = 2^-11), not the statistics; invstd's 0.700 is a channel with var = 0, whose bound is little more than the f32 rounding of
1 / sqrt(eps).  dres, the y = None dy and dgamma, every sentinel, foreign slot and row count, the second run of every call, the world-3
buffers with an empty slot against world 2, and world 1 against the fused kernels (dy as documented there) were exact.
"""
import functools
from collections import namedtuple

import torch

from pointwise_cases import F16, F32, DTYPES, VEC, U_T, U32, SENTINEL, dt_name  # noqa: F401  (one rule, one sentinel)

U = U32
Q16 = 2.0 ** -24                          # the f16 subnormal quantum

# launch constants mirrored from csrc/train_bwd.hip (test_bn_host.py greps the source for them)
BLOCK = 256                               # threads per workgroup of every BN kernel
CHAN_ROWS = 8                             # chan_blocks: rows per row lane that the uncapped grid is sized for
CHAN_BLOCK_CAP = 1024                     # ... and its cap (the workspace holds 1024 block partials)
AA_ROWS = BN_ROWS = SB_ROWS = 8           # rows a thread of affine_act_rows / bn_bwd_apply_rows / the sync apply kernels walks
CV_MAX = 256                              # largest channel-vector count the launchers accept
UNROLL = {0: 4, 1: 2}                     # rows in flight in chan_reduce_kernel's unrolled loop, per mode

CV_POW2, CV_ODD = 4, 3                    # rows kernels and shift/mask sb_split; generic kernels and div/mod sb_split
CEIL = {"invstd": {F32: 2e-6, F16: 2e-6}, "z": {F32: 2e-6, F16: 4e-3}, "grad": {F32: 2e-5, F16: 2e-2}}
CEIL_MIN_ROWS = 63                        # the smallest M of the table beyond the CV = 1 one- and two-row cases
Z_SPECIALS = ("+0", "+sub", "-0", "nan", "+1", "-sub", "-1")
SUBNORMAL = {F16: 2.0 ** -24, F32: 2.0 ** -149}
WORLDS = (1, 2, 3)


# ------------------------------------------------------------------------------------------------------------------------
# launch geometry
# ------------------------------------------------------------------------------------------------------------------------
def rows_per_pass(CV):
    return BLOCK // CV


def chan_blocks(M, CV):
    return max(1, min(CHAN_BLOCK_CAP, -(-M // (rows_per_pass(CV) * CHAN_ROWS))))


def chan_lanes(M, CV):
    """rows that every row lane (block, rl < rows_per_pass) of chan_reduce_kernel adds"""
    step = chan_blocks(M, CV) * rows_per_pass(CV)
    return [max(0, -(-(M - lane) // step)) for lane in range(step)]


def chan_profile(M, CV, mode):
    """what the row lanes do: idle lanes, (unrolled iterations, tail steps) of the busy ones"""
    u, ks = UNROLL[mode], set(chan_lanes(M, CV))
    return {"idle": 0 in ks, "loops": {(k // u, k % u) for k in ks if k}}


def n_red(M, CV):
    levels = (rows_per_pass(CV) - 1).bit_length()
    return min(M, max(chan_lanes(M, CV)) + levels)


def is_pow2(CV):
    return CV & (CV - 1) == 0


def rows_kernel_split(M, CV, rows=AA_ROWS):
    """(rows written by the fast path, rows written by the tail loop) of affine_act_rows / bn_bwd_apply_rows"""
    ppb = BLOCK // CV
    fast = tail = 0
    for b in range(-(-M // (ppb * rows))):
        for lane_px in range(ppb):
            m0 = b * ppb * rows + lane_px
            if m0 + (rows - 1) * ppb < M:
                fast += rows
            else:
                tail += len(range(m0, min(M, m0 + rows * ppb), ppb))
    return fast, tail


def apply_blocks(M, CV):
    """(workgroups, threads past M * CV) of the generic apply kernels and of the sync apply kernels"""
    t = M * CV
    g, s = -(-t // BLOCK), -(-t // (BLOCK * SB_ROWS))
    return (g, g * BLOCK - t), (s, s * BLOCK * SB_ROWS - t)


def rank_rows(M, W):
    """rows of each of W simulated ranks (contiguous chunks); with M < W the last ranks are empty: their slots hold zeros"""
    base, extra = divmod(M, W)
    return [base + (r < extra) for r in range(W)]


# ------------------------------------------------------------------------------------------------------------------------
# the tables
# ------------------------------------------------------------------------------------------------------------------------
# into: which of (dgamma, dbeta) land in a caller's slot
BnCase = namedtuple("BnCase", "CV M res relu eps momentum grad_mult into strided note")
_SETTINGS = [(True, True, 1e-5, 0.1, 1.0, "both"), (False, True, 1e-3, 0.03, 0.25, "dgamma"), (True, False, 1e-5, 0.03, 0.25, "none"),
             (False, False, 1e-3, 0.1, 1.0, "both")]


def _cases():
    shapes = [(1, 1, "CV = 1, one row: 255 idle lanes; the M > 1 guard"), (1, 2, "CV = 1, two rows"),
              (1, 255, "CV = 1: one idle lane, one row each")]
    for CV in (CV_POW2, CV_ODD):
        r = rows_per_pass(CV)
        shapes += [(CV, r - 1, "M < rows_per_pass: an idle lane"), (CV, r, "tail loop only, no idle lane"),
                   (CV, 4 * r, "mode 0: one unrolled step, remainder 0; mode 1: two, remainder 0"),
                   (CV, 5 * r, "mode 0: remainder 1; mode 1: two unrolled steps, remainder 1"),
                   (CV, 6 * r, "mode 0: remainder 2; mode 1: three unrolled steps, remainder 0"),
                   (CV, 7 * r, "mode 0: remainder 3; mode 1: remainder 1"),
                   (CV, 14 * r, "two blocks; dealt to two ranks of 7 r rows: the row after a rank's last is the next rank's first"),
                   (CV, 16 * r, "two blocks; rows kernels: fast path only (pow2); sync apply: two workgroups"),
                   (CV, 16 * r + 1, "three blocks; rows kernels: one tail row (pow2); a ragged last workgroup")]
    shapes += [(CV_MAX, CHAN_ROWS * CHAN_BLOCK_CAP + 1, "CV = 256: rows_per_pass = 1, the 1024-block cap at its smallest M")]
    out = []
    for i, (CV, M, note) in enumerate(shapes):
        res, relu, eps, mom, gm, into = _SETTINGS[i % len(_SETTINGS)]
        if CV == CV_MAX:
            res = False
        out.append(BnCase(CV, M, res, relu, eps, mom, gm, into, False, note))
    out += [BnCase(CV_POW2, 16 * rows_per_pass(CV_POW2) + 1, True, True, 1e-5, 0.1, 0.25, "both", True, "every tensor a channel slice; rows kernels"),
            BnCase(CV_ODD, 7 * rows_per_pass(CV_ODD), True, True, 1e-3, 0.03, 1.0, "none", True, "every tensor a channel slice; generic kernels")]
    return out


BN_CASES = _cases()
# the no-statistics modes of bn_train_bwd (y = None): bias gradients and ReLU masks of the conv layers
NoStatCase = namedtuple("NoStatCase", "CV M relu grad_mult strided")
NOSTAT_CASES = [NoStatCase(CV, M, relu, gm, False) for CV in (CV_POW2, CV_ODD) for relu in (False, True)
                for (M, gm) in ((1, 1.0), (5 * rows_per_pass(CV), 0.25), (16 * rows_per_pass(CV) + 1, 1.0))]
NOSTAT_CASES += [NoStatCase(CV_POW2, 16 * rows_per_pass(CV_POW2) + 1, True, 0.25, True), NoStatCase(CV_ODD, 7 * rows_per_pass(CV_ODD), True, 0.25, True)]
# hand-built gathered buffers: where the two live ranks of a world-2 run sit in a world-3 buffer
HAND_SLOTS = {"empty_middle": (0, 2), "empty_first": (1, 2), "empty_middle_nan": (0, 2)}
# ..._nan: the empty slot's mean and variance fields hold NaN.  A slot without rows carries no statistics, whatever those fields hold;
# with zeros in them, combining the slot instead of skipping it changes no f32 output (var * n / n in f64), so zeros cannot pin the skip
HAND_POISON = {"empty_middle_nan": 1}
HAND_CASES = [c for c in BN_CASES if c.M >= 2 and c.CV != CV_MAX]
# pixel strides of the strided cases, C + k * N, and the channel offset of the slice, per tensor
STRIDE_K = {"y": 1, "res": 2, "z": 3, "dz": 4, "dy": 5, "dres": 6, "zin": 7}
GUARD_ROWS = -(-(BLOCK - 1) // CV_ODD) + 1      # sentinel rows behind the last: more than the threads past M * CV of a generic kernel cover
OFFSET_N = {"y": 1, "res": 0, "z": 1, "dz": 0, "dy": 1, "dres": 0, "zin": 1}


def bn_id(c):
    extra = "".join(["-res" if getattr(c, "res", False) else "", "-relu" if c.relu else "", "-strided" if c.strided else ""])
    return f"cv{c.CV}-m{c.M}{extra}"


def channels(c, dt):
    return c.CV * VEC[dt]


def stride_of(name, C, dt):
    return C + STRIDE_K[name] * VEC[dt]


def offset_of(name, dt):
    return OFFSET_N[name] * VEC[dt]


# ------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------
def _seed(*parts):
    return int(sum((i + 1) * 7919 * int(p) for i, p in enumerate(parts)) % (2 ** 31))


def z_special(M, C, dt):
    """the hand-built post-activation tensor of the backward kernels"""
    s = SUBNORMAL[dt]
    vals = torch.tensor([0.0, s, -0.0, float("nan"), 1.0, -s, -1.0], dtype=torch.float64).to(dt)
    idx = (torch.arange(M)[:, None] + torch.arange(C)[None, :]) % len(Z_SPECIALS)
    return vals[idx]


@functools.lru_cache(maxsize=None)
def bn_inputs(case, dt):
    """y, res, dz, zin [M, C] of type dt; gamma, beta, rm0, rv0 f32 [C]"""
    M, C = case.M, channels(case, dt)
    g = torch.Generator().manual_seed(_seed(M, C, VEC[dt], case.strided))
    sd = torch.linspace(0.5, 2.0, C)
    mu = torch.linspace(-0.5, 0.5, C) * sd
    e = torch.randn(M, C, generator=g)
    y = e * sd + mu
    y[0] = mu + 0.25 * sd
    y[:, 0] = 1.5
    half = M // 2
    y[M - half:, 1] = -y[:half, 1].flip(0)
    if M % 2:
        y[half, 1] = 0.0
    y = y.to(dt)
    y[M - half:, 1] = -y[:half, 1].flip(0)          # mirrored after the rounding too
    if dt == F32:
        y[:, 2] = 1000.0 + torch.randn(M, generator=g)
        y[0, 2] = 1000.25
    sign = 1 - 2 * (torch.arange(C) % 2).float()
    # dz leans to one side per channel and on y - mean: sum g and sum g * xhat are no cancelling sums (the ceiling is a relative one)
    dz = 0.5 * torch.randn(M, C, generator=g) + 0.75 * sign + 0.5 * e
    out = {"y": y, "dz": dz.to(dt), "zin": z_special(M, C, dt),
           "res": torch.randn(M, C, generator=g).to(dt) if getattr(case, "res", False) else None}
    out["gamma"] = (torch.rand(C, generator=g) + 0.5) * sign
    out["beta"] = torch.randn(C, generator=g)
    out["rm0"] = torch.randn(C, generator=g)
    out["rv0"] = torch.rand(C, generator=g) + 0.5
    return out


def nostat_inputs(case, dt):
    M, C = case.M, channels(case, dt)
    g = torch.Generator().manual_seed(_seed(M, C, VEC[dt], 3))
    return {"dz": torch.randn(M, C, generator=g).to(dt), "zin": z_special(M, C, dt)}


def f32v(x):
    """the f32 number a kernel receives for a Python float, as a Python float"""
    return torch.tensor(x, dtype=torch.float32).double().item()


def slab(t, name, dt, fill=None):
    """t [M, C] as the channel slice of the first M rows of its own wider and longer sentinel-filled buffer [M + GUARD_ROWS, stride]:
    (buffer, view)"""
    M, C = t.shape
    it = torch.int16 if dt == F16 else torch.int32
    buf = torch.full((M + GUARD_ROWS, stride_of(name, C, dt)), SENTINEL[dt], dtype=it).view(dt)
    off = offset_of(name, dt)
    view = buf[:M, off:off + C]
    if fill is not False:
        view.copy_(t)
    return buf, view


def read_strided(buf, off, stride, M, C):
    """rows of C elements at off + m * stride of the flat buffer: what a kernel reads with that pixel stride"""
    flat = buf.reshape(-1)
    idx = off + torch.arange(M)[:, None] * stride + torch.arange(C)[None, :]
    return flat[idx.clamp_max(flat.numel() - 1)]


# ------------------------------------------------------------------------------------------------------------------------
# float64 references
# ------------------------------------------------------------------------------------------------------------------------
def mask_of(z, relu, ge=False):
    if not relu:
        return torch.ones_like(z, dtype=torch.bool)
    return (z >= 0) if ge else (z > 0)


@functools.lru_cache(maxsize=None)
def fwd_reference(case, dt, wrong=None):
    """wrong: 'unbiased_out' (unbiased variance in the output), 'biased_running' (biased variance in the running statistics)"""
    inp = bn_inputs(case, dt)
    y, M = inp["y"].double(), case.M
    eps, mom = f32v(case.eps), f32v(case.momentum)
    mean = y.mean(0)
    var = (y - mean).square().mean(0)
    unb = var * M / (M - 1) if M > 1 else var
    vo = unb if wrong == "unbiased_out" else var
    invstd = 1.0 / torch.sqrt(vo + eps)
    scale = inp["gamma"].double() * invstd
    z = (y - mean) * scale + inp["beta"].double()
    if case.res:
        z = z + inp["res"].double()
    if case.relu:
        z = z.clamp_min(0.0)
    rv_in = var if wrong == "biased_running" else unb
    return {"mean": mean, "var": var, "invstd": invstd, "scale": scale, "z": z,
            "rm": (1 - mom) * inp["rm0"].double() + mom * mean, "rv": (1 - mom) * inp["rv0"].double() + mom * rv_in}


def stats_in(case, dt):
    """mean, invstd, scale f32 [C]: what the backward kernels are handed"""
    fw = fwd_reference(case, dt)
    return fw["mean"].float(), fw["invstd"].float(), fw["scale"].float()


@functools.lru_cache(maxsize=None)
def bwd_reference(case, dt, wrong=None):
    """g (type dt: dres), dy, s0, s1 (float64).  wrong: 'drop_xhat' (dy without its sum g*xhat term), 'mask_ge' (z >= 0)"""
    inp = bn_inputs(case, dt)
    mean, invstd, scale = (t.double() for t in stats_in(case, dt))
    y, dz, M = inp["y"].double(), inp["dz"].double(), case.M
    g = torch.where(mask_of(inp["zin"], case.relu, wrong == "mask_ge"), dz, torch.zeros_like(dz))
    xh = (y - mean) * invstd
    s0, s1 = g.sum(0), (g * xh).sum(0)
    dy = scale * (g - s0 / M - (0 if wrong == "drop_xhat" else xh * (s1 / M)))
    return {"g": g.to(dt), "dy": dy, "s0": s0, "s1": s1}


def local_sums(case, dt, parts, global_dgamma=False):
    """per rank with rows: (dbeta, dgamma) references = gm * the rank's own sums.  global_dgamma: WRONG on purpose -- all ranks' sums"""
    inp, bw = bn_inputs(case, dt), bwd_reference(case, dt)
    mean, invstd, _ = (t.double() for t in stats_in(case, dt))
    gm, out, lo = f32v(case.grad_mult), [], 0
    for Mr in parts:
        g = bw["g"][lo:lo + Mr].double()
        xh = (inp["y"][lo:lo + Mr].double() - mean) * invstd
        out.append((gm * g.sum(0), gm * (bw["s1"] if global_dgamma else (g * xh).sum(0))))
        lo += Mr
    return out


def nostat_reference(case, dt, ge=False):
    inp = nostat_inputs(case, dt)
    dz = inp["dz"]
    g = torch.where(mask_of(inp["zin"], case.relu, ge), dz, torch.zeros_like(dz))
    A = g.double().abs().sum(0)
    gm = f32v(case.grad_mult)
    ref = gm * g.double().sum(0)
    return {"dy": g, "dbeta": ref, "b_dbeta": gm * (n_red(case.M, case.CV) + 1) * U * A + U * ref.abs()}


def combine_slots(slots, count_empty=False):
    """Chan's update over (n, mean, var) float64 slots in order, empty slots skipped.  count_empty: WRONG on purpose -- an empty slot
    is taken as a rank with one row of zeros"""
    n = mean = var = None
    for (nb, mb, vb) in slots:
        if nb == 0:
            if not count_empty:
                continue
            nb, mb, vb = 1, torch.zeros_like(slots[-1][1]), torch.zeros_like(slots[-1][1])
        if n is None:
            n, mean, var = nb, mb.clone(), vb.clone()
            continue
        nt, d = n + nb, mb - mean
        var = (var * n + vb * nb + d * d * (n * nb / nt)) / nt
        mean = mean + d * (nb / nt)
        n = nt
    return n, mean, var


def rank_slots(case, dt, parts):
    """float64 (n, mean, var) of every rank's rows, (0, 0, 0) for an empty rank"""
    y, out, lo = bn_inputs(case, dt)["y"].double(), [], 0
    zero = torch.zeros(y.shape[1], dtype=torch.float64)
    for Mr in parts:
        yr = y[lo:lo + Mr]
        out.append((Mr, yr.mean(0), (yr - yr.mean(0)).square().mean(0)) if Mr else (0, zero, zero))
        lo += Mr
    return out


# ------------------------------------------------------------------------------------------------------------------------
# bounds
# ------------------------------------------------------------------------------------------------------------------------
def _invstd_bound(var, b_var, eps):
    f = lambda v: 1.0 / torch.sqrt(v.clamp_min(0.0) + eps)
    return torch.maximum((f(var - b_var) - f(var)).abs(), (f(var + b_var) - f(var)).abs()) + U * f(var)


def fwd_bounds(case, dt, parts):
    """bounds of mean, invstd, scale, rm, rv [C] and z [M, C] for ranks of `parts` rows (one entry: the fused kernels)"""
    inp, fw = bn_inputs(case, dt), fwd_reference(case, dt)
    y, M = inp["y"].double(), case.M
    eps, mom = f32v(case.eps), f32v(case.momentum)
    b_mean, b_var, lo = 0.0, 0.0, 0
    for Mr in parts:
        if Mr == 0:
            continue
        yr = y[lo:lo + Mr]
        lo += Mr
        f = yr - (yr[0] if dt == F32 else 0.0)
        n, dm = n_red(Mr, case.CV), f.mean(0)
        b_dm = (n + 1) * U * f.abs().mean(0)
        b_var_r = (n + 3) * U * f.square().mean(0) + 2 * dm.abs() * b_dm + b_dm ** 2
        w = Mr / M
        b_mean = b_mean + w * b_dm
        b_var = b_var + w * (b_var_r + 2 * (yr.mean(0) - fw["mean"]).abs() * b_dm + b_dm ** 2)
    b_mean32 = b_mean + U * fw["mean"].abs()
    b_invstd = _invstd_bound(fw["var"], b_var, eps)
    gamma, beta = inp["gamma"].double(), inp["beta"].double()
    b_scale = gamma.abs() * b_invstd + U * fw["scale"].abs()
    A = (y * fw["scale"]).abs() + (fw["mean"] * fw["scale"]).abs() + beta.abs()
    if case.res:
        A = A + inp["res"].double().abs()
    b_z = (y - fw["mean"]).abs() * b_scale + fw["scale"].abs() * b_mean32 + b_scale * b_mean32 + 5 * U * A + U_T[dt] * fw["z"].abs()
    if dt == F16:
        b_z = b_z + Q16
    unb_k = M / (M - 1) if M > 1 else 1.0
    b_rm = mom * b_mean32 + 4 * U * (((1 - mom) * inp["rm0"].double()).abs() + (mom * fw["mean"]).abs())
    b_rv = mom * b_var * unb_k + 4 * U * (((1 - mom) * inp["rv0"].double()).abs() + (mom * fw["var"] * unb_k).abs())
    return {"mean": b_mean32, "invstd": b_invstd, "scale": b_scale, "z": b_z, "rm": b_rm, "rv": b_rv, "var": b_var}


def bwd_bounds(case, dt, parts):
    """bounds of dy [M, C] and, per rank with rows, of (dbeta, dgamma) from its local sums"""
    inp, bw = bn_inputs(case, dt), bwd_reference(case, dt)
    mean, invstd, scale = (t.double() for t in stats_in(case, dt))
    y, M, gm = inp["y"].double(), case.M, f32v(case.grad_mult)
    g = bw["g"].double()
    xh = (y - mean) * invstd
    b_s0, b_s1, local, lo = 0.0, 0.0, [], 0
    refs = local_sums(case, dt, parts)
    for Mr, (dbeta, dgamma) in zip(parts, refs):
        if Mr == 0:
            local.append(None)
            continue
        n = n_red(Mr, case.CV)
        b0 = (n + 1) * U * g[lo:lo + Mr].abs().sum(0)
        b1 = (n + 4) * U * (g[lo:lo + Mr] * xh[lo:lo + Mr]).abs().sum(0)
        lo += Mr
        local.append((gm * b0 + U * dbeta.abs(), gm * b1 + U * dgamma.abs()))
        b_s0, b_s1 = b_s0 + b0, b_s1 + b1
    A = scale.abs() * (g.abs() + (bw["s0"] / M).abs() + (xh * (bw["s1"] / M)).abs())
    b_dy = scale.abs() * b_s0 / M + (scale * xh).abs() * b_s1 / M + 8 * U * A + U_T[dt] * bw["dy"].abs()
    if dt == F16:
        b_dy = b_dy + Q16
    return {"dy": b_dy, "local": local}


def ratio(got, ref, b):
    """worst |got - ref| / bound over all elements; an element whose bound is 0 must be met exactly; a NaN anywhere is inf"""
    err = (got.double() - ref).abs()
    b = b.expand_as(err) if torch.is_tensor(b) else torch.full_like(err, b)
    r = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    r = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), r)
    return r.max().item()


def eligible(case, dt):
    """channels that the ceiling of test_syncbn_gpu.py speaks about: |mean| / std <= 10 (std > 0), in maps of at least CEIL_MIN_ROWS
    rows -- a max-norm over two or five rows of one channel vector is the size of single elements, not of a map"""
    fw = fwd_reference(case, dt)
    return (fw["mean"].abs() <= 10 * torch.sqrt(fw["var"])) & (fw["var"] > 0) & (case.M >= CEIL_MIN_ROWS)


# ------------------------------------------------------------------------------------------------------------------------
# the same formulas in f32 on the CPU (stored tensors rounded to their type): shows that the bounds are attainable
# ------------------------------------------------------------------------------------------------------------------------
def emulate(case, dt, parts):
    inp = bn_inputs(case, dt)
    y32, M = inp["y"].float(), case.M
    eps, mom = f32v(case.eps), torch.tensor(case.momentum, dtype=torch.float32)
    slots, lo = [], 0
    for Mr in parts:
        if Mr == 0:
            slots.append((0, None, None))
            continue
        yr = y32[lo:lo + Mr]
        lo += Mr
        K = yr[0] if dt == F32 else torch.zeros_like(yr[0])
        f = yr - K
        dm = f.sum(0).double() / Mr
        slots.append((Mr, K.double() + dm, ((f * f).sum(0).double() / Mr - dm * dm).clamp_min(0.0)))
    live = next(s for s in slots if s[0])
    slots = [s if s[0] else (0, torch.zeros_like(live[1]), torch.zeros_like(live[1])) for s in slots]
    n, mean, var = combine_slots(slots)
    invstd = 1.0 / torch.sqrt(var + eps)
    mean32, is32 = mean.float(), invstd.float()
    sc = inp["gamma"] * is32
    z = y32 * sc + (inp["beta"] - mean32 * sc)
    if case.res:
        z = z + inp["res"].float()
    if case.relu:
        z = z.clamp_min(0.0)
    unb = (var * n / (n - 1) if n > 1 else var).float()
    out = {"mean": mean32, "invstd": is32, "scale": sc, "z": z.to(dt), "rm": (1 - mom) * inp["rm0"] + mom * mean32,
           "rv": (1 - mom) * inp["rv0"] + mom * unb}
    m_in, is_in, sc_in = stats_in(case, dt)
    dz32 = inp["dz"].float()
    g = torch.where(mask_of(inp["zin"], case.relu), dz32, torch.zeros_like(dz32))
    xh = (y32 - m_in) * is_in
    gm, local, s0, s1, lo = torch.tensor(case.grad_mult, dtype=torch.float32), [], 0.0, 0.0, 0
    for Mr in parts:
        if Mr == 0:
            local.append(None)
            continue
        a0, a1 = g[lo:lo + Mr].sum(0).double(), (g[lo:lo + Mr] * xh[lo:lo + Mr]).sum(0).double()
        lo += Mr
        local.append((a0.float() * gm, a1.float() * gm))
        s0, s1 = s0 + a0, s1 + a1
    invM = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(M), dtype=torch.float32)
    out["dy"] = (sc_in * (g - s0.float() * invM - xh * (s1.float() * invM))).to(dt)
    out["dres"] = g.to(dt)
    out["local"] = local
    return out
