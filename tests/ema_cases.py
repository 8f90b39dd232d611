"""Cases, float64 oracle and error bound of the weight-EMA kernels (csrc/ema.hip): ema_advance_kernel,
ema_lerp_segments_kernel, ema_swap_segments_kernel.

The definition (one update, t the 0-based update count before it):

    d = min(decay, (1 + t) / (10 + t)) under warm-up, else decay            in f64
    w = f32(1 - d)                                                          rounded once
    e' = e + w (p - e)

The oracle evaluates e' in float64 with the kernel's own f32 w, so w carries no error.

Bound of one step.  The kernel computes s = fl(p - e) = (p - e)(1 + d1) and e' = fl(e + w s) = (e + w s)(1 + d2) -- a fused
multiply-add, one rounding -- with |d1|, |d2| <= u = 2^-24.  Against the exact x = e + w (p - e):

    e'_kernel - x = w (p - e) d1 (1 + d2) + x d2          |.| <= u |x| + u (1 + u) |w (p - e)|

An evaluation that rounds the product on its own (numpy float32, nothing fused) has one more factor (1 + d3) on w s:
<= u |x| + (2u + 3u^2) |w (p - e)|.  The bound used for both is therefore

    step(x, q) = (1 + 4u) u (|x| + 2 |q|) + 3 * 2^-149,        q = w (p - e)

the constant being 1 on |e'| and 2 on |w (p - e)|; (1 + 4u) covers the second-order terms and the float64 oracle's own
roundings (a few 2^-53), and 2^-149 per rounding replaces u |r| where a result is subnormal.

Over steps.  The kernel's next update starts from its own e, which is off by at most B: x moves by (1 - w) B, exactly, since
e + w (p - e) = (1 - w) e + w p; the magnitudes inside `step` move by at most (1 - w) B and w B.  Hence, as
tests/optimizer_cases.py carries its running bound,

    B' = (1 - w) B + step(|x| + (1 - w) B, |q| + w B),        B_0 = 0 (the EMA starts as a copy)

p is compared as a snapshot of what the device held, an exact f32 value."""
import numpy as np

U = 2.0 ** -24
F32_DENORM = 2.0 ** -149
GUARD = 64                  # sentinel elements on either side of every buffer (a multiple of 4: keeps the alignment)
SENTINEL = 777.0
WG = 1024                   # elements of one trip of a workgroup (256 threads x 4)
GRID_CAP = 2048             # csrc/ema.hip: ema_grid

DECAY = 0.9998
WRONG = ("decay_as_weight", "weight_of_previous_update", "warmup_ignored", "updates_not_advanced")


def f32(x):
    return float(np.float32(x))


def decay_at(t, decay=DECAY, warmup=True):
    """d of update t, in Python floats (f64), as the kernel's one thread computes it"""
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


def weight_at(t, decay=DECAY, warmup=True, wrong=None):
    """the f32 weight of update t as a Python float; `wrong`: one of the seeded wrong schedules"""
    if wrong == "weight_of_previous_update":
        t = max(t - 1, 0)
    if wrong == "updates_not_advanced":
        t = 0
    if wrong == "warmup_ignored":
        warmup = False
    d = decay_at(t, decay, warmup)
    return f32(d) if wrong == "decay_as_weight" else f32(1.0 - d)


def crossover(decay=DECAY):
    """the first update whose ramp (1 + t) / (10 + t) reaches `decay`: from it on d == decay"""
    t = 0
    while (1.0 + t) / (10.0 + t) < decay:
        t += 1
    return t


def lerp64(e, p, w):
    """the definition in float64 -> (x, q)"""
    e, p = np.asarray(e, dtype=np.float64), np.asarray(p, dtype=np.float64)
    with np.errstate(all="ignore"):
        q = w * (p - e)
        return e + q, q


def lerp_f32_unfused(e, p, w):
    """numpy float32, one rounding per operation, nothing fused"""
    e, p, w = np.asarray(e, dtype=np.float32), np.asarray(p, dtype=np.float32), np.float32(w)
    with np.errstate(all="ignore"):
        return e + w * (p - e)


def lerp_f32_fused(e, p, w):
    """the kernel's shape: the difference rounded to f32, then e + w s rounded once (the product of two f32 values is exact in
    float64; the float64 sum's own rounding sits 29 bits below the f32 one)"""
    e, p = np.asarray(e, dtype=np.float32), np.asarray(p, dtype=np.float32)
    with np.errstate(all="ignore"):
        s = (p - e).astype(np.float64)
        return (e.astype(np.float64) + np.float64(w) * s).astype(np.float32)


def step_bound(x, q, w, B=0.0):
    """B' of the module docstring, elementwise; non-finite entries of x give inf/nan bounds, which `ratio` never reads"""
    with np.errstate(all="ignore"):
        keep = 1.0 - w
        return keep * B + (1.0 + 4.0 * U) * U * ((np.abs(x) + keep * B) + 2.0 * (np.abs(q) + w * B)) + 3.0 * F32_DENORM


class Chain:
    """the f64 recurrence over snapshots of p with its running bound: `e`, `bound` after every `update(p)`"""

    def __init__(self, e0, decay=DECAY, warmup=True, wrong=None, t0=0):
        self.e = np.asarray(e0, dtype=np.float64).copy()
        self.bound = np.zeros_like(self.e)
        self.t, self.decay, self.warmup, self.wrong = t0, decay, warmup, wrong

    def update(self, p):
        w = weight_at(self.t, self.decay, self.warmup, self.wrong)
        x, q = lerp64(self.e, p, w)
        self.bound = step_bound(x, q, w, self.bound)
        self.e = x
        self.t += 1
        return w


def ratio(got, ref, bound):
    """worst |got - ref| / bound over the finite elements of the reference; where the reference is not finite the result must
    be the same non-finite value"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN where the definition has none, or none where it has one"
    inf = np.isinf(ref)
    assert np.array_equal(got[inf], ref[inf])
    fin = np.isfinite(ref)
    if not fin.any():
        return 0.0
    return float((np.abs(got[fin] - ref[fin]) / np.asarray(bound, dtype=np.float64)[fin]).max())


# ------------------------------------------------------------------------------------------------------------------------
# segment tables of the kernel tests
# ------------------------------------------------------------------------------------------------------------------------
class SegTable:
    """`lens` -> seg_start (nseg + 1 cumulative offsets into the EMA buffer, the C ABI's layout) and the place of every
    segment's live data in ONE live buffer: 16-byte aligned, `shift[s]` elements further for the segments named there, with
    eight sentinel elements between neighbours and GUARD on the outside.  `max_len`: what the launcher is told (None: the
    true maximum)"""

    def __init__(self, name, lens, shift=None, max_len=None):
        self.name, self.lens, shift = name, list(lens), shift or {}
        self.starts = [0]
        for n in self.lens:
            self.starts.append(self.starts[-1] + n)
        self.total = self.starts[-1]
        self.live_off, off = [], GUARD
        for s, n in enumerate(self.lens):
            self.live_off.append(off + shift.get(s, 0))
            off += (n + shift.get(s, 0) + 3) // 4 * 4 + 8
        self.live_total = off + GUARD
        self.max_len = max(self.lens, default=0) if max_len is None else max_len

    def inputs(self, seed):
        """(live buffer, EMA buffer) as float32 arrays with the sentinels in place: values over five decades, both signs,
        the EMA within a few per cent of the live value for most elements (where p - e is exact) and far away for the rest"""
        r = np.random.default_rng(seed)
        live = np.full(self.live_total, SENTINEL, dtype=np.float32)
        ema = np.full(GUARD + self.total + GUARD, SENTINEL, dtype=np.float32)
        for s, n in enumerate(self.lens):
            p = (r.standard_normal(n) * 10.0 ** r.uniform(-3, 2, n)).astype(np.float32)
            near = r.random(n) < 0.7
            e = np.where(near, p * (1.0 + 0.03 * r.standard_normal(n)), r.standard_normal(n) * 10.0 ** r.uniform(-3, 2, n))
            live[self.live_off[s]:self.live_off[s] + n] = p
            ema[GUARD + self.starts[s]:GUARD + self.starts[s] + n] = e.astype(np.float32)
        return live, ema

    def live_mask(self):
        """True where the live buffer holds a segment's data (everything else is sentinel)"""
        m = np.zeros(self.live_total, dtype=bool)
        for off, n in zip(self.live_off, self.lens):
            m[off:off + n] = True
        return m

    def gather(self, live):
        """the live data in the order of the EMA buffer"""
        return np.concatenate([live[off:off + n] for off, n in zip(self.live_off, self.lens)] + [live[:0]])


def _padded(lens):
    """`lens` with a filler segment behind every length that is no multiple of 4, so that every listed segment starts 16-byte
    aligned in the EMA buffer (solver/ema.py lays the statistics out like this)"""
    out = []
    for n in lens:
        out.append(n)
        if n % 4:
            out.append(4 - n % 4)
    return out


EDGE_LENS = [0, 1, 3, 4, 5, 1023, 1024, 1025]
# cumulative starts 0, 0, 1, 4, 8, 13, ...: aligned (4, 5: the float4 path with and without a tail) and unaligned (1023,
# 1024, 1025: the scalar path) EMA offsets
PACKED = SegTable("packed", EDGE_LENS + [0, 2 * WG + 7])
# every edge length on the float4 path with its tail; segment 10 of the padded list (length 1024) reads a live pointer 4 bytes
# off alignment and so takes the scalar path on an aligned EMA offset
ALIGNED = SegTable("aligned", _padded(EDGE_LENS), shift={_padded(EDGE_LENS).index(1024): 1})
# loop trips: 12 segments leave 2048 / 12 = 170 workgroups a segment; the long one gives each a range of 4096 elements, four
# trips, the last used workgroup a tail of 5, the workgroups behind it nothing
LOOPS = SegTable("loops", [5, 170 * 3 * WG + 2 * WG + 5] + [WG] * 10)
# the same, by telling the launcher a max_len far below the long segment: one workgroup walks it all
SHORT_GRID = SegTable("short_grid", [9 * WG + 3, 4], max_len=4)
# one segment at the capped grid: 2048 workgroups with ranges of 2048 elements, two trips each; the last ones idle or partial
CAPPED = SegTable("capped", [GRID_CAP * WG + 3 * WG + 5])
ONE = SegTable("one", [37])
TABLES = [PACKED, ALIGNED, LOOPS, SHORT_GRID, CAPPED, ONE]

# non-finite values at float4 and tail positions of a 4-aligned segment of 11 elements: (index, p, e)
NONFINITE = [(0, np.nan, 1.0), (1, 1.0, np.nan), (2, np.inf, 1.0), (3, 1.0, -np.inf), (5, np.inf, np.inf), (6, -np.inf, np.inf),
             (8, np.nan, 2.0), (9, -np.inf, 3.0), (10, 4.0, np.inf)]
NONFINITE_TABLE = SegTable("nonfinite", [11])
