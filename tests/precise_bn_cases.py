"""PreciseBN (csrc/precise_bn.hip): a float64 restatement of ctdet_precise_bn_merge_segments / _finish_segments, the error
bound the tests hold the kernels to, and the case tables.  numpy only.

THE STEP.  The state of a channel is (n, mu, M2): row count, mean, sum of squared deviations.  A block of M rows with mean m
and sum of squared deviations M2_b is folded in by Chan's formula

    n' = n + M,  w = M / n',  d = m - mu,  mu' = mu + d w,  M2' = M2 + (M2_b + d d (n w))

and a channel with n = 0 takes (M, m, M2_b) as they are.  MERGE feeds it a batch: m = running_mean, M2_b = u (M - 1) with
u = running_var, the unbiased batch variance.  FINISH feeds it the rank slots in rank order (a slot with n = 0 is skipped)
and writes mean = f32(mu), var = f32(M2 / n).

THE BOUND.  e = 2^-53 is the unit roundoff of f64, g(k) = k e / (1 - k e) bounds the product of k factors (1 + t), |t| <= e
(Higham, Accuracy and Stability, lemma 3.1); g(a) (1 + g(b)) <= g(a + b).  Hats are computed values, emu / eM2 the running
bounds of |mu^ - mu| and |M2^ - M2| against the exact recurrence on the same inputs.  n, M and n' are integers below 2^53:
exact.  An fma may contract a product into the following sum, which removes a rounding and never adds one: the counts below
are upper bounds for either code.  Inputs may carry errors of their own: em on m, eM2b on M2_b (zero for the kernels' inputs,
which are what they are; an f32 rounding in the host test that starts from rows; the slots' own bounds in finish).

  M2_b^ = fl(u (M - 1))                   one rounding:  eM2b = g(1) M2_b^                  (M - 1 is exact)
  w^ = fl(M / n')                         one rounding
  d^ = fl(m - mu^) = D (1 + t),           D = m - mu^   (D is off the true d by at most ed = emu + em)
  mu'^ = fl(mu^ + fl(d^ w^)) = (mu^ + D w (1 + t)^3) (1 + t)
      against mu^ + D w:                  g(3) |D| w + g(1) |mu'^|  <=  g(5) |d^| w^ + g(1) |mu'^|
      mu^ + D w = mu^ (1 - w) + m w  against the true mu (1 - w) + m w:   emu (1 - w) + em w
        emu' = emu n / n' + em w^ + g(5) |d^| w^ + g(1) |mu'^|
      (the inherited error SHRINKS by n / n': this is why the chain's bound grows linearly, not like 2^steps)
  T^ = fl(fl(d^ d^) fl(n w^)) = D^2 n w (1 + t)^6        against D^2 n w:  g(6) D^2 n w <= g(8) T^
  M2'^ = fl(M2^ + fl(M2_b^ + T^))         two roundings of sums of non-negative terms:  <= g(3) M2'^
      D^2 against d^2:                    |D^2 - d^2| <= ed (2 |D| + ed)
        eM2' = eM2 + eM2b + (1 + g(3)) ed (2 |d^| + ed) n w^ + g(8) T^ + g(3) M2'^
  n = 0:  mu' = m, M2' = M2_b^ bit for bit:  emu' = em, eM2' = eM2b.

  finish:  v^ = fl(M2^ / n): eM2 / n + g(1) v^;  the stores round to f32: 2^-24 relative (2^-150 absolute below the normal
  range).  The bound is itself evaluated in f64; every g(k) above counts at least one rounding more than occurs, which covers
  its own rounding.

Two computations that both obey the bound -- the kernel and this restatement -- differ by at most TWICE the f64 part."""
import numpy as np

EPS = 2.0 ** -53
F32 = 2.0 ** -24
F32_TINY = 2.0 ** -150
GUARD = 16
SENTINEL = -7.25          # exactly representable; a variance is never negative and no mean below is -7.25


def g(k):
    return k * EPS / (1.0 - k * EPS)


class Acc:
    """the state of `total` channels with its running bounds"""

    def __init__(self, total):
        self.n, self.mu, self.m2 = (np.zeros(total) for _ in range(3))
        self.emu, self.em2 = np.zeros(total), np.zeros(total)

    def state(self):
        return np.stack([self.n, self.mu, self.m2])

    def step(self, M, m, m2b, em=0.0, em2b=0.0):
        """one Chan step on every channel; M (integers as f64), m, m2b and the input errors broadcast over the channels.
        Channels with M == 0 are left alone (finish skips an empty slot)."""
        total = self.n.size
        M, m, m2b, em, em2b = (np.broadcast_to(np.asarray(a, dtype=np.float64), (total,)) for a in (M, m, m2b, em, em2b))
        n, mu, m2, emu, em2 = self.n, self.mu, self.m2, self.emu, self.em2
        live = M > 0
        fresh = live & (n == 0)
        go = live & ~fresh
        with np.errstate(invalid="ignore", divide="ignore"):
            nt = n + M
            w = M / nt
            d = m - mu
            mu1 = mu + d * w
            T = (d * d) * (n * w)
            m21 = m2 + (m2b + T)
            ed = emu + em
            emu1 = emu * (n / nt) + em * w + g(5) * np.abs(d) * w + g(1) * np.abs(mu1)
            em21 = em2 + em2b + (1 + g(3)) * ed * (2 * np.abs(d) + ed) * n * w + g(8) * T + g(3) * m21
        self.n = np.where(live, nt, n)
        self.mu = np.where(fresh, m, np.where(go, mu1, mu))
        self.m2 = np.where(fresh, m2b, np.where(go, m21, m2))
        self.emu = np.where(fresh, em, np.where(go, emu1, emu))
        self.em2 = np.where(fresh, em2b, np.where(go, em21, em2))

    def merge(self, M, m, u, em=0.0, eu=0.0):
        """what ctdet_precise_bn_merge_segments does with a batch: m, u the f32 running_mean / running_var (as f64), M the
        per-channel row count; em / eu: errors the inputs carry against what they stand for"""
        M = np.asarray(M, dtype=np.float64)
        m2b = np.asarray(u, dtype=np.float64) * (M - 1.0)
        self.step(M, np.asarray(m, dtype=np.float64), m2b, em, g(1) * m2b + np.asarray(eu, dtype=np.float64) * (M - 1.0))

    def outputs(self):
        """(mean, var) in f64 before the f32 store, their bounds against the exact values AFTER the store (f64 part, f32
        part), and the mask of channels that are written at all (n > 0)"""
        has = self.n > 0
        with np.errstate(invalid="ignore", divide="ignore"):
            v = np.where(has, self.m2 / self.n, 0.0)
            ev = np.where(has, self.em2 / self.n, 0.0) + g(1) * v
        return (self.mu, v), (self.emu, ev), has


def finish64(slots):
    """slots [world][3][total] (f64) -> the Acc after combining them in rank order; the slots are exact inputs"""
    world, _, total = slots.shape
    acc = Acc(total)
    for r in range(world):
        acc.step(slots[r, 0], slots[r, 1], slots[r, 2])
    return acc


def f32_part(x):
    return F32 * np.abs(x) + F32_TINY


def ratio(got, want, bound):
    """max |got - want| / bound; 0 where both the error and the bound are 0, inf where only the bound is"""
    got, want, bound = (np.asarray(a, dtype=np.float64).ravel() for a in (got, want, bound))
    if got.size == 0:
        return 0.0
    err = np.abs(got - want)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err == 0, 0.0, np.where(bound > 0, err / bound, np.inf))
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max())


# ------------------------------------------------------------------------------------------------------------------------
# the tables: segment lengths, and max_len as the caller passes it (it only sizes the grid)
# ------------------------------------------------------------------------------------------------------------------------
class Table:
    def __init__(self, name, lens, max_len=None):
        self.name, self.lens = name, list(lens)
        self.starts = [0] + list(np.cumsum(self.lens, dtype=np.int64)) if self.lens else [0]
        self.starts = [int(s) for s in self.starts]
        self.total = self.starts[-1]
        self.max_len = max(self.lens, default=0) if max_len is None else max_len
        # the live f32 buffer: per segment GUARD | mean | GUARD | var, and a last GUARD
        self.mean_off, self.var_off, off = [], [], 0
        for n in self.lens:
            self.mean_off.append(off + GUARD)
            self.var_off.append(off + 2 * GUARD + n)
            off += 2 * GUARD + 2 * n
        self.live_size = off + GUARD

    def seg_of(self):
        """channel -> segment"""
        return np.repeat(np.arange(len(self.lens)), self.lens)

    def live(self, m, u):
        """the live buffer holding the per-channel m and u (f32), sentinels elsewhere"""
        buf = np.full(self.live_size, SENTINEL, dtype=np.float32)
        for s, n in enumerate(self.lens):
            a, b = self.starts[s], self.starts[s + 1]
            buf[self.mean_off[s]:self.mean_off[s] + n] = m[a:b]
            buf[self.var_off[s]:self.var_off[s] + n] = u[a:b]
        return buf

    def gather(self, buf):
        m, u = np.empty(self.total, dtype=np.float32), np.empty(self.total, dtype=np.float32)
        for s, n in enumerate(self.lens):
            a, b = self.starts[s], self.starts[s + 1]
            m[a:b] = buf[self.mean_off[s]:self.mean_off[s] + n]
            u[a:b] = buf[self.var_off[s]:self.var_off[s] + n]
        return m, u

    def guards_intact(self, buf):
        mask = np.ones(self.live_size, dtype=bool)
        for s, n in enumerate(self.lens):
            mask[self.mean_off[s]:self.mean_off[s] + n] = False
            mask[self.var_off[s]:self.var_off[s] + n] = False
        return bool((buf[mask] == SENTINEL).all())


# every length the issue names: 1, 3, 4, 5, an empty segment in the middle, 64, 65 (one past a wave), 257 (one past a workgroup)
EDGES = Table("edges", [1, 3, 4, 5, 0, 64, 65, 257])
# max_len below the longest segment: the grid is sized for 256 channels and the workgroup of segment 0 loops three times
SHORT_GRID = Table("short-grid", [600, 7], max_len=256)
# past the cap of 64 workgroups per segment (16384 channels): every workgroup of the segment loops
CAPPED = Table("capped", [64 * 256 + 5, 2])
EMPTY = Table("no-segments", [])
TABLES = [EDGES, SHORT_GRID, CAPPED]

# chains of 1, 2 and 7 merges: the row count of (merge k, segment s) -- different per segment and per merge, with M = 2 (the
# smallest a batch statistic exists for) and M around 4e6 (16 x 512 x 512 rows: the stem of a full-size batch)
BIG = 4 * 10 ** 6 + 3
CHAINS = [1, 2, 7]


def rows_of(k, nseg):
    """row counts of merge k for nseg segments"""
    base = [2, BIG, 96, 6, 1024, 2, 4099, 33]
    return [int(base[(s + 3 * k) % len(base)] + (k if base[(s + 3 * k) % len(base)] > 2 else 0)) for s in range(nseg)]


REGIMES = ["unit", "cancel", "zero-var", "alt-sign"]


def batch_stats(regime, k, total, seed):
    """(m, u) of merge k as f32 arrays: what the live buffers hold"""
    rng = np.random.default_rng([seed, k, REGIMES.index(regime)])
    if regime == "unit":
        m, u = rng.standard_normal(total), rng.uniform(0.5, 1.5, total)
    elif regime == "cancel":        # mean 1e3, variance 1e-6: M2 is tiny next to n mu^2, a sum-of-squares form would lose it all
        m, u = 1e3 + 1e-3 * rng.standard_normal(total), 1e-6 * rng.uniform(0.5, 1.5, total)
    elif regime == "zero-var":      # the same constant in every batch: the variance must come out 0
        m, u = np.random.default_rng([seed, 99]).standard_normal(total), np.zeros(total)
    else:                           # means of alternating sign, per channel and per merge
        sign = np.where((np.arange(total) + k) % 2 == 0, 1.0, -1.0)
        m, u = sign * rng.uniform(1.0, 2.0, total), rng.uniform(0.5, 1.5, total)
    return m.astype(np.float32), u.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------
# seeded wrong formulas (tests/test_precise_bn_host.py holds the bound against them)
# ------------------------------------------------------------------------------------------------------------------------
def wrong_chain(kind, batches):
    """batches: [(M, m, u)] per-channel arrays -> (mean, population variance) by a formula with one seeded mistake"""
    n = mu = m2 = None
    means = []
    for M, m, u in batches:
        M, m, u = (np.asarray(a, dtype=np.float64) for a in (M, m, u))
        m2b = u * M if kind == "biased-u" else u * (M - 1.0)
        means.append(m)
        if n is None:
            n, mu, m2 = M.copy(), m.copy(), m2b.copy()
            continue
        nt = n + M
        d = m - mu
        mu = mu + d * M / nt
        m2 = m2 + m2b + (d * d if kind == "no-weight" else d * d * n * M / nt)
        n = nt
    if kind == "mean-of-means":
        mu = np.mean(means, axis=0)
    return mu, m2 / n
