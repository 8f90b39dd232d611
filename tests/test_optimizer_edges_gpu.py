"""Every instantiation of the flat optimizer-step kernels (csrc/train_ops.hip) against the float64 reference with its running
error bound (tests/optimizer_cases.py; tests/test_optimizer_edges_host.py validates both on the CPU): run tables with runs of
0 .. 8 elements and workgroup seams, a first step over a NaN momentum buffer, the capped grids, non-finite gradients, Adam at
t = 1 and where the bias correction is exactly 1, adam_advance, and the two norm kernels from 0 to 65 chunks a parameter.

Every f32 buffer is a view 64 elements into a larger allocation filled with a sentinel, which is asserted after every launch;
only tables that satisfy the launchers' contract are launched.  Tolerance per element 2 e + 2^-149 (e: the running bound);
where the definition fixes the bits -- non-finite values, lr == 0, all-zero Adam elements, the gradient buffer, a repeated
launch -- equality is asserted."""
import math

import numpy as np
import pytest
import torch

import optimizer_cases as C

pytestmark = pytest.mark.gpu


class Guarded:
    """an f32 buffer GUARD elements into a larger allocation: 16-byte aligned, sentinels on either side"""

    def __init__(self, values, dev, dtype=torch.float32):
        values = torch.as_tensor(np.asarray(values)).to(dtype)
        n = values.numel()
        self.big = torch.full((n + 2 * C.GUARD,), C.SENTINEL, dtype=dtype, device=dev)
        self.t = self.big[C.GUARD:C.GUARD + n]
        self.t.copy_(values)
        assert self.t.data_ptr() % 16 == 0

    def check(self):
        assert (self.big[:C.GUARD] == C.SENTINEL).all() and (self.big[-C.GUARD:] == C.SENTINEL).all(), "a guard element changed"

    def numpy(self):
        return self.t.cpu().numpy()


def _tables(c, dev):
    t = c.table
    return (torch.tensor(t.run_end, dtype=torch.int64, device=dev), torch.tensor(t.lr_index, dtype=torch.int32, device=dev),
            Guarded(t.wd, dev), Guarded(C.LR_TABLE, dev))


def _advance(t_before, dev):
    import detectron2_centernet_amd.ops as ops
    step = torch.tensor([t_before], dtype=torch.int64, device=dev)
    bias = Guarded([0.0, 0.0], dev)
    ops.adam_advance_(step, bias.t, *C.BETAS)
    bias.check()
    return int(step.item()), bias


def launch(c, dev):
    """one launch of the case's kernel; returns ({name: f32 array}, bias read back or None)"""
    import detectron2_centernet_amd.ops as ops
    d = c.inputs()
    buf = {k: Guarded(d[k], dev) for k in ("p", "g", "m")}
    guards = list(buf.values())
    bias = None
    if c.kind == "sgd":
        lr = Guarded([C.LR_TABLE[0]], dev)
        guards.append(lr)
        ops.sgd_momentum_(buf["p"].t, buf["g"].t, buf["m"].t, lr.t, C.MOMENTUM, C.WEIGHT_DECAY, c.first)
    else:
        run_end, lr_index, wd, lrs = _tables(c, dev)
        coefs = Guarded(d["coefs"], dev) if d["coefs"] is not None else None
        guards += [wd, lrs] + ([coefs] if coefs else [])
        ct = coefs.t if coefs else None
        if c.kind == "sgd_runs":
            ops.sgd_momentum_runs_(buf["p"].t, buf["g"].t, buf["m"].t, run_end, lr_index, wd.t, lrs.t, C.MOMENTUM, c.first)
        elif c.kind == "sgd_clip":
            ops.sgd_momentum_runs_clip_(buf["p"].t, buf["g"].t, buf["m"].t, run_end, lr_index, wd.t, lrs.t, C.MOMENTUM, c.first,
                                        nesterov=c.nest, clip_type=c.clip, clip_value=c.clip_value, coefs=ct)
        else:
            buf["v"] = Guarded(d["v"], dev)
            guards.append(buf["v"])
            if c.amsgrad:
                buf["x"] = Guarded(d["x"], dev)
                guards.append(buf["x"])
            t, bg = _advance(c.t - 1, dev)
            assert t == c.t
            guards.append(bg)
            bias = tuple(float(b) for b in bg.numpy())
            ops.adam_runs_(buf["p"].t, buf["g"].t, buf["m"].t, buf["v"].t, buf["x"].t if c.amsgrad else None, run_end, lr_index,
                           wd.t, lrs.t, bg.t, C.BETAS[0], C.BETAS[1], C.EPS, decoupled=c.decoupled, amsgrad=c.amsgrad,
                           clip_type=c.clip, clip_value=c.clip_value, coefs=ct)
    torch.cuda.synchronize()
    for g in guards:
        g.check()
    got = {k: b.numpy() for k, b in buf.items()}
    assert np.array_equal(got["g"].view(np.uint32), d["g"].view(np.uint32)), "the gradient buffer is only read"
    return got, bias


def _check(c, dev, worst):
    got, bias = launch(c, dev)
    ref = c.evaluate(bias=bias)
    rs = {k: C.ratio(got[k], ref[k]) for k in ref}
    worst[c.name] = max(rs.values())
    assert max(rs.values()) < 1.0, (c.name, rs)
    keep = c.exact_unchanged()
    assert np.array_equal(got["p"][keep].view(np.uint32), c.inputs()["p"][keep].view(np.uint32)), (c.name, "lr == 0")
    return got, ref


def _report(title, worst):
    by = {}
    for name, r in worst.items():
        by.setdefault(name.split("-")[0], []).append((r, name))
    for name, r in worst.items():
        print(f"  {name:44s} {r:.3f}")
    for kind, rs in sorted(by.items()):
        print(f"{title} {kind:9s} worst error / tolerance {max(rs)[0]:.3f} ({max(rs)[1]}), {len(rs)} cases")


def test_update_kernels_on_run_tables(dev):
    """1 + 1 + 5 + 12 instantiations over the 12 k table (runs of 0 .. 8 elements, ends at 1023 / 1024 / 1025, a run over
    three workgroups, three learning rates one of them 0) and over tables of 1 and 3 elements"""
    worst = {}
    for c in C.update_cases():
        _check(c, dev, worst)
    _report("run tables", worst)
    assert any(c.exact_unchanged().sum() > 4000 for c in C.update_cases())      # the lr == 0 runs were there


def test_first_step_ignores_the_momentum_buffer(dev):
    """first = 1 over a momentum buffer full of NaN: finite, and the reference with buf = g'"""
    worst = {}
    for c in C.first_step_cases():
        got, _ = _check(c, dev, worst)
        assert np.isfinite(got["p"]).all() and np.isfinite(got["m"]).all()
    _report("first step", worst)


def test_capped_grids(dev):
    """more elements than the grid cap times one trip: the run kernels' `per` is 2048, sgd_kernel's grid-stride loop wraps"""
    worst = {}
    for c in C.capped_cases():
        _check(c, dev, worst)
    _report("capped grid", worst)


def test_nonfinite_gradients(dev):
    """value clipping leaves NaN and clamps +-inf; the neighbours are untouched; AMSGrad keeps a NaN of v or vmax"""
    worst = {}
    for c in C.nonfinite_cases():
        got, ref = _check(c, dev, worst)                                        # C.ratio: the same NaNs, exactly
        for i, val in C.NONFINITE_G.items():
            assert np.isnan(got["p"][i]) == math.isnan(val) and np.isnan(got["m"][i]) == math.isnan(val)
        if c.kind == "adam":
            for i in list(C.NONFINITE_V) + list(C.NONFINITE_X):
                assert np.isnan(got["x"][i]) and np.isnan(got["p"][i])
    _report("non-finite", worst)


def test_adam_edges(dev):
    """t = 1 and the bias of t = 10^6; g = m = v = 0 (exact); v tiny against eps^2; vmax above, below and equal to the new v"""
    worst = {}
    for c in C.adam_edge_cases():
        got, _ = _check(c, dev, worst)
        for z in C.zero_slices():
            want = c.zero_expected(z)
            if want is not None:
                assert np.array_equal(got["p"][z].view(np.uint32), want.view(np.uint32)), c.name
                assert not got["m"][z].any() and not got["v"][z].any()
    _report("adam edges", worst)


@pytest.mark.parametrize("t0", [0, 1, 9, 10 ** 6, 2 ** 31])
def test_adam_advance(dev, t0):
    t, bias = _advance(t0, dev)
    assert t == t0 + 1
    b = bias.numpy().astype(np.float64)
    want = (1.0 / (1.0 - C.BETAS[0] ** t), 1.0 / math.sqrt(1.0 - C.BETAS[1] ** t))
    for got, w in zip(b, want):
        assert abs(got - w) <= 2.0 ** -23 * w, (t, got, w)                      # one f32 rounding plus libm
    if t0 >= 10 ** 6:
        assert b[0] == 1.0 and b[1] == 1.0


# ------------------------------------------------------------------------------------------------------------------------
# the norm kernels
# ------------------------------------------------------------------------------------------------------------------------
class NormTables:
    def __init__(self, dev):
        from detectron2_centernet_amd.solver.build import grad_chunks
        self.offsets = C.norm_offsets()
        self.starts, self.lens, self.ends = grad_chunks(self.offsets)
        self.d_starts = torch.tensor(self.starts, dtype=torch.int64, device=dev)
        self.d_lens = torch.tensor(self.lens, dtype=torch.int32, device=dev)
        self.d_ends = torch.tensor(self.ends, dtype=torch.int32, device=dev)
        self.dev = dev

    def run(self, g, norm_type, clip_value):
        import detectron2_centernet_amd.ops as ops
        gg = Guarded(g, self.dev)
        part = Guarded(np.full(len(self.starts), np.nan), self.dev)
        norms = Guarded(np.full(len(self.ends), np.nan), self.dev)
        coefs = Guarded(np.full(len(self.ends), np.nan), self.dev)
        ops.grad_chunk_norms_(gg.t, self.d_starts, self.d_lens, norm_type, part.t)
        ops.grad_clip_coefs_(part.t, self.d_ends, norm_type, clip_value, norms.t, coefs.t)
        torch.cuda.synchronize()
        for b in (gg, part, norms, coefs):
            b.check()
        assert np.array_equal(gg.numpy().view(np.uint32), np.asarray(g, np.float32).view(np.uint32))
        return part.numpy(), norms.numpy(), coefs.numpy()


@pytest.fixture(scope="module")
def norm_tables(dev):
    return NormTables(dev)


@pytest.mark.parametrize("norm_type", C.NORM_TYPES)
def test_norm_kernels_random(norm_tables, norm_type):
    """partials within 2 D u sum |term| of float64 (D: the depth of the kernel's summation shape), norms and coefficients
    within the running bound from the partials the first kernel wrote; a parameter without a chunk has norm 0; two launches
    give the same bits"""
    T = norm_tables
    rng = np.random.default_rng(710 + norm_type)
    g = (rng.standard_normal(C.norm_total()) * 10.0 ** rng.uniform(-3, 1, C.norm_total())).astype(np.float32)
    part, norms, coefs = T.run(g, norm_type, C.CLIP_NORM_AT)
    r_part = C.ratio(part, C.chunk_partials_ref(g, T.starts, T.lens, norm_type))
    nref, cref = C.coefs_ref(part, T.ends, norm_type, C.CLIP_NORM_AT)
    r_norm, r_coef = C.ratio(norms, nref), C.ratio(coefs, cref)
    print(f"norm type {norm_type}: partials {r_part:.3f}, norms {r_norm:.3f}, coefs {r_coef:.3f} of the tolerance")
    assert r_part < 1.0 and r_norm < 1.0 and r_coef < 1.0
    assert (coefs == 1.0).any() and (coefs < 1.0).any() and (coefs <= 1.0).all()
    for q, (off, n) in enumerate(T.offsets):
        if n == 0:
            assert norms[q] == 0.0 and coefs[q] == 1.0
        else:                                                                   # end to end against float64 of the elements
            want = np.linalg.norm(g[off:off + n].astype(np.float64), {C.NORM_L1: 1, C.NORM_L2: 2, C.NORM_INF: np.inf}[norm_type])
            assert abs(norms[q] - want) <= 2 * (C.CHUNK_DEPTH + 1 + C.coef_depth(65) + 2) * C.U * want, (q, norms[q], want)
    again = T.run(g, norm_type, C.CLIP_NORM_AT)
    for a, b in zip((part, norms, coefs), again):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("norm_type", C.NORM_TYPES)
def test_norm_kernels_one_hot(norm_tables, norm_type):
    """a single non-zero element per parameter, at the first and last element of the parameter and of its chunks (every
    residue mod 4 among them) and in the 65th chunk: a dropped or double-counted element is a 100 % error.  The values are
    small integers, so every norm is exact."""
    T = norm_tables
    places = {"first": lambda n: 0, "last": lambda n: n - 1, "end of chunk 0": lambda n: min(n, C.GRAD_CHUNK) - 1,
              "start of chunk 1": lambda n: min(n - 1, C.GRAD_CHUNK), "end of chunk 63": lambda n: min(n, 64 * C.GRAD_CHUNK) - 1,
              "lane 63's share": lambda n: min(n - 1, 63 * 4 + 2)}
    for name, place in places.items():
        g = np.zeros(C.norm_total(), dtype=np.float32)
        want = np.zeros(len(T.offsets))
        for q, (off, n) in enumerate(T.offsets):
            if n:
                g[off + place(n)] = -(q + 2.0)
                want[q] = q + 2.0
        _, norms, coefs = T.run(g, norm_type, 1.0)
        assert np.array_equal(norms.astype(np.float64), want), (name, norms, want)
        c64 = np.minimum(1.0, 1.0 / (want + C.f32(1e-6)))
        assert (np.abs(coefs - c64) <= 4 * C.U * c64).all() and (coefs[want == 0] == 1.0).all(), (name, coefs)
    last = T.offsets[-2]
    assert last[1] == 64 * C.GRAD_CHUNK + 1 and len(T.starts) - T.ends[-3] == 65          # "last" sat alone in the 65th chunk


@pytest.mark.parametrize("norm_type", [C.NORM_L2, C.NORM_INF])
def test_norm_kernels_nan(norm_tables, norm_type):
    """a NaN gives its parameter a NaN norm and a NaN coefficient wherever it sits -- first or last element of a chunk, lane 0
    or lane 63's share -- and leaves the neighbours finite"""
    T = norm_tables
    rng = np.random.default_rng(720)
    base = rng.standard_normal(C.norm_total()).astype(np.float32)
    q = C.NORM_PARAM_LENGTHS.index(4097)
    off, n = T.offsets[q]
    for at in (0, 1, 63 * 4 + 1, 255 * 4 + 3, C.GRAD_CHUNK - 1, C.GRAD_CHUNK):
        g = base.copy()
        g[off + at] = np.nan
        part, norms, coefs = T.run(g, norm_type, C.CLIP_NORM_AT)
        assert np.isnan(norms[q]) and np.isnan(coefs[q]), (at, norms[q], coefs[q])
        others = np.arange(len(norms)) != q
        assert np.isfinite(norms[others]).all() and np.isfinite(coefs[others]).all(), at
        assert np.isnan(part).sum() == 1


def test_norm_kernels_zero(norm_tables):
    """an all-zero gradient: norm 0 and coefficient exactly 1; with a clip value below 1e-6, clip / 1e-6 inside its bound"""
    T = norm_tables
    g = np.zeros(C.norm_total(), dtype=np.float32)
    for norm_type in C.NORM_TYPES:
        part, norms, coefs = T.run(g, norm_type, 1.0)
        assert not part.any() and not norms.any() and (coefs == 1.0).all()
        part, norms, coefs = T.run(g, norm_type, 5e-7)
        nref, cref = C.coefs_ref(part, T.ends, norm_type, 5e-7)
        assert not norms.any() and C.ratio(coefs, cref) < 1.0 and (np.abs(coefs - 0.5) < 1e-6).all()
