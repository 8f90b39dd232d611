"""The BatchNorm training kernels -- fused (bn_train_fwd / bn_train_bwd) and split around the SyncBN collectives (bn_local_stats /
bn_sync_fwd / bn_local_grad_sums / bn_sync_bwd), f16 and f32 -- against the float64 references of bn_cases.py at its edge cases,
under its per-element bounds.  Every kernel call is made twice and the second result must be bit-identical (the kernels claim
determinism); every test prints its err / bound before it asserts and the module prints the worst per path and dtype when it ends
(run with -s).  In a strided case every tensor is a channel slice of its own wider sentinel-filled buffer, all pixel strides differ,
and everything outside a written slice -- the sentinel rows behind the last row included -- must come back bit-identical."""
import pytest
import torch

import bn_cases as T

pytestmark = pytest.mark.gpu

F16, F32 = T.F16, T.F32
WORST = {}


@pytest.fixture(scope="module")
def ot():
    import detectron2_centernet_amd.ops_train as ot

    return ot


@pytest.fixture(scope="module", autouse=True)
def _worst_table():
    yield
    for (kernel, dt), r in sorted(WORST.items()):
        print(f"worst err / bound  {kernel:<34}{dt}  {r:.3f}")


def _check(path, dt, got, ref, b):
    r = T.ratio(got.cpu().reshape(ref.shape), ref, b)
    key = (path, T.dt_name(dt))
    WORST[key] = max(WORST.get(key, 0.0), r)
    print(f"{path} {T.dt_name(dt)}: err / bound {r:.3f}")
    assert r <= 1, (path, T.dt_name(dt), r)


def _int(dt):
    return torch.int16 if dt == F16 else torch.int32


def _bits(t):
    return t.view(_int(t.dtype)).cpu()


class Op:
    """one tensor operand on the device, as the kernels see it ([1, 1, M, C]): dense, or the channel slice of its own buffer"""

    def __init__(self, t, name, dt, dev, strided, output=False):
        if strided:
            buf, _ = T.slab(t, name, dt, fill=not output)
            self.buf = buf.to(dev)
            off = T.offset_of(name, dt)
            self.view = self.buf[:t.shape[0], off:off + t.shape[1]].unsqueeze(0).unsqueeze(0)
            self.before = _bits(self.buf)
        else:
            self.buf = None
            self.view = (torch.empty(t.shape, dtype=dt, device=dev) if output else t.to(dev)).view(1, 1, *t.shape)
        self.off, self.C, self.M = (T.offset_of(name, dt) if strided else 0), t.shape[1], t.shape[0]

    def untouched(self):
        if self.buf is not None:
            assert torch.equal(_bits(self.buf), self.before), "an input buffer was written"

    def only_slice_written(self):
        if self.buf is not None:
            b, s = _bits(self.buf), T.SENTINEL[self.buf.dtype]
            assert bool((b[:, :self.off] == s).all()) and bool((b[:, self.off + self.C:] == s).all()), "written outside the slice"
            assert bool((b[self.M:] == s).all()), "written behind the last row"


def _rows(op_or_t, lo, n):
    t = op_or_t.view if isinstance(op_or_t, Op) else op_or_t
    return t[:, :, lo:lo + n]


def _same(a, b):
    """bit-identical tuples of tensors / None"""
    for x, y in zip(a, b):
        if x is None or y is None:
            assert x is None and y is None
        elif x.dtype.is_floating_point and x.dtype != torch.float64:
            assert torch.equal(_bits(x.contiguous()), _bits(y.contiguous())), "second run differs"
        else:
            assert torch.equal(x, y), "second run differs"


def _twice(fn):
    """fn() -> tuple of tensors; run twice, the second result bit-identical; returns the first"""
    a = fn()
    a = tuple(None if t is None else t.clone() for t in a)
    _same(a, fn())
    return a


def _operands(case, dt, dev):
    inp = T.bn_inputs(case, dt)
    ops = {k: Op(inp[k], k, dt, dev, case.strided) for k in ("y", "dz", "zin")}
    ops["res"] = Op(inp["res"], "res", dt, dev, case.strided) if case.res else None
    for k in ("z", "dy", "dres"):
        ops[k] = Op(inp["y"], k, dt, dev, case.strided, output=True)
    par = {k: inp[k].to(dev) for k in ("gamma", "beta", "rm0", "rv0")}
    return inp, ops, par


def _into(case, C, dev):
    """the (dgamma, dbeta) slots the case asks for and the tuple to hand to the wrapper"""
    slots = [torch.full((C,), 7.0, device=dev) if (case.into == "both" or (case.into == "dgamma" and i == 0)) else None for i in range(2)]
    return slots, (None if case.into == "none" else tuple(slots))


def _check_into(slots, dgamma, dbeta):
    for s, t in zip(slots, (dgamma, dbeta)):
        if s is not None:
            assert t.data_ptr() == s.data_ptr(), "the gradient did not land in the caller's slot"


# ------------------------------------------------------------------------------------------------------------- fused
@pytest.mark.parametrize("dt", T.DTYPES, ids=T.dt_name)
@pytest.mark.parametrize("case", T.BN_CASES, ids=T.bn_id)
def test_fused_forward(ot, dev, case, dt):
    inp, ops, par = _operands(case, dt, dev)
    ref, b = T.fwd_reference(case, dt), T.fwd_bounds(case, dt, [case.M])

    def run():
        rm, rv = par["rm0"].clone(), par["rv0"].clone()
        z, mean, invstd, scale = ot.bn_train_fwd(ops["y"].view, par["gamma"], par["beta"], rm, rv, case.eps, case.momentum,
                                                 res=ops["res"].view if case.res else None, relu=case.relu, out=ops["z"].view)
        return z, mean, invstd, scale, rm, rv

    z, mean, invstd, scale, rm, rv = _twice(run)
    ops["z"].only_slice_written()
    for k in ("y", "res"):
        if ops[k] is not None:
            ops[k].untouched()
    kern = "affine_act_rows" if T.is_pow2(case.CV) else "affine_act"
    for name, got in (("mean", mean), ("invstd", invstd), ("scale", scale), ("rm", rm), ("rv", rv)):
        _check(f"chan_reduce+finalize m0 {name}", dt, got, ref[name], b[name])
    _check(f"{kern} z", dt, z, ref["z"], b["z"])


@pytest.mark.parametrize("dt", T.DTYPES, ids=T.dt_name)
@pytest.mark.parametrize("case", T.BN_CASES, ids=T.bn_id)
def test_fused_backward(ot, dev, case, dt):
    inp, ops, par = _operands(case, dt, dev)
    ref, b = T.bwd_reference(case, dt), T.bwd_bounds(case, dt, [case.M])
    (dbeta_ref, dgamma_ref), (b_dbeta, b_dgamma) = T.local_sums(case, dt, [case.M])[0], b["local"][0]
    mean, invstd, scale = (t.to(dev) for t in T.stats_in(case, dt))
    slots, into = _into(case, inp["y"].shape[1], dev)

    def run():
        dy, dres, dgamma, dbeta = ot.bn_train_bwd(ops["dz"].view, ops["zin"].view, ops["y"].view, mean, invstd, scale, relu=case.relu,
                                                  want_dres=True, grad_mult=case.grad_mult, into=into,
                                                  out=(ops["dy"].view, ops["dres"].view))
        _check_into(slots, dgamma, dbeta)
        return dy, dres, dgamma, dbeta

    dy, dres, dgamma, dbeta = _twice(run)
    ops["dy"].only_slice_written(), ops["dres"].only_slice_written()
    for k in ("y", "dz", "zin"):
        ops[k].untouched()
    assert torch.equal(dres.cpu().reshape(ref["g"].shape), ref["g"])
    kern = "bn_bwd_apply_rows" if T.is_pow2(case.CV) else "bn_bwd_apply"
    _check("chan_reduce+finalize m1 dbeta", dt, dbeta, dbeta_ref, b_dbeta)
    _check("chan_reduce+finalize m1 dgamma", dt, dgamma, dgamma_ref, b_dgamma)
    _check(f"{kern} dy", dt, dy, ref["dy"], b["dy"])


@pytest.mark.parametrize("dt", T.DTYPES, ids=T.dt_name)
@pytest.mark.parametrize("case", T.NOSTAT_CASES, ids=T.bn_id)
def test_fused_backward_without_statistics(ot, dev, case, dt):
    """y = None: dy = g bit for bit, dbeta = grad_mult * sum g, dgamma = 0; z = None too where there is no ReLU"""
    inp, ref = T.nostat_inputs(case, dt), T.nostat_reference(case, dt)
    dz, zin = Op(inp["dz"], "dz", dt, dev, case.strided), Op(inp["zin"], "zin", dt, dev, case.strided)
    out = Op(inp["dz"], "dy", dt, dev, case.strided, output=True)

    def run():
        dy, dres, dgamma, dbeta = ot.bn_train_bwd(dz.view, zin.view if case.relu else None, None, None, None, None, relu=case.relu,
                                                  grad_mult=case.grad_mult, out=(out.view, None))
        assert dres is None
        return dy, dgamma, dbeta

    dy, dgamma, dbeta = _twice(run)
    out.only_slice_written(), dz.untouched(), zin.untouched()
    assert torch.equal(dy.cpu().reshape(ref["dy"].shape), ref["dy"])
    assert torch.count_nonzero(dgamma).item() == 0
    _check("chan_reduce+finalize m1 dbias (y=None)", dt, dbeta, ref["dbeta"], ref["b_dbeta"])


# ------------------------------------------------------------------------------------------------------------- split
def _local_stats(ot, ops, parts, world, slot_of=None):
    """the gathered forward buffer: every live rank's slots summed on the device (the all-reduce)"""
    total, lo = None, 0
    for r, Mr in enumerate(parts):
        if Mr == 0:
            continue
        slot = r if slot_of is None else slot_of[r]
        (one,) = _twice(lambda: (ot.bn_local_stats(_rows(ops["y"], lo, Mr), slot, world),))
        assert one[slot, 0].eq(Mr).all(), "row count of the slot"
        assert torch.count_nonzero(torch.cat([one[q] for q in range(world) if q != slot] or [one[:0]])).item() == 0, "foreign slots"
        total = one if total is None else total + one
        lo += Mr
    return total


def _split_run(ot, dev, case, dt, parts, world, slot_of=None, check=True, poison=None):
    """the whole split pipeline over simulated ranks of `parts` rows; returns per-rank outputs for comparisons"""
    inp, ops, par = _operands(case, dt, dev)
    C = inp["y"].shape[1]
    stats = _local_stats(ot, ops, parts, world, slot_of)
    if poison is not None:
        assert stats[poison, 0].eq(0).all()
        stats[poison, 1:] = float("nan")
    fref, fb = T.fwd_reference(case, dt), T.fwd_bounds(case, dt, parts)
    bref, bb = T.bwd_reference(case, dt), T.bwd_bounds(case, dt, parts)
    lrefs = T.local_sums(case, dt, parts)
    mean_in, invstd_in, scale_in = (t.to(dev) for t in T.stats_in(case, dt))
    outs, gsum, lo = [], None, 0
    for r, Mr in enumerate(parts):
        if Mr == 0:
            continue
        slot = r if slot_of is None else slot_of[r]
        sl = slice(lo, lo + Mr)

        def fwd():
            rm, rv = par["rm0"].clone(), par["rv0"].clone()
            z, mean, invstd, scale = ot.bn_sync_fwd(_rows(ops["y"], lo, Mr), stats, par["gamma"], par["beta"], rm, rv, case.eps,
                                                    case.momentum, res=_rows(ops["res"], lo, Mr) if case.res else None,
                                                    relu=case.relu, out=_rows(ops["z"], lo, Mr))
            return z, mean, invstd, scale, rm, rv

        z, mean, invstd, scale, rm, rv = _twice(fwd)
        slots, into = _into(case, C, dev)

        def sums():
            s, dgamma, dbeta = ot.bn_local_grad_sums(_rows(ops["dz"], lo, Mr), _rows(ops["zin"], lo, Mr), _rows(ops["y"], lo, Mr),
                                                     mean_in, invstd_in, slot, world, relu=case.relu, grad_mult=case.grad_mult, into=into)
            _check_into(slots, dgamma, dbeta)
            return s, dgamma, dbeta

        s, dgamma, dbeta = _twice(sums)
        assert torch.count_nonzero(torch.cat([s[q] for q in range(world) if q != slot] or [s[:0]])).item() == 0, "foreign slots"
        gsum = s if gsum is None else gsum + s
        o = dict(z=z, mean=mean, invstd=invstd, scale=scale, rm=rm, rv=rv, dgamma=dgamma, dbeta=dbeta, rows=sl, r=r)
        outs.append(o)
        if check:
            for name in ("mean", "invstd", "scale", "rm", "rv"):
                _check(f"slot_finalize+sync_fwd w{world} {name}", dt, o[name], fref[name], fb[name])
            _check(f"bn_sync_fwd_apply w{world} z", dt, z, fref["z"][sl], fb["z"][sl])
            _check(f"slot_finalize m1 w{world} dbeta", dt, dbeta, lrefs[r][0], bb["local"][r][0])
            _check(f"slot_finalize m1 w{world} dgamma", dt, dgamma, lrefs[r][1], bb["local"][r][1])
        lo += Mr
    ops["z"].only_slice_written()
    lo = 0
    for o in outs:
        Mr = o["rows"].stop - o["rows"].start
        lo = o["rows"].start

        def bwd():
            return ot.bn_sync_bwd(_rows(ops["dz"], lo, Mr), _rows(ops["zin"], lo, Mr), _rows(ops["y"], lo, Mr), mean_in, invstd_in,
                                  scale_in, stats, gsum, relu=case.relu, want_dres=True,
                                  out=(_rows(ops["dy"], lo, Mr), _rows(ops["dres"], lo, Mr)))

        o["dy"], o["dres"] = _twice(bwd)
        if check:
            assert torch.equal(o["dres"].cpu().reshape(Mr, C), bref["g"][o["rows"]])
            _check(f"bn_sync_bwd_apply w{world} dy", dt, o["dy"], bref["dy"][o["rows"]], bb["dy"][o["rows"]])
    ops["dy"].only_slice_written(), ops["dres"].only_slice_written()
    for k in ("y", "dz", "zin", "res"):
        if ops[k] is not None:
            ops[k].untouched()
    for o in outs[1:]:      # every rank derives the same statistics
        for k in ("mean", "invstd", "scale", "rm", "rv"):
            assert torch.equal(o[k], outs[0][k])
    return outs


@pytest.mark.parametrize("world", T.WORLDS)
@pytest.mark.parametrize("dt", T.DTYPES, ids=T.dt_name)
@pytest.mark.parametrize("case", T.BN_CASES, ids=T.bn_id)
def test_split_simulated_ranks(ot, dev, case, dt, world):
    """the case's rows dealt to `world` ranks in contiguous chunks (a rank left without rows contributes a slot of zeros): the
    results are those of BatchNorm over all rows; dgamma / dbeta those of the rank's own rows"""
    _split_run(ot, dev, case, dt, T.rank_rows(case.M, world), world)


@pytest.mark.parametrize("where", list(T.HAND_SLOTS))
@pytest.mark.parametrize("dt", T.DTYPES, ids=T.dt_name)
@pytest.mark.parametrize("case", T.HAND_CASES, ids=T.bn_id)
def test_empty_slot_changes_nothing(ot, dev, case, dt, where):
    """a gathered world-3 buffer with an empty first or middle slot (built by hand: bn_local_stats refuses an empty rank): every
    output is bit-identical to the world-2 run of the same two ranks in the same order, also where the empty slot's mean and
    variance fields hold NaN -- a slot without rows is skipped, not combined"""
    parts = T.rank_rows(case.M, 2)
    two = _split_run(ot, dev, case, dt, parts, 2, check=False)
    three = _split_run(ot, dev, case, dt, parts, 3, slot_of=T.HAND_SLOTS[where], check=False, poison=T.HAND_POISON.get(where))
    for a, b in zip(two, three):
        _same([a[k] for k in ("z", "mean", "invstd", "scale", "rm", "rv", "dgamma", "dbeta", "dy", "dres")],
              [b[k] for k in ("z", "mean", "invstd", "scale", "rm", "rv", "dgamma", "dbeta", "dy", "dres")])


@pytest.mark.parametrize("dt", T.DTYPES, ids=T.dt_name)
@pytest.mark.parametrize("case", T.BN_CASES, ids=T.bn_id)
def test_world_one_equals_fused(ot, dev, case, dt):
    """world 1, each pipeline on its own forward's statistics: bit-identical, dy of f32 tensors included -- the three backward-apply
    kernels share one expression (bn_bwd_elem: scale * (g - s0/M - xhat * (s1/M))), at power-of-two and other channel-vector counts
    alike.  dy of f16 tensors is not: the compiler contracts that f32 arithmetic differently in the two kernels before the rounding
    to f16 (measured on an MI355X: 13 of the 24 cases differ, by at most 1.6e-4 of max |dy|) -- bounded as in
    test_one_slot_equals_fused_kernels"""
    inp, ops, par = _operands(case, dt, dev)
    y, dz, zin = ops["y"].view, ops["dz"].view, ops["zin"].view
    res = ops["res"].view if case.res else None
    rm1, rv1, rm2, rv2 = par["rm0"].clone(), par["rv0"].clone(), par["rm0"].clone(), par["rv0"].clone()
    zf, mf, isf, scf = ot.bn_train_fwd(y, par["gamma"], par["beta"], rm1, rv1, case.eps, case.momentum, res=res, relu=case.relu)
    stats = ot.bn_local_stats(y, 0, 1)
    zs, ms, iss, scs = ot.bn_sync_fwd(y, stats, par["gamma"], par["beta"], rm2, rv2, case.eps, case.momentum, res=res, relu=case.relu)
    _same((zf, mf, isf, scf, rm1, rv1), (zs, ms, iss, scs, rm2, rv2))
    dyf, dresf, dgf, dbf = ot.bn_train_bwd(dz, zin, y, mf, isf, scf, relu=case.relu, want_dres=True, grad_mult=case.grad_mult)
    sums, dgs, dbs = ot.bn_local_grad_sums(dz, zin, y, ms, iss, 0, 1, relu=case.relu, grad_mult=case.grad_mult)
    dys, dress = ot.bn_sync_bwd(dz, zin, y, ms, iss, scs, stats, sums, relu=case.relu, want_dres=True)
    _same((dgf, dbf, dresf), (dgs, dbs, dress))
    if dt == F32:
        _same((dyf,), (dys,))
    else:
        a, b = dys.double(), dyf.double()
        assert (a - b).abs().max().item() <= 2e-3 * max(1e-30, b.abs().max().item())
