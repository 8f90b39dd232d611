"""The map-wise kernels between the convolutions -- both max pools, the depthwise up-convolution, the eSE kernels, depth_to_space2 and
preprocess, forward and backward, f16 and f32 -- against float64 references at the edge cases of pointwise_cases.py, which also
states the bounds and records the worst err / bound measured per kernel.  Every test prints its err / bound before it asserts, and
the module prints the worst per kernel and dtype when it ends (run with -s).

The wrappers of ops.py / ops_train.py are used wherever they take what the case needs; the backward wrappers allocate dx themselves,
so the strided backward cases (and ctdet_ese_dot, ctdet_ese_bwd, ctdet_depth_to_space2, which have no wrapper) call the library the
way EseFn and _conv_dgrad_s2_phases do.  In every strided case each tensor is the channel slice [N : N + C] of a buffer 2C + N wide
(16-byte aligned) that is pre-filled with a sentinel bit pattern: everything outside the written slice must come back bit-identical.
"""
import faulthandler
import sys

import pytest
import torch

import pointwise_cases as T

pytestmark = pytest.mark.gpu

F16, F32 = T.F16, T.F32
WORST = {}
WRAP_TIME_LIMIT = 120        # seconds for the wrap case (inputs and reference ~4 s on the CPU, kernels ~1 ms): a hang ends the run there


@pytest.fixture(scope="module")
def ops():
    import detectron2_centernet_amd.ops as ops

    return ops


@pytest.fixture(scope="module")
def ot():
    import detectron2_centernet_amd.ops_train as ot

    return ot


@pytest.fixture(scope="module", autouse=True)
def _worst_table():
    yield
    for (kernel, dt), r in sorted(WORST.items()):
        print(f"worst err / bound  {kernel:<28}{dt}  {r:.3f}")


def _check(kernel, dt, got, ref, n, A, out_dt=None):
    r = T.ratio(got.cpu(), ref, n, A, dt if out_dt is None else out_dt)
    key = (kernel, T.dt_name(dt))
    WORST[key] = max(WORST.get(key, 0.0), r)
    print(f"{kernel} {T.dt_name(dt)}: err / bound {r:.3f}")
    assert r <= 1, (kernel, T.dt_name(dt), r)


def _int(dt):
    return torch.int16 if dt == F16 else torch.int32


def _sentinel(shape, dt, dev):
    return torch.full(shape, T.SENTINEL[dt], dtype=_int(dt), device=dev).view(dt)


def _bits(buf):
    return buf.view(_int(buf.dtype)).cpu()


class Slab:
    """a sentinel-filled buffer [..., 2C + N] and its channel slice [N : N + C], holding t if given"""

    def __init__(self, shape, dt, dev, t=None):
        self.N, self.C = T.VEC[dt], shape[3]
        self.buf = _sentinel((*shape[:3], 2 * self.C + self.N), dt, dev)
        self.view = self.buf[..., self.N:self.N + self.C]
        if t is not None:
            assert tuple(t.shape) == tuple(shape) and t.dtype == dt
            self.view.copy_(t.to(dev))
        self.before = _bits(self.buf)

    def untouched(self):
        """an input: the whole buffer is as it was"""
        assert torch.equal(_bits(self.buf), self.before)

    def only_slice_written(self):
        b, s = _bits(self.buf), T.SENTINEL[self.buf.dtype]
        assert bool((b[..., :self.N] == s).all()) and bool((b[..., self.N + self.C:] == s).all()), "written outside the slice"


def _give(t, dev, strided):
    """(tensor for the kernel, Slab or None)"""
    if not strided:
        return t.to(dev), None
    s = Slab(t.shape, t.dtype, dev, t)
    return s.view, s


def _lib_call(name, *args):
    from detectron2_centernet_amd import _lib

    _lib.check(getattr(_lib.lib(), name)(*args), name)


# ---------------------------------------------------------------------------------------------------------------- pools
@pytest.mark.parametrize("dt", T.DTYPES, ids=T.dt_name)
@pytest.mark.parametrize("case", T.POOL_CASES, ids=T.pool_id)
def test_maxpool(ops, dev, case, dt):
    inp, ref = T.pool_inputs(case, dt), T.pool_reference(case, dt)
    fn = {"2x2": ops.maxpool2x2, "pad1": ops.maxpool3x3s2, "ceil": ops.maxpool3x3s2_ceil}[case.mode]
    x, xs = _give(inp["x"], dev, case.strided)
    if case.strided:
        out = Slab(ref["y"].shape, dt, dev)
        y = fn(x, out=out.view)
        out.only_slice_written()
        xs.untouched()
    else:
        y = fn(x)
    assert y.shape == ref["y"].shape and y.dtype == dt and torch.equal(y.cpu(), ref["y"])


@pytest.mark.parametrize("dt", T.DTYPES, ids=T.dt_name)
@pytest.mark.parametrize("case", T.POOL_CASES, ids=T.pool_id)
def test_maxpool_bwd(ops, ot, dev, case, dt):
    inp, ref = T.pool_inputs(case, dt), T.pool_reference(case, dt)
    x, xs = _give(inp["x"], dev, case.strided)
    dz, dzs = _give(inp["dz"], dev, case.strided)
    B, H, W, C = inp["x"].shape
    if case.strided:
        out = Slab(inp["x"].shape, dt, dev)
        st = ops._nhwc_stride
        if case.mode == "2x2":
            _lib_call("ctdet_maxpool2x2_bwd", ops._ptr(x), st(x), ops._ptr(dz), st(dz), ops._ptr(out.view), st(out.view), B, H, W, C,
                      ops.dt_of(x), ops._stream())
        else:
            _lib_call("ctdet_maxpool3x3s2_bwd", ops._ptr(x), st(x), ops._ptr(dz), st(dz), ops._ptr(out.view), st(out.view),
                      ops.dt_of(x), B, H, W, C, int(case.mode == "ceil"), ops._stream())
        dx = out.view
        out.only_slice_written()
        xs.untouched()
        dzs.untouched()
    else:
        dx = ot.maxpool2x2_bwd(x, dz) if case.mode == "2x2" else ot.maxpool3x3s2_bwd(x, dz, case.mode == "ceil")
    assert dx.dtype == dt and torch.equal(dx.cpu(), ref["dx"])


# ------------------------------------------------------------------------------------------------------- up-convolution
@pytest.mark.parametrize("dt", T.DTYPES, ids=T.dt_name)
@pytest.mark.parametrize("case", T.UP_FWD_CASES, ids=T.up_id)
def test_dwconvT_add(ops, dev, case, dt):
    inp = T.up_inputs(case, dt)
    kernel = f"dwconvT_add_rows<{case.f}>" if T.up_rows_kernel(case) else "dwconvT_add"
    w = inp["w"].to(dev)
    for with_skip in (True, False):
        ref = T.up_fwd_reference(case, dt, with_skip)
        x, xs = _give(inp["x"], dev, case.strided)
        skip, ss = _give(inp["skip"], dev, case.strided) if with_skip else (None, None)
        if case.strided:
            out = Slab(ref["y"].shape, dt, dev)
            y = ops.dwconvT_add(x, w, case.f, skip=skip, out=out.view)
            out.only_slice_written()
            xs.untouched()
            if ss is not None:
                ss.untouched()
        else:
            y = ops.dwconvT_add(x, w, case.f, skip=skip)
        assert y.shape == ref["y"].shape and y.dtype == dt
        _check(kernel, dt, y, ref["y"], ref["n"], ref["A"])


def _dwconvT_bwd(ops, ot, dev, case, dt, inp):
    """dx [B,H,W,C], dw [C,1,k,k] of the kernels; strided: through the library, x, dz and dx as channel slices"""
    if not case.strided:
        return ot.dwconvT_bwd(inp["x"].to(dev), inp["dz"].to(dev), inp["w"].to(dev), case.f)
    B, H, W, C = inp["x"].shape
    k = 2 * case.f
    x, xs = _give(inp["x"], dev, True)
    dz, dzs = _give(inp["dz"], dev, True)
    out = Slab(inp["x"].shape, dt, dev)
    wk = inp["w"].reshape(C, k, k).permute(1, 2, 0).contiguous().to(dev)
    dw = torch.zeros(k, k, C, dtype=F32, device=dev)
    st = ops._nhwc_stride
    _lib_call("ctdet_dwconvT_bwd", ops._ptr(x), st(x), ops._ptr(dz), st(dz), ops._ptr(wk), ops._ptr(out.view), st(out.view),
              ops._ptr(dw), B, H, W, C, case.f, ops.dt_of(x), ops._stream())
    out.only_slice_written()
    xs.untouched()
    dzs.untouched()
    return out.view, dw.permute(2, 0, 1).reshape(C, 1, k, k)


@pytest.mark.parametrize("dt", T.DTYPES, ids=T.dt_name)
@pytest.mark.parametrize("case", T.UP_BWD_CASES, ids=T.up_id)
def test_dwconvT_bwd(ops, ot, dev, case, dt):
    inp, ref = T.up_inputs(case, dt), T.up_bwd_reference(case, dt)
    dx, dw = _dwconvT_bwd(ops, ot, dev, case, dt, inp)
    assert dx.dtype == dt and dw.dtype == F32 and dx.shape == ref["dx"].shape and dw.shape == ref["dw"].shape
    _check("dwconvT_dx", dt, dx, ref["dx"], ref["n_dx"], ref["A_dx"])
    _check("dwconvT_dw", dt, dw, ref["dw"], ref["n_dw"], ref["A_dw"], out_dt=F32)


def test_dwconvT_bwd_wrap(ops, ot, dev):
    """both grid caps: dwconvT_dw_kernel strides past 512 workgroups per phase, dwconvT_dx_kernel past 4096.  Its own time limit:
    the process ends with a traceback if the case hangs, and nothing more is started on the GPU."""
    case, dt = T.UP_WRAP_CASE, T.UP_WRAP_DTYPE
    faulthandler.dump_traceback_later(WRAP_TIME_LIMIT, exit=True, file=sys.__stderr__)
    try:
        inp, ref = T.up_inputs(case, dt), T.up_wrap_reference()
        dx, dw = ot.dwconvT_bwd(inp["x"].to(dev), inp["dz"].to(dev), inp["w"].to(dev), case.f)
        torch.cuda.synchronize()
    finally:
        faulthandler.cancel_dump_traceback_later()
    _check("dwconvT_dx (wrap)", dt, dx, ref["dx"], ref["n_dx"], ref["A_dx"])
    _check("dwconvT_dw (wrap)", dt, dw, ref["dw"], ref["n_dw"], ref["A_dw"], out_dt=F32)


@pytest.mark.parametrize("dt", T.DTYPES, ids=T.dt_name)
def test_dwconvT_refuses_odd_factors_in_both_directions(ops, ot, dev, dt):
    """f = 1 (no IDAUp builds it: ConvTranspose2d(k=2, s=1, p=0) has H + 1 rows) and odd f are refused before any launch, forward as
    backward"""
    C = 2 * T.VEC[dt]
    x = torch.ones(1, 3, 2, C, dtype=dt, device=dev)
    for f in (1, 3):
        w = torch.ones(C, 1, 2 * f, 2 * f, device=dev)
        out = Slab((1, 3 * f, 2 * f, C), dt, dev)
        with pytest.raises(RuntimeError, match="up factor"):
            ops.dwconvT_add(x, w, f, out=out.view)
        with pytest.raises(RuntimeError, match="dwconvT_bwd"):
            ot.dwconvT_bwd(x, torch.ones(1, 3 * f, 2 * f, C, dtype=dt, device=dev), w, f)
        torch.cuda.synchronize()
        out.untouched()
    assert bool((x == 1).all())


# ------------------------------------------------------------------------------------------------------------------ eSE
@pytest.mark.parametrize("dt", T.DTYPES, ids=T.dt_name)
@pytest.mark.parametrize("case", T.ESE_CASES, ids=T.ese_id)
def test_global_avgpool(ops, dev, case, dt):
    inp, ref = T.ese_inputs(case, dt), T.ese_reference(case, dt)
    x, xs = _give(inp["x"], dev, case.strided)
    out = ops.global_avgpool(x)
    if xs is not None:
        xs.untouched()
    assert out.dtype == F32 and out.shape == ref["mean"].shape
    _check("global_avgpool", dt, out, ref["mean"], ref["HW"], ref["A_mean"], out_dt=F32)


@pytest.mark.parametrize("dt", T.DTYPES, ids=T.dt_name)
@pytest.mark.parametrize("case", T.ESE_CASES, ids=T.ese_id)
def test_ese_scale(ops, dev, case, dt):
    inp, ref = T.ese_inputs(case, dt), T.ese_reference(case, dt)
    gi = T.ese_gate_index(case.B, inp["x"].shape[3])[:, None, None, :].expand(inp["x"].shape)
    gate0 = (gi == T.ESE_GATE0[0]) | (gi == T.ESE_GATE0[1])
    gate1 = (gi == T.ESE_GATE1[0]) | (gi == T.ESE_GATE1[1])
    s = inp["s"].to(dev)
    for with_id in (True, False):
        x, xs = _give(inp["x"], dev, case.strided)
        idn, ids = _give(inp["identity"], dev, case.strided) if with_id else (None, None)
        if case.strided:
            out = Slab(inp["x"].shape, dt, dev)
            y = ops.ese_scale(x, s, idn, out=out.view)
            out.only_slice_written()
            xs.untouched()
            if ids is not None:
                ids.untouched()
        else:
            y = ops.ese_scale(x, s, idn)
        key = "scale_id" if with_id else "scale"
        _check("ese_scale", dt, y, ref[key], 2 if with_id else 1, ref["A_" + key])
        # the saturated gates: identity (or 0) where the gate is 0, x + identity (or x) after one rounding where it is 1
        y = y.cpu()
        zero, one = (inp["identity"], (inp["x"].double() + inp["identity"].double()).to(dt)) if with_id else (torch.zeros_like(y), inp["x"])
        assert torch.equal(y[gate0], zero[gate0]) and torch.equal(y[gate1], one[gate1])


@pytest.mark.parametrize("dt", T.DTYPES, ids=T.dt_name)
@pytest.mark.parametrize("case", T.ESE_CASES, ids=T.ese_id)
def test_ese_dot(ops, dev, case, dt):
    inp, ref = T.ese_inputs(case, dt), T.ese_reference(case, dt)
    B, H, W, C = inp["x"].shape
    x, xs = _give(inp["x"], dev, case.strided)
    dy, dys = _give(inp["dy_dot"], dev, case.strided)
    r = _sentinel((B, C), F32, dev)
    st = ops._nhwc_stride
    _lib_call("ctdet_ese_dot", ops._ptr(dy), st(dy), ops._ptr(x), st(x), ops.dt_of(x), B, H * W, C, ops._ptr(r), ops._stream())
    if case.strided:
        xs.untouched()
        dys.untouched()
    _check("ese_dot", dt, r, ref["dot"], ref["HW"], ref["A_dot"], out_dt=F32)


@pytest.mark.parametrize("dt", T.DTYPES, ids=T.dt_name)
@pytest.mark.parametrize("case", T.ESE_CASES, ids=T.ese_id)
def test_ese_bwd(ops, dev, case, dt):
    inp, ref = T.ese_inputs(case, dt), T.ese_reference(case, dt)
    B, H, W, C = inp["x"].shape
    dy, dys = _give(inp["dy"], dev, case.strided)
    gate, gp = inp["gate"].to(dev), inp["gp"].to(dev)
    out = Slab(inp["x"].shape, dt, dev) if case.strided else None
    dx = out.view if case.strided else _sentinel(inp["x"].shape, dt, dev)
    st = ops._nhwc_stride
    _lib_call("ctdet_ese_bwd", ops._ptr(dy), st(dy), ops._ptr(gate), ops._ptr(gp), ops._ptr(dx), st(dx), ops.dt_of(dy), B, H * W, C,
              ops._stream())
    if case.strided:
        out.only_slice_written()
        dys.untouched()
    _check("ese_bwd", dt, dx, ref["bwd"], 2, ref["A_bwd"])
    gi = T.ese_gate_index(B, C)[:, None, None, :].expand(inp["x"].shape)
    gate0 = (gi == T.ESE_GATE0[0]) | (gi == T.ESE_GATE0[1])
    assert torch.equal(dx.cpu()[gate0].double(), inp["gp"][:, None, None, :].expand(inp["x"].shape)[gate0].to(dt).double())


# ------------------------------------------------------------------------------------------------------ depth_to_space2
def _depth_to_space2(ops, src, dst, case, Hs, Ws):
    B, H, W, C = dst.shape
    _lib_call("ctdet_depth_to_space2", ops._ptr(src), src.shape[3], ops._ptr(dst), dst.stride(2),
              B, H, W, C, Hs, Ws, ops.dt_of(dst), ops._stream())


@pytest.mark.parametrize("dt", T.DTYPES, ids=T.dt_name)
@pytest.mark.parametrize("case", T.D2S_CASES, ids=T.d2s_id)
def test_depth_to_space2(ops, dev, case, dt):
    src_cpu, ref = T.d2s_inputs(case, dt), T.d2s_reference(case, dt)
    src = src_cpu.to(dev)
    out = Slab(ref.shape, dt, dev)
    _depth_to_space2(ops, src, out.view, case, *T.d2s_src_hw(case.H, case.W))
    out.only_slice_written()
    assert torch.equal(out.view.cpu(), ref) and torch.equal(src.cpu(), src_cpu)


@pytest.mark.parametrize("dt", T.DTYPES, ids=T.dt_name)
def test_depth_to_space2_refuses_a_source_one_row_short(ops, dev, dt):
    case = T.D2S_RAISES
    Hs, Ws = T.d2s_src_hw(case.H, case.W)
    src = T.d2s_inputs(case, dt).to(dev)
    out = Slab((case.B, case.H, case.W, case.CV * T.VEC[dt]), dt, dev)
    for hs, ws in ((Hs - 1, Ws), (Hs, Ws - 1)):
        with pytest.raises(RuntimeError, match="too small"):
            _depth_to_space2(ops, src, out.view, case, hs, ws)
    torch.cuda.synchronize()
    out.untouched()


# ----------------------------------------------------------------------------------------------------------- preprocess
@pytest.mark.parametrize("case", T.PRE_CASES, ids=T.pre_id)
def test_preprocess(ops, dev, case):
    img, ref = T.pre_inputs(case.in_dt, case.H, case.W), T.pre_reference(case)
    b = case.border
    out = _sentinel((T.PRE_B, case.Hp + 2 * b, case.Wp + 2 * b, case.out_stride), case.out_dt, dev)
    got = ops.preprocess(img.to(dev), T.PRE_MEAN, T.PRE_STD, case.Hp, case.Wp, out_dtype=case.out_dt, out=out, border=b)
    assert got.data_ptr() == out.data_ptr()
    bits = _bits(out)
    inner = torch.zeros(bits.shape[:3], dtype=torch.bool)
    inner[:, b:b + case.Hp, b:b + case.Wp] = True
    assert bool((bits[~inner] == T.SENTINEL[case.out_dt]).all()), "the border frame was touched"
    y = out.cpu()[:, b:b + case.Hp, b:b + case.Wp]
    assert not y[..., 3:].any(), "channels 3.. are not zero"
    assert not y[:, case.H:].any() and not y[:, :, case.W:].any(), "the padding is not zero"
    kernel = f"preprocess {'u8' if case.in_dt == torch.uint8 else 'f32'}->{T.dt_name(case.out_dt)}"
    _check(kernel, case.out_dt, y[..., :3], ref["y"], ref["n"], ref["A"])
