"""The case tables of pointwise_cases.py against their own conditions, without a GPU: every shape takes the branch it is listed for
(computed from the launch constants mirrored from the sources), the promised ties / infinities / gates / 0 and 255 pixels are in
place, no f16 reference output is subnormal, torch in f32 on the CPU meets every bound against the float64 reference (the bounds
are attainable), a deliberately wrong reference of every family breaks its bound or its equality on a listed case, and nothing is
filtered out on the way to the GPU tests."""
import pytest
import torch
import torch.nn.functional as F

import pointwise_cases as T

F16, F32 = T.F16, T.F32


def _params(fn, name=None):
    marks = [m for m in fn.pytestmark if m.name == "parametrize" and (name is None or m.args[0] == name)]
    return [p for m in marks for p in m.args[1]]


def _no_subnormal(ref, dt):
    a = ref.abs()
    return dt != F16 or bool(((a == 0) | (a >= T.F16_MIN_NORMAL)).all())


def test_mirrored_constants_match_the_sources():
    import os
    import re

    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "detectron2-centernet_amd", "csrc")
    pw, bw = open(os.path.join(csrc, "pointwise.hip")).read(), open(os.path.join(csrc, "train_bwd.hip")).read()
    assert int(re.search(r"constexpr int DW_ROWS = (\d+);", pw).group(1)) == T.DW_ROWS
    body = bw[bw.index("static int launch_dwconvT_bwd_t"):bw.index("int launch_dwconvT_bwd(")]
    assert f"S * {T.DW_POS_PER_SUB} - 1) / (S * {T.DW_POS_PER_SUB})" in body and "const int S = 256 / (C / N);" in body
    assert f"if (nb > {T.DW_GRID_CAP}) nb = {T.DW_GRID_CAP};" in body and f"if (nbx > {T.DX_GRID_CAP}) nbx = {T.DX_GRID_CAP};" in body
    assert f"blockIdx.x * {T.ESE_CH} + (threadIdx.x & {T.ESE_CH - 1}), pl = threadIdx.x >> 6" in pw and "p += 4" in pw
    assert T.ESE_CH * T.ESE_PL == T.BLOCK and T.VEC == {F16: 8, F32: 4}


# ---------------------------------------------------------------------------------------------------------------- pools
def test_pool_table():
    two = [c for c in T.POOL_CASES if c.mode == "2x2"]
    assert [(c.B, c.H, c.W, c.CV, c.strided) for c in two] == [(1, 2, 2, 1, False), (2, 6, 10, 3, False), (2, 10, 14, 5, False), (2, 6, 10, 3, True)]
    vecs = [c.B * (c.H // 2) * (c.W // 2) * c.CV for c in two]
    assert vecs[0] == 1 and vecs[2] == 350 and T.BLOCK < 350 < 2 * T.BLOCK
    assert two[1].CV & (two[1].CV - 1) and two[2].CV & (two[2].CV - 1)
    for mode in ("pad1", "ceil"):
        got = {(c.H, c.W) for c in T.POOL_CASES if c.mode == mode and not c.strided}
        assert got == {(3, 3), (4, 7), (5, 8), (8, 5), (4, 6), (17, 25)}
        assert sum(c.mode == mode and c.strided for c in T.POOL_CASES) == 1
        assert all(c.CV == 2 for c in T.POOL_CASES if c.mode == mode)
    # which ceil windows hang over the map: the last one covers rows 2 (Ho - 1) .. 2 (Ho - 1) + 2
    hang = {(H, W): (2 * (T.pool_out_hw("ceil", H, W)[0] - 1) + 2 - (H - 1), 2 * (T.pool_out_hw("ceil", H, W)[1] - 1) + 2 - (W - 1))
            for (H, W) in ((3, 3), (4, 7), (5, 8), (8, 5), (4, 6), (17, 25))}
    assert hang == {(3, 3): (0, 0), (4, 7): (1, 0), (5, 8): (0, 1), (8, 5): (1, 0), (4, 6): (1, 1), (17, 25): (0, 0)}
    assert T.pool_out_hw("ceil", 3, 3) == (1, 1) and T.pool_out_hw("pad1", 3, 3) == (2, 2)
    # 17 x 25: element (8, 12) lies in four ceil windows, element (7, 11) in four pad-1 windows
    for mode, (ey, ex) in (("pad1", (7, 11)), ("ceil", (8, 12))):
        Ho, Wo = T.pool_out_hw(mode, 17, 25)
        n = sum(ey in T.pool_window(mode, 17, 25, ho, wo)[0] and ex in T.pool_window(mode, 17, 25, ho, wo)[1] for ho in range(Ho) for wo in range(Wo))
        assert n == 4
    # launch_maxpool3x3s2's `--Ho` never fires: the last ceil window always starts inside the map, and torch agrees on the size
    for H in range(3, 65):
        Ho = (H - 3 + 1) // 2 + 1
        assert (Ho - 1) * 2 < H and Ho == T.pool_out_hw("ceil", H, H)[0]
        assert F.max_pool2d(torch.zeros(1, 1, H, 3), 3, 2, 0, ceil_mode=True).shape[2] == Ho
    assert len(set(T.POOL_CASES)) == len(T.POOL_CASES)


@pytest.mark.parametrize("dt", T.DTYPES, ids=T.dt_name)
@pytest.mark.parametrize("case", T.POOL_CASES, ids=T.pool_id)
def test_pool_case_holds_what_it_promises(case, dt):
    inp = T.pool_inputs(case, dt)
    x, dz = inp["x"].double(), inp["dz"].double()
    C = case.CV * T.VEC[dt]
    assert inp["x"].dtype == inp["dz"].dtype == dt and x.shape == (case.B, case.H, case.W, C)
    assert dz.shape == (case.B, *T.pool_out_hw(case.mode, case.H, case.W), C)
    assert torch.equal(dz * 64, (dz * 64).round()) and dz.abs().max() <= 4
    fin = torch.isfinite(x)
    assert torch.equal(x[fin] * 2, (x[fin] * 2).round()) and x[fin].abs().max() <= 2
    ys, xs = T.pool_window(case.mode, case.H, case.W, 0, 0)
    win = inp["x"][0][ys][:, xs]                                   # [rows, cols, C] of window (0, 0)
    assert T.POOL_SPECIALS == ("constant", "zeros", "ninf", "pinf") and C >= 4
    assert bool((win[..., 0] == 1).all())
    z = win[..., 1].reshape(-1)
    assert bool((z == 0).all()) and torch.signbit(z).any() and not torch.signbit(z).all()
    assert bool((win[..., 2] == float("-inf")).all())
    assert int((win[..., 3] == float("inf")).sum()) == 1 and int(torch.isinf(inp["x"][..., 3]).sum()) == 1
    # ties in most windows of the random part
    y = T.pool_reference(case, dt)["y"]
    ties = 0
    Ho, Wo = y.shape[1:3]
    for ho in range(Ho):
        for wo in range(Wo):
            ys, xs = T.pool_window(case.mode, case.H, case.W, ho, wo)
            w = inp["x"][:, ys][:, :, xs]
            ties += int(((w == y[:, ho:ho + 1, wo:wo + 1]).sum((1, 2)) > 1).sum())
    assert ties > 0.15 * y.numel()
    # sums of up to four gradients are representable in the tensor type: rounding the float64 gradient loses nothing
    x64 = T.nchw(inp["x"]).double().requires_grad_(True)
    T._pool_f(case.mode, x64).backward(T.nchw(dz))
    assert torch.equal(T.nhwc(x64.grad), T.pool_reference(case, dt)["dx"].double())


@pytest.mark.parametrize("dt", T.DTYPES, ids=T.dt_name)
@pytest.mark.parametrize("case", T.POOL_CASES, ids=T.pool_id)
def test_pool_f32_torch_equals_f64(case, dt):
    r64, r32 = T.pool_reference(case, dt), T.pool_reference(case, dt, compute=torch.float32)
    assert torch.equal(r64["y"], r32["y"]) and torch.equal(r64["dx"], r32["dx"])
    dz = T.pool_inputs(case, dt)["dz"].double()
    assert r64["dx"].double().sum((1, 2)).sub(dz.sum((1, 2))).abs().max() == 0        # every gradient lands exactly once


def test_pool_wrong_references_are_told_apart():
    for dt in T.DTYPES:
        two = [c for c in T.POOL_CASES if c.mode == "2x2"]
        assert all(not torch.equal(T.pool_reference_last_max(c, dt), T.pool_reference(c, dt)["dx"]) for c in two)
        for c in T.POOL_CASES:
            if c.mode != "ceil":
                continue
            good, floor = T.pool_reference(c, dt)["y"], T.pool_reference_floor(c, dt)
            hangs = (c.H % 2 == 0, c.W % 2 == 0)
            assert (good.shape[1] - floor.shape[1], good.shape[2] - floor.shape[2]) == (int(hangs[0]), int(hangs[1]))
            assert torch.equal(good[:, :floor.shape[1], :floor.shape[2]], floor)
        assert sum(T.pool_reference(c, dt)["y"].shape != T.pool_reference_floor(c, dt).shape for c in T.POOL_CASES if c.mode == "ceil") >= 4


# ------------------------------------------------------------------------------------------------------- up-convolution
def test_up_forward_table():
    cases = T.UP_FWD_CASES
    assert len(set(cases)) == len(cases)
    rows = [c for c in cases if T.up_rows_kernel(c)]
    gen = [c for c in cases if not T.up_rows_kernel(c)]
    assert {(c.f, c.CV) for c in rows} == {(f, cv) for f in (2, 4, 8) for cv in (1, 8)}
    assert {(c.f, c.CV) for c in gen} == {(2, 3), (4, 3), (6, 8), (6, 3)}
    for f in (2, 4, 8):
        for cv in (1, 8):
            maps = {(c.B, c.H, c.W) for c in rows if (c.f, c.CV) == (f, cv) and not c.strided}
            assert {(1, 1, 1), (1, 9, 3), (2, 9, 3)} <= maps
    assert -(-9 // T.DW_ROWS) == 2 and 9 - T.DW_ROWS == 1                # two chunks, the second with one input row
    assert T.up_grid(T.UpCase(2, 9, 3, 8, 4, False)) == (1, 2 * 2 * 4)    # blockIdx.y = (b, chunk, phase)
    wide = [c for c in rows if c.W * c.f * c.CV == 320]
    assert len(wide) == 3 and {c.f for c in wide} == {2, 4, 8} and all(T.up_grid(c)[0] == 2 and 320 % T.BLOCK for c in wide)
    assert all(c.W * c.f * c.CV < T.BLOCK for c in rows if c not in wide)
    assert any(T.up_grid(c)[0] > 1 and (c.B * c.H * c.f * c.W * c.f * c.CV) % T.BLOCK for c in gen)      # generic: ragged last workgroup
    assert sorted(T.up_rows_kernel(c) for c in cases if c.strided) == [False, True]
    assert all(c.f % 2 == 0 for c in cases)


def test_up_backward_table():
    cases = T.UP_BWD_CASES
    assert len(set(cases)) == len(cases) and T.UP_WRAP_CASE not in cases
    assert {c.f for c in cases} == {2, 4, 8} and {c.CV for c in cases} == {1, 3, 8, 256}
    for f in (2, 4, 8):
        for cv in (1, 3, 8):
            assert {(1, 1, 1), (1, 9, 3), (2, 9, 3)} <= {(c.B, c.H, c.W) for c in cases if (c.f, c.CV) == (f, cv)}
    assert T.dw_sub_threads(3) == 85 and 85 * 3 < T.BLOCK                 # idle threads
    big = next(c for c in cases if c.CV == 256)
    assert T.dw_sub_threads(256) == 1 and (big.H, big.W) == (2, 2) and 4 * 256 * 8 * 4 == 32768

    def dw_groups(c):
        npos, S = c.B * (c.H + 1) * (c.W + 1), T.dw_sub_threads(c.CV)
        return min(max(-(-npos // (S * T.DW_POS_PER_SUB)), 1), T.DW_GRID_CAP)

    def dx_groups(c):
        return min(-(-(c.B * c.H * c.W * c.CV) // T.BLOCK), T.DX_GRID_CAP)

    assert [c for c in cases if dw_groups(c) > 1] == [T.UpCase(2, 17, 15, 8, 2, False)] and dw_groups(T.UpCase(2, 17, 15, 8, 2, False)) == 2
    assert any(dx_groups(c) > 1 for c in cases) and sum(c.strided for c in cases) == 1
    # the wrap case: both caps, and one row fewer misses the first
    w = T.UP_WRAP_CASE
    S = T.dw_sub_threads(w.CV)
    assert w == T.UpCase(4, 255, 256, 8, 2, False) and w.CV & (w.CV - 1) == 0 and T.UP_WRAP_DTYPE == F16
    assert w.B * (w.H + 1) * (w.W + 1) == 263168 > T.DW_GRID_CAP * T.DW_POS_PER_SUB * S == 262144
    assert w.B * w.H * w.W * w.CV == 2088960 > T.DX_GRID_CAP * T.BLOCK == 1048576
    assert w.B * w.H * (w.W + 1) == 262140 <= T.DW_GRID_CAP * T.DW_POS_PER_SUB * S          # one row fewer misses the first
    assert -(-(w.B * w.H * (w.W + 1)) // (S * T.DW_POS_PER_SUB)) == T.DW_GRID_CAP               # ... its grid is exactly the cap
    assert 4 * 257 * 257 == 264196 and 4 * 256 * 257 > 262144      # 256 x 256 is not the smallest: a row less still wraps
    assert dw_groups(w) == T.DW_GRID_CAP and dx_groups(w) == T.DX_GRID_CAP
    assert T.up_wrap_tail(w) == (3, 253) and w.B - 1 == 3       # the last two input rows of the last image


@pytest.mark.parametrize("dt", T.DTYPES, ids=T.dt_name)
@pytest.mark.parametrize("case", T.UP_FWD_CASES, ids=T.up_id)
def test_up_forward_bounds_are_attainable(case, dt):
    inp = T.up_inputs(case, dt)
    C = case.CV * T.VEC[dt]
    sg, tau = T.chan_signs(C)
    assert inp["x"].dtype == inp["skip"].dtype == dt and inp["w"].dtype == F32 and inp["w"].shape == (C, 1, 2 * case.f, 2 * case.f)
    assert bool((torch.sign(inp["x"].float()) == sg).all()) and bool((torch.sign(inp["skip"].float()) == sg * tau).all())
    assert bool((torch.sign(inp["w"]) == tau.view(C, 1, 1, 1)).all()) and inp["x"].abs().min() >= 0.25 and inp["w"].abs().min() >= 0.25
    for with_skip in (True, False):
        r64 = T.up_fwd_reference(case, dt, with_skip)
        r32 = T.up_fwd_reference(case, dt, with_skip, compute=torch.float32)
        n = r64["n"] - (1 if with_skip else 0)
        assert n.min() >= 1 and n.max() == (4 if case.H > 1 and case.W > 1 else 2 if case.H * case.W > 1 else 1)
        if case.H == case.W == 1:
            assert n.max() == 1                  # every tap hits a border
        assert torch.equal(r64["A"], r64["y"].abs()) and _no_subnormal(r64["y"], dt)
        assert T.ratio(r32["y"].to(dt), r64["y"], r64["n"], r64["A"], dt) <= 1
        bad = T.up_fwd_reference(case, dt, with_skip, drop_tap=True)          # one border tap dropped
        assert T.ratio(bad["y"].to(dt), r64["y"], r64["n"], r64["A"], dt) > 1


@pytest.mark.parametrize("dt", T.DTYPES, ids=T.dt_name)
@pytest.mark.parametrize("case", T.UP_BWD_CASES, ids=T.up_id)
def test_up_backward_bounds_are_attainable(case, dt):
    inp = T.up_inputs(case, dt)
    sg, _ = T.chan_signs(case.CV * T.VEC[dt])
    assert bool((torch.sign(inp["dz"].float()) == sg).all()) and inp["dz"].abs().min() >= 0.25
    r64, r32 = T.up_bwd_reference(case, dt), T.up_bwd_reference(case, dt, compute=torch.float32)
    k = 2 * case.f
    assert r64["n_dx"].max() <= k * k and r64["n_dx"].min() >= 1 and r64["n_dw"].max() <= case.B * case.H * case.W
    if case.H == case.W == 1:
        assert r64["n_dx"].max() == case.f * case.f and r64["n_dw"].max() == 1
    assert torch.equal(r64["A_dx"], r64["dx"].abs()) and _no_subnormal(r64["dx"], dt)
    assert T.ratio(r32["dx"].to(dt), r64["dx"], r64["n_dx"], r64["A_dx"], dt) <= 1
    assert T.ratio(r32["dw"], r64["dw"], r64["n_dw"], r64["A_dw"], F32) <= 1
    # the tap-by-tap form that the wrap case uses is the same function
    dx, dw, ndx, ndw = T.up_bwd_by_taps(inp["x"], inp["dz"], inp["w"], case.f)
    assert torch.equal(ndx, r64["n_dx"]) and torch.equal(ndw, r64["n_dw"])
    assert (dx - r64["dx"]).abs().max() <= 1e-12 * r64["A_dx"].max() and (dw - r64["dw"]).abs().max() <= 1e-12 * r64["A_dw"].max()
    assert (dw.abs() - r64["A_dw"]).abs().max() <= 1e-12 * r64["A_dw"].max()          # one sign per sum: A = |ref|
    # wrong on purpose: the last dx pixel without the tap of the last output pixel, dw without the last input row
    bad, q = r64["dx"].clone(), case.f - 1 + case.f // 2
    bad[:, -1, -1] -= inp["dz"].double()[:, -1, -1] * inp["w"].double()[:, 0, q, q]
    assert T.ratio(bad.to(dt), r64["dx"], r64["n_dx"], r64["A_dx"], dt) > 1
    _, bad_dw, _, _ = T.up_bwd_by_taps(inp["x"], inp["dz"], inp["w"], case.f, skip_from=(case.B - 1, case.H - 1))
    assert T.ratio(bad_dw, r64["dw"], r64["n_dw"], r64["A_dw"], F32) > 1


# ------------------------------------------------------------------------------------------------------------------ eSE
def test_ese_table():
    assert [(c.B, c.H * c.W, c.C) for c in T.ESE_CASES if not c.strided] == [(1, 1, None), (2, 3, None), (3, 117, 80), (2, 64, 128)]
    assert sum(c.strided for c in T.ESE_CASES) == 1
    assert 1 < T.ESE_PL and 3 < T.ESE_PL and max(T.VEC.values()) < T.ESE_CH and 80 % T.ESE_CH and -(-80 // T.ESE_CH) == 2
    gates = torch.tensor(T.ESE_GATES, dtype=torch.float32)
    assert gates.double().tolist() == T.ESE_GATES                               # all seven are f32 numbers
    assert (gates + 3.0).double().tolist() == [g + 3.0 for g in T.ESE_GATES]     # s + 3 is exact in f32
    g = T.hsigmoid(gates.double())
    assert [g[i].item() for i in T.ESE_GATE0] == [0.0, 0.0] and [g[i].item() for i in T.ESE_GATE1] == [1.0, 1.0]
    assert g[T.ESE_TINY].item() == 2.0 ** -20 / 6 and g[3].item() == 0.5 and 0 < 1 - g[4].item() < 1e-6
    for dt in T.DTYPES:
        for c in T.ESE_CASES:
            gi = T.ese_gate_index(c.B, T.ese_channels(c, dt))
            assert c.B * T.ese_channels(c, dt) < 7 or set(gi.reshape(-1).tolist()) == set(range(7)), (c, dt)
    assert set(T.ese_gate_index(2, 4).reshape(-1).tolist()) == set(range(7))


@pytest.mark.parametrize("dt", T.DTYPES, ids=T.dt_name)
@pytest.mark.parametrize("case", T.ESE_CASES, ids=T.ese_id)
def test_ese_bounds_are_attainable(case, dt):
    inp = T.ese_inputs(case, dt)
    C = T.ese_channels(case, dt)
    assert all(inp[k].dtype == dt and inp[k].shape == (case.B, case.H, case.W, C) for k in ("x", "identity", "dy", "dy_dot"))
    assert all(inp[k].dtype == F32 and inp[k].shape == (case.B, C) for k in ("s", "gate", "gp"))
    assert torch.equal(inp["s"], torch.tensor(T.ESE_GATES, dtype=F32)[T.ese_gate_index(case.B, C)])
    assert torch.equal(inp["gate"].double(), T.hsigmoid(inp["s"].double()).float().double())
    r64, r32 = T.ese_reference(case, dt), T.ese_reference(case, dt, compute=torch.float32)
    HW = r64["HW"]
    for key, n, odt in (("mean", HW, F32), ("scale", 1, dt), ("scale_id", 2, dt), ("dot", HW, F32), ("bwd", 2, dt)):
        assert _no_subnormal(r64[key], odt), key
        assert T.ratio(r32[key].to(odt), r64[key], n, r64["A_" + key], odt) <= 1, key
    # x + identity is exact in float64: "one rounding" is one rounding
    x, idn = inp["x"].double(), inp["identity"].double()
    assert torch.equal((x + idn) - x, idn) and torch.equal((x + idn) - idn, x)
    # wrong references: the mean over HW + 1 values, hsigmoid without its upper clamp
    assert T.ratio(T.ese_reference(case, dt, mean_div_extra=1)["mean"].float(), r64["mean"], HW, r64["A_mean"], F32) > 1
    bad = T.ese_reference(case, dt, clamp_hi=False)
    if case.B * C >= 7:
        assert T.ratio(bad["scale_id"].to(dt), r64["scale_id"], 2, r64["A_scale_id"], dt) > 1
        assert T.ratio(bad["scale"].to(dt), r64["scale"], 1, r64["A_scale"], dt) > 1


# ------------------------------------------------------------------------------------------------------ depth_to_space2
def test_d2s_table():
    assert [(c.B, c.H, c.W, c.CV) for c in T.D2S_CASES if not c.wide] == [(1, 1, 1, 1), (2, 5, 4, 3), (1, 6, 7, 2)]
    assert [c._replace(wide=False) for c in T.D2S_CASES if c.wide] == [c for c in T.D2S_CASES if not c.wide]
    assert [T.d2s_src_hw(c.H, c.W) for c in T.D2S_CASES if not c.wide] == [(1, 1), (3, 3), (4, 4)]
    assert T.D2S_RAISES._replace(wide=True) in T.D2S_CASES
    for dt in T.DTYPES:
        for c in T.D2S_CASES:
            src, ref = T.d2s_inputs(c, dt), T.d2s_reference(c, dt)
            C = c.CV * T.VEC[dt]
            assert src.shape[3] == 4 * C + (T.VEC[dt] if c.wide else 0) and src.dtype == dt
            assert src.double().reshape(-1).tolist() == list(range(src.numel())) and src.numel() <= 2048        # distinct, exact in f16
            Hs, Ws = src.shape[1:3]
            assert (c.H // 2 + 1, c.W // 2 + 1) == (Hs, Ws)                 # the largest source index read is (H / 2, W / 2)
            assert len(set(ref.double().reshape(-1).tolist())) == ref.numel()
            if c.H > 1 or c.W > 1:
                assert not torch.equal(T.d2s_reference(c, dt, swap_parity=True), ref)
    assert sum(not torch.equal(T.d2s_reference(c, F16, swap_parity=True), T.d2s_reference(c, F16)) for c in T.D2S_CASES) == 4


# ----------------------------------------------------------------------------------------------------------- preprocess
def test_preprocess_table():
    assert len(T.PRE_CASES) == len(set(T.PRE_CASES)) == 3 * 2 * (2 * 1 + 2 * 2)
    assert {(c.in_dt, c.out_dt) for c in T.PRE_CASES} == {(i, o) for i in (torch.uint8, F32) for o in (F16, F32)}
    assert {(c.H, c.W, c.Hp, c.Wp) for c in T.PRE_CASES} == {(1, 1, 2, 3), (5, 7, 5, 7), (50, 70, 64, 96)}
    assert {c.border for c in T.PRE_CASES} == {0, 3}
    assert {c.out_stride for c in T.PRE_CASES if c.out_dt == F32} == {4, 8} and {c.out_stride for c in T.PRE_CASES if c.out_dt == F16} == {8}
    assert T.PRE_B * 64 * 96 > 2 * T.BLOCK and (T.PRE_B * 64 * 96) % T.BLOCK == 0 and (T.PRE_B * 5 * 7) % T.BLOCK


@pytest.mark.parametrize("case", T.PRE_CASES, ids=T.pre_id)
def test_preprocess_bounds_are_attainable(case):
    img = T.pre_inputs(case.in_dt, case.H, case.W)
    assert img.dtype == case.in_dt and img.shape == (T.PRE_B, 3, case.H, case.W)
    for ch in range(3):
        assert bool((img[:, ch] == 0).any()) and bool((img[:, ch] == 255).any())
    assert img.min() >= 0 and img.max() <= 255
    if case.in_dt == F32 and case.H > 1:
        assert bool((img != img.round()).any())
    r64, r32 = T.pre_reference(case), T.pre_reference(case, compute=torch.float32)
    assert r64["y"].shape == (T.PRE_B, case.Hp, case.Wp, 3)
    assert not r64["y"][:, case.H:].any() and not r64["y"][:, :, case.W:].any() and not r64["A"][:, case.H:].any()
    inside = r64["y"][:, :case.H, :case.W]
    assert bool((inside != 0).all()) and _no_subnormal(inside, F16)
    assert T.ratio(r32["y"].to(case.out_dt), r64["y"], r64["n"], r64["A"], case.out_dt) <= 1
    # a wrong reference: normalised with the mean of the next channel
    m = torch.tensor(T.PRE_MEAN, dtype=F32).double()
    s = torch.tensor(T.PRE_STD, dtype=F32).double()
    bad = r64["y"].clone()
    bad[:, :case.H, :case.W] = (T.nhwc(img.double()) / 255 - m.roll(1)) / s
    assert T.ratio(bad.to(case.out_dt), r64["y"], r64["n"], r64["A"], case.out_dt) > 1


# ---------------------------------------------------------------------------------------------- the wrap case, on the host
def test_up_wrap_inputs_have_one_sign_per_sum():
    """A = |ref| for the wrap case rests on this: x and dz carry the channel's sign sigma, w the sign tau; every magnitude >= 0.25"""
    inp = T.up_inputs(T.UP_WRAP_CASE, T.UP_WRAP_DTYPE)
    C = T.UP_WRAP_CASE.CV * T.VEC[T.UP_WRAP_DTYPE]
    sg, tau = T.chan_signs(C)
    sg16 = sg.to(F16)
    assert inp["skip"] is None and inp["x"].dtype == inp["dz"].dtype == F16
    assert bool((torch.sign(inp["x"]) == sg16).all()) and bool((torch.sign(inp["dz"]) == sg16).all())
    assert bool((torch.sign(inp["w"]) == tau.view(C, 1, 1, 1)).all())
    assert inp["x"].abs().min() >= 0.25 and inp["dz"].abs().min() >= 0.25 and inp["w"].abs().min() >= 0.25
    b0, y0 = T.up_wrap_tail(T.UP_WRAP_CASE)
    assert inp["x"][b0, y0:].abs().min() >= 0.25 * T.UP_WRAP_BOOST and inp["x"][b0, :y0].abs().max() <= 4
    assert inp["x"].abs().max() <= 4 * T.UP_WRAP_BOOST
    # a dw without the rows that only the wrapped pass of dwconvT_dw_kernel reaches breaks the bound (without the boost those rows
    # would be 0.4 % of every sum, below the 1.6 % that 2.6e5 roundings are allowed)
    ref = T.up_wrap_reference()
    assert ref["n_dw"].max() == 4 * 255 * 256 and (ref["n_dw"].max() + 2) * T.U32 > 0.0039 * 2
    assert _no_subnormal(ref["dx"], F16) and ref["n_dx"].max() == 16 and ref["n_dx"].min() == 9
    _, short, _, _ = T.up_bwd_by_taps(inp["x"][-1:], inp["dz"][-1:], inp["w"], T.UP_WRAP_CASE.f, skip_from=(0, y0))
    _, last, _, _ = T.up_bwd_by_taps(inp["x"][-1:], inp["dz"][-1:], inp["w"], T.UP_WRAP_CASE.f)
    assert T.ratio(ref["dw"] - last + short, ref["dw"], ref["n_dw"], ref["A_dw"], F32) > 1


# ------------------------------------------------------------------------------------------------- nothing is left out
def test_gpu_module_runs_every_case():
    import test_pointwise_gpu as G

    assert _params(G.test_maxpool, "case") == T.POOL_CASES and _params(G.test_maxpool_bwd, "case") == T.POOL_CASES
    assert _params(G.test_dwconvT_add, "case") == T.UP_FWD_CASES and _params(G.test_dwconvT_bwd, "case") == T.UP_BWD_CASES
    for fn in (G.test_global_avgpool, G.test_ese_scale, G.test_ese_dot, G.test_ese_bwd):
        assert _params(fn, "case") == T.ESE_CASES
    assert _params(G.test_depth_to_space2, "case") == T.D2S_CASES and _params(G.test_preprocess, "case") == T.PRE_CASES
    for fn in (G.test_maxpool, G.test_maxpool_bwd, G.test_dwconvT_add, G.test_dwconvT_bwd, G.test_global_avgpool, G.test_ese_scale,
               G.test_ese_dot, G.test_ese_bwd, G.test_depth_to_space2):
        assert _params(fn, "dt") == T.DTYPES
    assert any(m.name == "gpu" for m in (G.pytestmark if isinstance(G.pytestmark, list) else [G.pytestmark]))
