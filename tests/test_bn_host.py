"""The case tables of bn_cases.py against their own conditions, without a GPU: the mirrored launch constants match train_bwd.hip,
every shape takes the branch it is listed for (computed from those constants), the strided cases have pairwise different strides and
an offset slice, the special z values and channels are in place, the same formulas in f32 on the CPU meet every bound against the
float64 reference (the bounds are attainable) and stay under the ceiling of test_syncbn_gpu.py, the float64 reference agrees with
float64 F.batch_norm under autograd, every deliberately wrong reference breaks its bound or its equality on a listed case, and
nothing is filtered out on the way to the GPU tests."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import bn_cases as T

F16, F32 = T.F16, T.F32
PLAIN = [c for c in T.BN_CASES if not c.strided]


def _params(fn, name):
    return [p for m in fn.pytestmark if m.name == "parametrize" and m.args[0] == name for p in m.args[1]]


def test_mirrored_constants_match_the_source():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "detectron2-centernet_amd", "csrc", "train_bwd.hip")).read()
    for name in ("AA_ROWS", "BN_ROWS", "SB_ROWS"):
        assert int(re.search(rf"constexpr int {name} = (\d+);", src).group(1)) == getattr(T, name)
    body = src[src.index("static int chan_blocks("):src.index("static int launch_bn_train_fwd_t")]
    assert f"const int rows = {T.BLOCK} / (C / N);" in body
    assert f"long nb = ((long)M + rows * {T.CHAN_ROWS} - 1) / (rows * {T.CHAN_ROWS});" in body
    assert f"if (nb > {T.CHAN_BLOCK_CAP}) nb = {T.CHAN_BLOCK_CAP};" in body
    assert f"(size_t)({T.CHAN_BLOCK_CAP} * 2 + 2) * C * sizeof(float)" in src
    assert f"return (float*)b.workspace + (size_t){T.CHAN_BLOCK_CAP} * 2 * b.C;" in src      # the sums slot behind the partials
    red = src[src.index("void __launch_bounds__(256) chan_reduce_kernel"):src.index("chan_finalize_kernel(")]
    assert f"const int rows_per_pass = {T.BLOCK} / CV;" in red
    assert "for (; m + 3 * step < a.M; m += 4 * step)" in red and T.UNROLL[0] == 4
    assert "for (; m + step < a.M; m += 2 * step)" in red and T.UNROLL[1] == 2
    # the channel-count check stands once, in the helper that every launcher calls before it launches anything
    check = src[src.index("static int bn_check("):src.index("static float* bn_sums_slot(")]
    assert f"CTDET_CHECK(C % N == 0 && C / N <= {T.CV_MAX}," in check and src.count("CTDET_CHECK(C % N == 0 && C / N <=") == 1
    for fn in ("bn_train_fwd", "bn_train_bwd", "bn_local_stats", "bn_sync_fwd", "bn_local_grad_sums", "bn_sync_bwd"):
        launcher = src[src.index(f"static int launch_{fn}_t("):]
        launcher = launcher[:launcher.index("CTDET_LAUNCH_CHECK();")]
        assert "if (const int e = bn_check<T>(" in launcher and launcher.index("bn_check<T>(") < launcher.index("hipLaunchKernelGGL") and \
            ("bn_chan_reduce" not in launcher or launcher.index("bn_check<T>(") < launcher.index("bn_chan_reduce")), fn
    assert "struct VecT<f16> { typedef f16x8 type; static constexpr int N = 8; }" in src and T.VEC[F16] == 8
    assert "struct VecT<float> { typedef f32x4 type; static constexpr int N = 4; }" in src and T.VEC[F32] == 4
    assert src.count("__launch_bounds__(256) ") >= 9 and "dim3(256), 0, s, a);" in src
    assert f"256L * SB_ROWS - 1) / (256L * SB_ROWS)" in src and "const long ppb = (256 >> sh) * AA_ROWS;" in src
    assert "const long ppb = (256 >> sh) * BN_ROWS;" in src
    assert "const double unbiased = M > 1 ? var * M / (M - 1) : var;" in src and "if (!(nb > 0)) continue;" in src


def test_table_takes_the_branches_it_names():
    by = {(c.CV, c.M): c for c in PLAIN}
    assert len(by) == len(PLAIN)
    assert {(1, 1), (1, 2), (1, 255)} <= set(by)
    assert T.chan_profile(1, 1, 0) == {"idle": True, "loops": {(0, 1)}} and sum(k > 0 for k in T.chan_lanes(1, 1)) == 1
    assert sum(k == 0 for k in T.chan_lanes(255, 1)) == 1 and sum(k == 0 for k in T.chan_lanes(2, 1)) == 254
    assert T.is_pow2(T.CV_POW2) and not T.is_pow2(T.CV_ODD) and T.BLOCK % T.CV_ODD
    for CV in (T.CV_POW2, T.CV_ODD):
        r = T.rows_per_pass(CV)
        want = {r - 1: (True, {(0, 1)}, {(0, 1)}), r: (False, {(0, 1)}, {(0, 1)}),
                4 * r: (False, {(1, 0)}, {(2, 0)}), 5 * r: (False, {(1, 1)}, {(2, 1)}),
                6 * r: (False, {(1, 2)}, {(3, 0)}), 7 * r: (False, {(1, 3)}, {(3, 1)})}
        for M, (idle, l0, l1) in want.items():
            assert (CV, M) in by
            p0, p1 = T.chan_profile(M, CV, 0), T.chan_profile(M, CV, 1)
            assert (p0["idle"], p0["loops"], p1["loops"]) == (idle, l0, l1), (CV, M, p0, p1)
            assert T.chan_blocks(M, CV) == 1
        assert T.chan_blocks(16 * r, CV) == 2 and T.chan_blocks(16 * r + 1, CV) == 3 and {(CV, 16 * r), (CV, 16 * r + 1)} <= set(by)
        assert T.chan_profile(16 * r, CV, 0)["loops"] == {(2, 0)} and T.chan_profile(16 * r + 1, CV, 1)["loops"] == {(3, 0), (2, 1)}
        # the sync apply kernels: two full workgroups / a ragged last one; the generic kernels: threads past M * CV
        (g0, gx0), (s0, sx0) = T.apply_blocks(16 * r, CV)
        (g1, gx1), (s1, sx1) = T.apply_blocks(16 * r + 1, CV)
        assert s0 == 2 and s1 in (2, 3) and sx1 > 0 and (16 * r + 1) * CV % T.BLOCK
        if not T.is_pow2(CV):
            assert gx0 > 0 and gx1 > 0 and sx0 > 0 and g0 > 1
    # the rows kernels: fast path only at ppb * 8 * k, one tail row more at + 1, tail only below one workgroup's span
    r = T.rows_per_pass(T.CV_POW2)
    assert T.AA_ROWS == T.BN_ROWS and T.rows_kernel_split(16 * r, T.CV_POW2) == (16 * r, 0)
    assert T.rows_kernel_split(16 * r + 1, T.CV_POW2) == (16 * r, 1)
    assert T.rows_kernel_split(7 * r, T.CV_POW2) == (0, 7 * r) and T.rows_kernel_split(1, 1) == (0, 1)
    # the 1024-block cap: reached by exactly one case, at the smallest M that the cap binds for, with rows_per_pass = 1
    capped = [c for c in PLAIN if T.chan_blocks(c.M, c.CV) == T.CHAN_BLOCK_CAP]
    assert len(capped) == 1 and capped[0].CV == T.CV_MAX and T.rows_per_pass(T.CV_MAX) == 1
    M = capped[0].M
    assert -(-M // T.CHAN_ROWS) > T.CHAN_BLOCK_CAP and -(-(M - 1) // T.CHAN_ROWS) == T.CHAN_BLOCK_CAP
    assert set(T.chan_lanes(M, T.CV_MAX)) == {8, 9} and T.channels(capped[0], F16) == 2048 and T.channels(capped[0], F32) == 1024
    assert all(c.M <= 16 * T.rows_per_pass(1) for c in T.BN_CASES if c.CV != T.CV_MAX)
    # the settings all occur
    for field, vals in (("eps", {1e-5, 1e-3}), ("momentum", {0.1, 0.03}), ("grad_mult", {1.0, 0.25}), ("into", {"both", "dgamma", "none"}),
                        ("res", {True, False}), ("relu", {True, False})):
        assert {getattr(c, field) for c in T.BN_CASES} == vals
    for CV in (T.CV_POW2, T.CV_ODD):
        assert {c.relu for c in T.NOSTAT_CASES if c.CV == CV} == {True, False}
    assert {c.grad_mult for c in T.NOSTAT_CASES} == {1.0, 0.25}
    assert all(c.M >= 2 for c in T.HAND_CASES) and len(T.HAND_CASES) == len(T.BN_CASES) - 2
    assert T.rank_rows(1, 3) == [1, 0, 0] and T.rank_rows(7, 3) == [3, 2, 2]


@pytest.mark.parametrize("dt", T.DTYPES, ids=T.dt_name)
def test_strided_cases(dt):
    st = [c for c in T.BN_CASES if c.strided]
    assert {c.CV for c in st} == {T.CV_POW2, T.CV_ODD} and {c.CV for c in T.NOSTAT_CASES if c.strided} == {T.CV_POW2, T.CV_ODD}
    N = T.VEC[dt]
    for c in st:
        C = T.channels(c, dt)
        assert c.M > 1 and c.res and c.relu
        for group in (("y", "res", "z"), ("dz", "zin", "y", "dy", "dres")):      # the tensors of one entry point
            s = [T.stride_of(k, C, dt) for k in group]
            assert len(set(s)) == len(s) and all(v % N == 0 and v >= C + N for v in s)
            assert any(T.offset_of(k, dt) == N for k in group) and all(T.offset_of(k, dt) in (0, N) for k in group)
        buf, view = T.slab(T.bn_inputs(c, dt)["y"], "y", dt)
        assert torch.equal(view, T.bn_inputs(c, dt)["y"]) and buf.shape == (c.M + T.GUARD_ROWS, T.stride_of("y", C, dt))
        bits = buf.view(torch.int16 if dt == F16 else torch.int32)
        assert bool((bits[:, :N] == T.SENTINEL[dt]).all()) and bool((bits[:, N + C:] == T.SENTINEL[dt]).all())
        assert bool((bits[c.M:] == T.SENTINEL[dt]).all())
        # the guard rows hold every row that the threads past M * CV of a generic kernel would touch, and the row that a
        # chan_reduce loop running one step too far would add
        assert T.GUARD_ROWS * c.CV >= T.BLOCK and T.apply_blocks(c.M, c.CV)[0][1] < T.GUARD_ROWS * c.CV
    odd = [c for c in st if c.CV == T.CV_ODD][0]
    assert T.chan_profile(odd.M, odd.CV, 0)["loops"] == {(1, 3)} and T.apply_blocks(odd.M, odd.CV)[0][1] > 0
    r = T.rows_per_pass(T.CV_ODD)
    assert T.rank_rows(14 * r, 2) == [7 * r, 7 * r] and any(c.M == 14 * r and c.CV == T.CV_ODD for c in T.BN_CASES)


@pytest.mark.parametrize("dt", T.DTYPES, ids=T.dt_name)
@pytest.mark.parametrize("case", T.BN_CASES, ids=T.bn_id)
def test_case_holds_what_it_promises(case, dt):
    inp = T.bn_inputs(case, dt)
    M, C = case.M, T.channels(case, dt)
    y = inp["y"].double()
    assert all(inp[k].dtype == dt and inp[k].shape == (M, C) for k in ("y", "dz", "zin")) and (inp["res"] is not None) == case.res
    assert bool((y[:, 0] == 1.5).all()) and y[:, 1].sum().item() == 0.0
    fw = T.fwd_reference(case, dt)
    assert fw["var"][0].item() == 0 and fw["invstd"][0].item() == pytest.approx(T.f32v(case.eps) ** -0.5, rel=1e-12)
    assert fw["mean"][1].item() == 0
    if M >= 64:
        sd = fw["var"].sqrt()
        if dt == F32:
            assert 500 < (fw["mean"][2].abs() / sd[2]).item() < 2000
        rest = torch.arange(C) >= 3
        assert bool((fw["mean"].abs()[rest] <= sd[rest]).all()) and bool(T.eligible(case, dt)[rest].all()) and M >= T.CEIL_MIN_ROWS
    assert not bool((inp["rm0"] == 0).any()) and not bool((inp["rv0"] == 1).any()) and bool((inp["gamma"] < 0).any())
    # the hand-built z: every special value, the subnormals really subnormal, one NaN per seven elements
    z = inp["zin"]
    k = torch.tensor([(m + c) % 7 for m in range(min(M, 7)) for c in range(C)]).view(-1, C)
    zz = z[:k.shape[0]]
    s = T.SUBNORMAL[dt]
    assert torch.finfo(dt).smallest_normal > s > 0 and torch.tensor(s, dtype=dt).item() == s and torch.tensor(s / 2, dtype=dt).item() == 0
    assert bool(torch.isnan(zz[k == 3]).all()) and int(torch.isnan(z).sum()) == int((((torch.arange(M)[:, None] + torch.arange(C)) % 7) == 3).sum())
    for idx, v, neg in ((0, 0.0, False), (1, s, False), (2, 0.0, True), (4, 1.0, False), (5, -s, True), (6, -1.0, True)):
        assert bool((zz[k == idx].double() == v).all()) and bool((torch.signbit(zz[k == idx]) == neg).all())
    assert {0, 1, 2, 3} <= set(k.unique().tolist())          # even one row of one f32 vector holds +0, the subnormal, -0 and NaN
    if M >= 7:
        assert set(k[:, 0].tolist()) == set(range(7))


@pytest.mark.parametrize("world", T.WORLDS)
@pytest.mark.parametrize("dt", T.DTYPES, ids=T.dt_name)
@pytest.mark.parametrize("case", T.BN_CASES, ids=T.bn_id)
def test_f32_torch_meets_every_bound(case, dt, world):
    parts = T.rank_rows(case.M, world)
    em = T.emulate(case, dt, parts)
    fw, fb = T.fwd_reference(case, dt), T.fwd_bounds(case, dt, parts)
    bw, bb = T.bwd_reference(case, dt), T.bwd_bounds(case, dt, parts)
    rs = {k: T.ratio(em[k], fw[k], fb[k]) for k in ("mean", "invstd", "scale", "z", "rm", "rv")}
    rs["dy"] = T.ratio(em["dy"], bw["dy"], bb["dy"])
    for r, (ref, b, got) in enumerate(zip(T.local_sums(case, dt, parts), bb["local"], em["local"])):
        if parts[r]:
            rs[f"dbeta{r}"], rs[f"dgamma{r}"] = T.ratio(got[0], ref[0], b[0]), T.ratio(got[1], ref[1], b[1])
    assert all(v <= 1 for v in rs.values()), rs
    assert torch.equal(em["dres"], bw["g"])
    # the ceiling of test_syncbn_gpu.py, over the channels it speaks about
    ok = T.eligible(case, dt)
    if world == 1 and bool(ok.any()):
        rel = lambda b, ref: (b[..., ok].max() / ref[..., ok].abs().max()).item()
        assert rel(fb["invstd"], fw["invstd"]) <= T.CEIL["invstd"][dt]
        assert rel(fb["z"], fw["z"]) <= T.CEIL["z"][dt]
        assert rel(bb["dy"], bw["dy"]) <= T.CEIL["grad"][dt]
        ref = T.local_sums(case, dt, parts)[0]
        assert rel(bb["local"][0][0], ref[0]) <= T.CEIL["grad"][dt] and rel(bb["local"][0][1], ref[1]) <= T.CEIL["grad"][dt]


@pytest.mark.parametrize("dt", T.DTYPES, ids=T.dt_name)
@pytest.mark.parametrize("case", [c for c in T.BN_CASES if c.M > 1], ids=T.bn_id)
def test_reference_agrees_with_float64_autograd(case, dt):
    inp, fw, bw = T.bn_inputs(case, dt), T.fwd_reference(case, dt), T.bwd_reference(case, dt)
    y = inp["y"].double().requires_grad_(True)
    gamma, beta = inp["gamma"].double().requires_grad_(True), inp["beta"].double().requires_grad_(True)
    rm, rv = inp["rm0"].double().clone(), inp["rv0"].double().clone()
    out = F.batch_norm(y, rm, rv, gamma, beta, True, T.f32v(case.momentum), T.f32v(case.eps))
    z = out + inp["res"].double() if case.res else out
    z = z.clamp_min(0.0) if case.relu else z
    close = lambda a, b, tol: (a - b).abs().max().item() <= tol * max(1e-300, b.abs().max().item())
    assert close(fw["z"], z.detach(), 1e-12) and close(fw["rm"], rm, 1e-13) and close(fw["rv"], rv, 1e-12)
    out.backward(bw["g"].double())           # g = dz * (z > 0) on the hand-built z enters BatchNorm's output
    # the backward reference starts from the f32-rounded statistics: 2^-24 relative in mean and invstd
    assert close(bw["dy"], y.grad, 1e-4) and close(bw["s0"], beta.grad, 1e-12) and close(bw["s1"], gamma.grad, 1e-4)


def _breaks(case, dt, parts=None):
    parts = parts or [case.M]
    return T.fwd_reference(case, dt), T.fwd_bounds(case, dt, parts), T.bwd_reference(case, dt), T.bwd_bounds(case, dt, parts)


@pytest.mark.parametrize("dt", T.DTYPES, ids=T.dt_name)
def test_wrong_references_are_told_apart(dt):
    many = [c for c in PLAIN if 2 <= c.M <= 2000]
    # unbiased variance in the output; biased variance in the running statistics; dy without its sum g * xhat term
    for c in many:
        fw, fb, bw, bb = _breaks(c, dt)
        assert T.ratio(T.fwd_reference(c, dt, "unbiased_out")["z"], fw["z"], fb["z"]) > 1, c
        assert T.ratio(T.fwd_reference(c, dt, "unbiased_out")["invstd"], fw["invstd"], fb["invstd"]) > 1, c
        assert T.ratio(T.fwd_reference(c, dt, "biased_running")["rv"], fw["rv"], fb["rv"]) > 1, c
        assert T.ratio(T.bwd_reference(c, dt, "drop_xhat")["dy"], bw["dy"], bb["dy"]) > 1, c
        # mask z >= 0 instead of z > 0: +0.0 and -0.0 let dz through
        if c.relu:
            assert not torch.equal(T.bwd_reference(c, dt, "mask_ge")["g"], bw["g"]), c
        # global instead of local sums in the SyncBN dgamma
        parts = T.rank_rows(c.M, 2)
        loc, glob, b = T.local_sums(c, dt, parts), T.local_sums(c, dt, parts, global_dgamma=True), T.bwd_bounds(c, dt, parts)["local"]
        assert T.ratio(glob[0][1], loc[0][1], b[0][1]) > 1, c
        # an empty slot counted as a rank (one row of zeros)
        slots = T.rank_slots(c, dt, parts)
        for order in ([slots[0], T.rank_slots(c, dt, [0])[0], slots[1]], [T.rank_slots(c, dt, [0])[0], slots[0], slots[1]]):
            n, mean, var = T.combine_slots(order)
            assert n == c.M and (mean - fw["mean"]).abs().max() <= 1e-12 * (1 + fw["mean"].abs().max()) and (var - fw["var"]).abs().max() <= 1e-12 * (1 + fw["var"].abs().max())
            _, wm, _ = T.combine_slots(order, count_empty=True)
            assert T.ratio(wm, fw["mean"], T.fwd_bounds(c, dt, parts)["mean"]) > 1, c
    for c in T.NOSTAT_CASES:
        if c.relu:
            assert not torch.equal(T.nostat_reference(c, dt, ge=True)["dy"], T.nostat_reference(c, dt)["dy"])
    # a stride of one tensor applied to another: z read with dz's pixel stride
    for c in [c for c in T.BN_CASES if c.strided]:
        inp = T.bn_inputs(c, dt)
        M, C = inp["zin"].shape
        buf, view = T.slab(inp["zin"], "zin", dt)
        off = T.offset_of("zin", dt)
        right = T.read_strided(buf, off, T.stride_of("zin", C, dt), M, C)
        wrong = T.read_strided(buf, off, T.stride_of("dz", C, dt), M, C)
        assert torch.equal(right.view(torch.int16 if dt == F16 else torch.int32), inp["zin"].view(torch.int16 if dt == F16 else torch.int32))
        dz = inp["dz"]
        g_wrong = torch.where(T.mask_of(wrong, True), dz, torch.zeros_like(dz))
        assert not torch.equal(g_wrong, T.bwd_reference(c, dt)["g"])


def test_nothing_is_filtered_on_the_way_to_the_gpu():
    import test_bn_gpu as G

    for fn in (G.test_fused_forward, G.test_fused_backward, G.test_split_simulated_ranks, G.test_world_one_equals_fused):
        assert _params(fn, "case") == T.BN_CASES and _params(fn, "dt") == T.DTYPES
    assert _params(G.test_split_simulated_ranks, "world") == list(T.WORLDS) == [1, 2, 3]
    assert _params(G.test_fused_backward_without_statistics, "case") == T.NOSTAT_CASES
    assert _params(G.test_empty_slot_changes_nothing, "case") == T.HAND_CASES
    assert _params(G.test_empty_slot_changes_nothing, "where") == list(T.HAND_SLOTS) == ["empty_middle", "empty_first", "empty_middle_nan"]
    assert T.HAND_POISON == {"empty_middle_nan": 1} and 1 not in T.HAND_SLOTS["empty_middle_nan"]
    assert len(set(T.BN_CASES)) == len(T.BN_CASES) and len(set(T.NOSTAT_CASES)) == len(T.NOSTAT_CASES)
