"""The optimizer-step case tables (tests/optimizer_cases.py) validated on the CPU: the tables reach the edges they are there
for, an unfused numpy f32 evaluation and torch.optim itself stay inside the derived tolerance, seeded wrong formulas fall
outside it, and the SGD launchers refuse what their float4 accesses cannot take.  Nothing here needs a GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

import optimizer_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------------
# the tables
# ------------------------------------------------------------------------------------------------------------------------
def test_main_run_table_has_its_edges():
    t = C.MAIN
    lens, ends = t.run_len, t.run_end
    assert set(lens) >= {1, 2, 3, 4, 5, 7, 8}
    assert lens[0] == 0 and lens[-1] == 0 and 0 in lens[1:-1]                  # zero length: first, middle, last
    assert {1023, 1024, 1025} <= set(ends)
    spans = [(e - l) // C.WG != (e - 1) // C.WG and (e - 1) // C.WG - (e - l) // C.WG >= 2 for l, e in zip(lens, ends) if l]
    assert any(spans)                                                          # one run over three workgroups
    assert t.n % 4 != 0 and 11 * C.WG < t.n <= 13 * C.WG
    assert ends[-1] == t.n and all(a <= b for a, b in zip(ends, ends[1:]))     # in contract: ascending, last == n
    assert len(C.LR_TABLE) == 3 and 0.0 in C.LR_TABLE and set(t.lr_index) == {0, 1, 2}
    assert any(C.LR_TABLE[i] == 0.0 and l > 0 for i, l in zip(t.lr_index, lens))
    assert all(a != b for a, b in zip(t.lr_index, t.lr_index[1:]))
    assert all((a == 0) != (b == 0) for a, b in zip(t.wd, t.wd[1:]))           # weight decay alternates zero / non-zero
    nonempty = [(i, w) for i, w, l in zip(t.lr_index, t.wd, lens) if l]
    assert all(a[0] != b[0] for a, b in zip(nonempty, nonempty[1:]))           # ... also across the empty runs
    assert (C.LEN1.n, C.LEN3.n) == (1, 3)
    for table in (C.MAIN, C.LEN1, C.LEN3, C.SMALL, C.CAPPED, C.CAPPED_SGD):
        assert all(f == C.f32(f) for f in list(C.LR_TABLE) + table.wd)          # the tables hold f32 values
    # the capped grids: `per` of the run kernels is 2048, two trips a thread; sgd_kernel's grid-stride loop wraps
    n = C.CAPPED.n
    nb = min((n + C.WG - 1) // C.WG, C.RUNS_GRID_CAP)
    assert nb == C.RUNS_GRID_CAP and (((n + nb - 1) // nb) + 1023) & ~1023 == 2048
    assert C.CAPPED_SGD.n == C.SGD_GRID_CAP * 256 + 5
    assert C.CAPPED.run_end[0] % 4 and C.CAPPED_SGD.run_end[0] % 4 and len(C.CAPPED.run_len) == 2


def test_launch_constants_match_the_source():
    import re
    src = open(os.path.join(ROOT, "detectron2-centernet_amd", "csrc", "train_ops.hip")).read()
    assert [int(x) for x in re.findall(r"if \(nb > (\d+)\) nb = \1;", src)] == [2048, 2048, 8192, 2048]
    assert "i += 1024" in src and "& ~1023L" in src
    from detectron2_centernet_amd import _lib
    from detectron2_centernet_amd.solver.build import GRAD_CHUNK
    assert GRAD_CHUNK == C.GRAD_CHUNK
    assert (_lib.CLIP_NONE, _lib.CLIP_VALUE, _lib.CLIP_NORM) == (C.CLIP_NONE, C.CLIP_VALUE, C.CLIP_NORM)
    assert (_lib.NORM_L1, _lib.NORM_L2, _lib.NORM_INF) == (C.NORM_L1, C.NORM_L2, C.NORM_INF)


def test_cases_cover_every_instantiation():
    for table in (C.MAIN, C.LEN1, C.LEN3):
        cs = [c for c in C.update_cases() if c.table is table]
        assert sum(c.kind == "sgd" for c in cs) == 1 and sum(c.kind == "sgd_runs" for c in cs) == 1
        assert len({(c.clip, c.nest) for c in cs if c.kind == "sgd_clip"}) == 5
        assert len({(c.clip, c.decoupled, c.amsgrad) for c in cs if c.kind == "adam"}) == 12
    names = [c.name for c in C.finite_small_cases() + C.nonfinite_cases() + C.capped_cases()]
    assert len(set(names)) == len(names)
    # norm clipping: coefficients of exactly 1 and below 1, one per run
    d = next(c for c in C.update_cases() if c.table is C.MAIN and c.clip == C.CLIP_NORM).inputs()
    live = np.asarray(C.MAIN.run_len) > 0
    assert (d["coefs"][live] == 1.0).any() and (d["coefs"][live] < 1.0).any() and len(d["coefs"]) == len(C.MAIN.run_len)
    # value clipping clamps some gradients and leaves others
    g = np.abs(next(c for c in C.update_cases() if c.table is C.MAIN and c.clip == C.CLIP_VALUE).inputs()["g"])
    assert (g > C.CLIP_VALUE_AT).mean() > 0.2 and (g < C.CLIP_VALUE_AT).mean() > 0.2 and (g == 0).any()
    # a first step over a momentum buffer full of NaN
    assert all(np.isnan(c.inputs()["m"]).all() for c in C.first_step_cases())
    assert {c.kind for c in C.first_step_cases()} == {"sgd", "sgd_runs", "sgd_clip"}
    # the hand-made Adam elements
    for c in C.adam_edge_cases():
        d, ref = c.inputs(), c.evaluate()
        for z in C.zero_slices():
            assert not d["g"][z].any() and not d["m"][z].any() and not d["v"][z].any() and not d["x"][z].any()
        s0 = C.SMALL.run_end[2] - C.SMALL.run_len[2]                             # the run without weight decay
        tiny = slice(s0 + C.ZERO_AT, s0 + C.TINY_AT)
        assert (ref["v"].v[tiny] > 0).all() and (np.sqrt(ref["v"].v[tiny]) * c.bias()[1] < 0.1 * C.EPS).all()   # eps dominates
        if c.amsgrad:
            x, v = d["x"].astype(np.float64), ref["v"].v
            assert (x > 2 * v).any() and (x < 0.5 * v).any() and ((x == v) & (d["m"] != 0)).any()
    assert {c.t for c in C.adam_edge_cases()} == {1, 10 ** 6} and C.adam_bias(10 ** 6, *C.BETAS) == (1.0, 1.0)
    assert C.adam_bias(1, *C.BETAS)[0] == pytest.approx(10.0) and C.SMALL.wd[0] != 0 and C.SMALL.wd[2] == 0
    for c in C.nonfinite_cases():
        g = c.inputs()["g"]
        assert np.isnan(g).sum() >= 1 and (g == np.inf).sum() >= 1 and (g == -np.inf).sum() >= 1


def test_nonfinite_definition():
    """value clipping leaves NaN as NaN and clamps +-inf to +-clip; the other elements are what they are without the
    non-finite ones; AMSGrad keeps a NaN of v or of vmax (torch.maximum)"""
    for c in C.nonfinite_cases():
        d, ref = c.inputs(), c.evaluate()
        clean = C.Case(c.kind, c.table, c.seed, nest=c.nest, clip=c.clip, decoupled=c.decoupled, amsgrad=c.amsgrad, t=c.t)
        cref = clean.evaluate()
        touched = sorted(set(C.NONFINITE_G) | (set(C.NONFINITE_V) | set(C.NONFINITE_X) if c.kind == "adam" else set()))
        rest = np.setdiff1d(np.arange(c.table.n), touched)
        for k in ref:
            assert np.array_equal(ref[k].v[rest], cref[k].v[rest]) and np.isfinite(ref[k].v[rest]).all()
        for i, val in C.NONFINITE_G.items():
            assert np.isnan(ref["m"].v[i]) == np.isnan(val) and np.isnan(ref["p"].v[i]) == np.isnan(val)
        if c.kind == "adam":
            for i in C.NONFINITE_V:
                assert np.isnan(ref["v"].v[i]) and np.isnan(ref["x"].v[i]) and np.isnan(ref["p"].v[i])
            for i in C.NONFINITE_X:
                assert np.isfinite(ref["v"].v[i]) and np.isnan(ref["x"].v[i]) and np.isnan(ref["p"].v[i])
        # the f32 emulation agrees on where the NaNs are (C.ratio asserts it) and is inside the tolerance elsewhere
        emu = c.evaluate(C.F32)
        assert max(C.ratio(emu[k].v, ref[k]) for k in ref) < 1.0


# ------------------------------------------------------------------------------------------------------------------------
# the tolerance: f32 emulation and torch inside, wrong formulas outside
# ------------------------------------------------------------------------------------------------------------------------
def _family(c):
    return c.kind + ("" if c.table.name in ("main", "len1", "len3") else "/" + c.table.name) + ("/first" if c.first else "")


def test_unfused_f32_evaluation_passes_every_case():
    worst = {}
    for c in C.finite_small_cases() + C.capped_cases():
        ref, emu = c.evaluate(), c.evaluate(C.F32)
        r = max(C.ratio(emu[k].v, ref[k]) for k in ref)
        worst[_family(c)] = max(worst.get(_family(c), 0.0), r)
        assert r < 1.0, (c.name, r)
        keep = c.exact_unchanged()
        assert np.array_equal(emu["p"].v[keep], c.inputs()["p"][keep])          # lr == 0: bit-equal
    for fam, r in sorted(worst.items()):
        print(f"numpy f32 / tolerance  {fam:24s} {r:.3f}")
    # an Adam element with g = m = v = 0: p unchanged (Adam without weight decay), p * keep (AdamW), exact
    for c in C.adam_edge_cases():
        emu = c.evaluate(C.F32)
        for z in C.zero_slices():
            want = c.zero_expected(z)
            if want is not None:
                assert np.array_equal(emu["p"].v[z], want) and not emu["m"].v[z].any() and not emu["v"].v[z].any()


def _torch_step(c):
    d, t = c.inputs(), c.table
    if c.kind == "sgd":
        bounds = [(0, t.n, C.LR_TABLE[0], C.WEIGHT_DECAY)]
    else:
        bounds = [(e - l, e, C.LR_TABLE[i], w) for l, e, i, w in zip(t.run_len, t.run_end, t.lr_index, t.wd) if l]
    params, groups = [], []
    for s, e, lr, wd in bounds:
        q = torch.nn.Parameter(torch.from_numpy(d["p"][s:e].copy()))
        q.grad = torch.from_numpy(d["g"][s:e].copy())
        if c.clip == C.CLIP_VALUE:
            torch.nn.utils.clip_grad_value_([q], c.clip_value, foreach=False)
        elif c.clip == C.CLIP_NORM:
            torch.nn.utils.clip_grad_norm_([q], c.clip_value, foreach=False)
        params.append((q, s, e))
        groups.append({"params": [q], "lr": lr, "weight_decay": wd})
    if c.kind == "adam":
        cls = torch.optim.AdamW if c.decoupled else torch.optim.Adam
        opt = cls(groups, lr=0.1, betas=C.BETAS, eps=C.EPS, amsgrad=c.amsgrad, foreach=False)
        for q, s, e in params:
            st = {"step": torch.tensor(float(c.t - 1)), "exp_avg": torch.from_numpy(d["m"][s:e].copy()),
                  "exp_avg_sq": torch.from_numpy(d["v"][s:e].copy())}
            if c.amsgrad:
                st["max_exp_avg_sq"] = torch.from_numpy(d["x"][s:e].copy())
            opt.state[q] = st
        keys = {"m": "exp_avg", "v": "exp_avg_sq", "x": "max_exp_avg_sq"}
    else:
        opt = torch.optim.SGD(groups, lr=0.1, momentum=C.MOMENTUM, nesterov=c.nest, foreach=False)
        if not c.first:
            for q, s, e in params:
                opt.state[q] = {"momentum_buffer": torch.from_numpy(d["m"][s:e].copy())}
        keys = {"m": "momentum_buffer"}
    opt.step()
    out = {"p": np.concatenate([q.detach().numpy() for q, _, _ in params])}
    for k, name in keys.items():
        if k == "x" and not c.amsgrad:
            continue
        out[k] = np.concatenate([opt.state[q][name].numpy() for q, _, _ in params])
    return out


def test_torch_optim_passes_every_finite_case():
    """torch.optim.SGD / Adam / AdamW in f32 on the CPU, one parameter group per run, the clipper called with one parameter at
    a time: the reference is torch's semantics, not only the formulas' of this module"""
    worst = {}
    for c in C.finite_small_cases():
        ref, got = c.evaluate(), _torch_step(c)
        assert set(got) == set(ref)
        r = max(C.ratio(got[k], ref[k]) for k in ref)
        worst[_family(c)] = max(worst.get(_family(c), 0.0), r)
        assert r < 1.0, (c.name, {k: C.ratio(got[k], ref[k]) for k in ref})
    for fam, r in sorted(worst.items()):
        print(f"torch.optim / tolerance {fam:24s} {r:.3f}")


def test_wrong_references_are_rejected():
    cases = C.finite_small_cases()
    for wrong in C.WRONG_SGD + C.WRONG_ADAM:
        kinds = ("adam",) if wrong in C.WRONG_ADAM and wrong != "neighbour_lr" else \
            (("sgd_runs", "sgd_clip", "adam") if wrong == "neighbour_lr" else ("sgd", "sgd_runs", "sgd_clip"))
        worst = (0.0, "")
        for c in cases:
            if c.kind not in kinds or (wrong == "bias_of_previous_step" and c.t == 1):
                continue
            ref, bad = c.evaluate(), c.evaluate(C.F32, wrong=wrong)
            worst = max(worst, (max(C.ratio(bad[k].v, ref[k]) for k in ref), c.name))
        print(f"wrong reference {wrong:24s} worst error / tolerance {worst[0]:.3g} ({worst[1]})")
        assert worst[0] > 1.0, (wrong, worst)
    assert set(C.WRONG) <= set(C.WRONG_SGD + C.WRONG_ADAM) and len(C.WRONG) == 8


def test_adam_bound_on_200k_elements():
    """the bound at scale: 200 k elements, gradients over five decades, zeros in g, m and v, Adam / AdamW with and without
    AMSGrad.  The unfused f32 evaluation uses about half the tolerance on every buffer; 1.f - (float)beta2, eps inside the
    square root and a missing running maximum are each far outside it."""
    big = C.RunTable("big", [200000], wd=[C.WEIGHT_DECAY])
    for decoupled in (False, True):
        for amsgrad in (False, True):
            c = C.Case("adam", big, 600, decoupled=decoupled, amsgrad=amsgrad)
            ref, emu = c.evaluate(), c.evaluate(C.F32)
            rs = {k: C.ratio(emu[k].v, ref[k]) for k in ref}
            print(f"adam 200k w={int(decoupled)} ams={int(amsgrad)} f32 / tolerance", {k: round(r, 3) for k, r in rs.items()})
            assert max(rs.values()) < 1.0 and min(rs.values()) > 0.25            # a bound, and not a loose one
            for wrong, least in (("omb2_in_f32", 2.0), ("eps_in_sqrt", 1e3), ("no_running_max", 1e3)):
                if wrong == "no_running_max" and not amsgrad:
                    continue
                bad = c.evaluate(C.F32, wrong=wrong)
                rb = {k: C.ratio(bad[k].v, ref[k]) for k in ref}
                print(f"   {wrong:16s}", {k: float(f"{r:.3g}") for k, r in rb.items()})
                assert max(rb.values()) > least, (wrong, rb)


# ------------------------------------------------------------------------------------------------------------------------
# the norm kernels' tables and bound
# ------------------------------------------------------------------------------------------------------------------------
def _chunk_partial_f32(g, s, l, norm_type):
    """grad_chunk_norm_kernel's summation shape in numpy f32: a thread's elements in address order on the float4 grid anchored
    below the start, the xor butterfly of a wave, the four waves left to right"""
    a = s & ~3
    trips = -(-(s + l - a) // 1024)
    buf = np.zeros(trips * 1024, dtype=np.float32)
    buf[s - a:s - a + l] = np.abs(g[s:s + l])
    term = buf * buf if norm_type == C.NORM_L2 else buf
    acc = np.zeros(256, dtype=np.float32)
    for t in term.reshape(trips, 256, 4):
        for k in range(4):
            acc = acc + t[:, k]
    lane = np.arange(256)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[lane ^ o]
    return ((acc[0] + acc[64]) + acc[128]) + acc[192]


def test_norm_tables_and_bound():
    from detectron2_centernet_amd.solver.build import grad_chunks
    offsets = C.norm_offsets()
    starts, lens, ends = grad_chunks(offsets)
    lengths = C.NORM_PARAM_LENGTHS
    assert set(lengths) >= {0, 1, 2, 3, 4, 5, 4095, 4096, 4097, 64 * 4096, 64 * 4096 + 1}
    assert {off % 4 for off, n in offsets if n} == {0, 1, 2, 3}
    assert {off % 4 for off, n in offsets if n >= 4095} >= {2, 3}               # the chunked ones off the float4 grid
    per_param = np.diff([0] + ends)
    assert dict(zip(lengths, per_param))[64 * 4096] == 64 and dict(zip(lengths, per_param))[64 * 4096 + 1] == 65
    assert dict(zip(lengths, per_param))[0] == 0 and ends[-1] == len(starts) and lengths[-1] == 0
    assert C.coef_depth(64) == 7 and C.coef_depth(65) == 8 and C.coef_depth(0) == 6
    rng = np.random.default_rng(700)
    g = (rng.standard_normal(C.norm_total()) * 10.0 ** rng.uniform(-3, 1, C.norm_total())).astype(np.float32)
    for nt in (C.NORM_L1, C.NORM_L2):
        ref = C.chunk_partials_ref(g, starts, lens, nt)
        emu = np.array([_chunk_partial_f32(g, s, l, nt) for s, l in zip(starts, lens)])
        r = C.ratio(emu, ref)
        print(f"chunk partials, numpy f32 in the kernel's shape / tolerance, norm type {nt}: {r:.3f}")
        assert r < 1.0
        # a dropped element of a short chunk is far outside
        short = [c for c, l in enumerate(lens) if 2 <= l <= 5]
        drop = np.array([_chunk_partial_f32(g, starts[c] + 1, lens[c] - 1, nt) for c in short])
        sub = C.EV(ref.v[short], ref.e[short])
        assert (np.abs(drop - sub.v) > C.tolerance(sub)).all()
        # pass 2 from f32 partials, lane l taking l, l + 64, ..; torch's clip_grad_norm_ per parameter agrees with it
        part = emu.astype(np.float32)
        norm, coef = C.coefs_ref(part, ends, nt, C.CLIP_NORM_AT)
        first = 0
        for q, last in enumerate(ends):
            acc = np.zeros(64, dtype=np.float32)
            for c in range(first, last):
                acc[(c - first) % 64] += part[c]
            lane = np.arange(64)
            for o in (32, 16, 8, 4, 2, 1):
                acc = acc + acc[lane ^ o]
            n32 = np.sqrt(acc[0]) if nt == C.NORM_L2 else acc[0]
            c32 = min(np.float32(1.0), np.float32(C.CLIP_NORM_AT) / (n32 + np.float32(1e-6)))
            sub_n, sub_c = C.EV(norm.v[q], norm.e[q]), C.EV(coef.v[q], coef.e[q])
            assert C.ratio(n32, sub_n) < 1.0 and C.ratio(c32, sub_c) < 1.0, (nt, q)
            s, n = offsets[q]
            tn = torch.linalg.vector_norm(torch.from_numpy(g[s:s + n]).double(), 1 if nt == C.NORM_L1 else 2).item()
            assert abs(tn - norm.v[q]) <= 1e-5 * tn + 1e-30                    # the f32 partials against f64 of the elements
            first = last
    # clip value below 1e-6 on a zero norm: clip / 1e-6 < 1 inside the running bound
    norm, coef = C.coefs_ref(np.zeros(len(starts)), ends, C.NORM_L2, 5e-7)
    assert not norm.v.any() and (np.abs(coef.v - 0.5) < 1e-6).all() and (coef.e > 0).all() and (coef.e < 1e-6).all()
    norm, coef = C.coefs_ref(np.zeros(len(starts)), ends, C.NORM_L2, 1.0)
    assert np.array_equal(coef.v, np.ones(len(ends)))


def test_adam_bias_formula():
    for t in (1, 2, 10, 11, 10 ** 6 + 1, 2 ** 31 + 1):
        b = C.adam_bias(t, *C.BETAS)
        assert b[0] >= 1.0 and b[1] >= 1.0
        if t > 10 ** 6:
            assert b == (1.0, 1.0)


# ------------------------------------------------------------------------------------------------------------------------
# the C ABI: the SGD launchers refuse what their float4 accesses cannot take
# ------------------------------------------------------------------------------------------------------------------------
def test_sgd_launchers_refuse_misaligned_and_negative():
    from detectron2_centernet_amd import _lib
    l = _lib.lib()
    assert l.ctdet_abi_version() == 8                                           # no signature changed
    ok, off = ctypes.c_void_p(16), ctypes.c_void_p(20)
    # argument checks come before any device work: none of these calls reaches a launch
    for which in range(3):
        bufs = [off if k == which else ok for k in range(3)]
        assert l.ctdet_sgd_momentum_runs(*bufs, 4, ok, ok, ok, ok, 1, 0.9, 0, None) == -22
        assert b"aligned" in l.ctdet_last_error()
        assert l.ctdet_sgd_momentum_runs_clip(*bufs, 4, ok, ok, ok, ok, 1, 0.9, 0, 1, _lib.CLIP_VALUE, 1.0, None, None) == -22
        assert b"aligned" in l.ctdet_last_error()
    assert l.ctdet_sgd_momentum_runs(ok, ok, ok, -1, ok, ok, ok, ok, 1, 0.9, 0, None) == -22
    assert b"n=-1" in l.ctdet_last_error()
    assert l.ctdet_sgd_momentum_runs(ok, ok, ok, 4, ok, ok, ok, ok, -1, 0.9, 0, None) == -22
    assert b"nruns=-1" in l.ctdet_last_error()
    assert l.ctdet_sgd_momentum_runs_clip(ok, ok, ok, -4, ok, ok, ok, ok, 1, 0.9, 0, 0, _lib.CLIP_NONE, 0.0, None, None) == -22
    assert b"n=-4" in l.ctdet_last_error()
    assert l.ctdet_sgd_momentum_runs_clip(ok, ok, ok, 4, ok, ok, ok, ok, -2, 0.9, 0, 0, _lib.CLIP_NONE, 0.0, None, None) == -22
    assert b"nruns=-2" in l.ctdet_last_error()
    # the scalar kernel asks no alignment, only a count that is one
    assert l.ctdet_sgd_momentum(off, off, off, -1, ok, 0.9, 0.0, 0, None) == -22 and b"n=-1" in l.ctdet_last_error()
    # in contract and empty: accepted without a launch
    assert l.ctdet_sgd_momentum(off, off, off, 0, ok, 0.9, 0.0, 0, None) == 0
    assert l.ctdet_sgd_momentum_runs(ok, ok, ok, 0, ok, ok, ok, ok, 0, 0.9, 0, None) == 0
    assert l.ctdet_sgd_momentum_runs_clip(ok, ok, ok, 0, ok, ok, ok, ok, 0, 0.9, 0, 1, _lib.CLIP_VALUE, 1.0, None, None) == 0
    # ctdet_adam_runs' refusals, which these now match
    assert l.ctdet_adam_runs(off, ok, ok, ok, None, 4, ok, ok, ok, ok, 1, ok, 0.9, 0.999, 1e-8, 0, 0, 0, 0.0, None, None) == -22
    assert b"aligned" in l.ctdet_last_error()
    header = open(os.path.join(ROOT, "include", "ctdet_hip.h")).read()
    assert header.count("16-byte aligned") >= 3
