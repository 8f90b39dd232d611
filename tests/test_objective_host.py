"""The case tables of objective_cases.py against their own conditions, with the references alone and without a GPU: every shape
takes the branch it is there for, every promised positive / pinned logit / edge entry is in place, nothing is filtered out on the
way to the GPU tests, and the float64 oracle agrees with the float32 oracle on every case (the guard of the reference)."""
import math

import numpy as np
import pytest
import torch

import objective_cases as T
from oracle import ctdet_oracle as O


def _params(fn):
    return [p for m in fn.pytestmark if m.name == "parametrize" for p in m.args[1]]


# --------------------------------------------------------------------------------------------------------------- focal
def test_focal_shapes_and_block_counts():
    assert [tuple(c[:4]) for c in T.FOCAL_CASES] == [s for s in T.FOCAL_SHAPES for _ in (0, 1)]
    assert len(T.FOCAL_CASES) == 14 and sum(c.with_pos for c in T.FOCAL_CASES) == 7 and sum(c.pinned for c in T.FOCAL_CASES) == 1
    numel = {s: s[0] * s[1] * s[2] * s[3] for s in T.FOCAL_SHAPES}
    assert list(numel.values()) == [60, 60, 1512, 300, 224, 25600, 2100800]
    assert all(n % 4 == 0 for n in numel.values())
    assert math.prod(T.FOCAL_RAISES) == 105
    blocks = {s: -(-(n // 4) // T.FL_VEC_PER_BLOCK) for s, n in numel.items()}
    ragged = {s: (n // 4) % T.FL_VEC_PER_BLOCK != 0 for s, n in numel.items()}
    assert blocks[(1, 80, 16, 20)] == 4 and ragged[(1, 80, 16, 20)]
    big = (2, 80, 101, 130)
    assert numel[big] // 4 == 525200 and blocks[big] == 257 == T.FL_FINALIZE_THREADS + 1 and ragged[big]
    # the smallest such map of the model's class count: one row or one column less fits into 256 blocks
    assert -(-(2 * 80 * 100 * 130 // 4) // T.FL_VEC_PER_BLOCK) <= 256 and -(-(2 * 80 * 101 * 129 // 4) // T.FL_VEC_PER_BLOCK) <= 256
    assert {s[1] for s in T.FOCAL_SHAPES if s[1] < 4} == {1, 2, 3} and {s[1] for s in T.FOCAL_SHAPES if s[1] % 4} == {1, 2, 3, 5, 7}


@pytest.mark.parametrize("case", T.FOCAL_CASES, ids=T.focal_id)
def test_focal_case_holds_what_it_promises(case):
    inp = T.focal_inputs(case)
    C = case.C
    logits, gt, alpha, marks = inp["logits"].reshape(-1), inp["gt"].reshape(-1), inp["alpha"], inp["marks"]
    assert inp["logits"].shape == (case.B, case.H, case.W, C) and logits.dtype == gt.dtype == alpha.dtype == torch.float32
    assert len(set(alpha.tolist())) == C and sorted(alpha.tolist()) == [np.float32(0.25 + k / C) for k in range(C)]
    assert C < 3 or alpha.tolist() != sorted(alpha.tolist()), "alpha is not shuffled"
    assert float(gt.min()) >= 0 and float(gt.max()) <= 1
    pinned = [marks[k] for k in ("pin_pos", "pin_neg") if k in marks]
    rest = torch.ones_like(logits, dtype=torch.bool)
    rest[pinned] = False
    assert float(((logits[rest].abs() - T.CLAMP_LOGIT).abs()).min()) >= T.CLAMP_MARGIN
    assert math.isclose(1 / (1 + math.exp(-T.CLAMP_LOGIT)), 1 - 1e-4, rel_tol=1e-12)
    if not case.with_pos:
        assert int((gt == 1).sum()) == 0 and not marks
        return
    pos_classes = set(((gt == 1).nonzero().flatten() % C).tolist())
    assert gt[marks["last_class"]] == 1 and marks["last_class"] % C == C - 1
    assert marks["last_class"] // 4 // T.FL_VEC_PER_BLOCK == (gt.numel() // 4 - 1) // T.FL_VEC_PER_BLOCK      # in the last block
    if C >= 2:
        assert len(pos_classes) >= 2 and C - 1 in pos_classes
    if C >= 2 and C % 4:
        e = marks["straddle"]
        v0 = e - e % 4
        assert gt[e] == 1 and v0 // C != (v0 + 3) // C and e // C != v0 // C, "the vector does not straddle two pixels"
        assert alpha[e % C] != alpha[v0 % C], "the first lane's weight would do as well"
    else:           # no vector can straddle: a pixel is a whole number of vectors (or there is one class)
        assert "straddle" not in marks and (C == 1 or all((4 * v) // C == (4 * v + 3) // C for v in range(gt.numel() // 4)))
    if case.pinned:
        assert logits[marks["pin_pos"]] == T.PIN_LOGIT and gt[marks["pin_pos"]] == 1
        assert logits[marks["pin_neg"]] == -T.PIN_LOGIT and gt[marks["pin_neg"]] < 1
        assert T.PIN_LOGIT > T.CLAMP_LOGIT + 1


@pytest.mark.parametrize("case", T.FOCAL_CASES, ids=T.focal_id)
def test_focal_f64_and_f32_oracles_agree(case):
    """the same oracle evaluated in f32 meets the bounds that the GPU tests hold the f32 kernel to: they are attainable, and the f64
    reference is what it claims to be.  Gaps measured on these cases: 1.4e-8 .. 1.3e-6 relative on the loss (the largest where a
    60-element map has a logit near +8 and no positives: log(1 - p) loses digits in f32), 2e-10 .. 9.8e-7 of max(1, max|grad|) on
    the gradient."""
    r64, r32 = T.focal_reference(case), T.focal_reference_f32(case)
    assert r64["grad"].dtype == torch.float64 and r32["grad"].dtype == torch.float32
    assert r64["num_pos"] == r32["num_pos"] == int((T.focal_inputs(case)["gt"] == 1).sum())
    assert (r64["num_pos"] > 0) == case.with_pos
    assert r32["loss"] == pytest.approx(r64["loss"], rel=1e-5, abs=1e-6)
    gmax = r64["grad"].abs().max().item()
    assert gmax > 0
    assert (r32["grad"].double() - r64["grad"]).abs().max().item() <= 1e-5 * max(1.0, gmax)
    if case.pinned:
        m = T.focal_inputs(case)["marks"]
        assert r64["grad"].reshape(-1)[m["pin_pos"]] == 0 and r64["grad"].reshape(-1)[m["pin_neg"]] == 0
    # pos + neg recombine to the loss
    scale = r64["num_pos"] or 1
    assert -(r64["pos"] + r64["neg"]) / scale == pytest.approx(r64["loss"], rel=1e-12)
    assert (r64["pos"] < 0) == case.with_pos and r64["neg"] < 0


# ------------------------------------------------------------------------------------------------------------- targets
def test_target_table():
    edges, tail, wrap = T.TARGET_CASES
    assert (edges.H, edges.W, edges.C, tuple(edges.boxes.shape)) == (24, 40, 5, (3, 6, 4)) and edges.H < edges.W
    assert edges.counts.tolist() == [6, 0, 9] and [T.target_objects(edges, b) for b in range(3)] == [6, 0, 6]
    ref = T.target_reference(edges)
    assert ref["ind"][0, 2] == 959 == 23 * 40 + 39                                           # the corner box
    assert torch.equal(edges.boxes[0, 0], edges.boxes[0, 1]) and edges.classes[0, 0] == edges.classes[0, 1]
    h, w = (edges.boxes[0, 3, 3] - edges.boxes[0, 3, 1]) / 4, (edges.boxes[0, 3, 2] - edges.boxes[0, 3, 0]) / 4
    assert max(0, int(O.gaussian_radius((math.ceil(h), math.ceil(w))))) == 0                 # the radius-0 box
    assert (ref["hm"][0, 0] > 0).sum() == 1 and ref["hm"][0, 0].max() == 1
    big = edges.boxes[0, 4] / 4
    assert big[0] < 0 and big[1] < 0 and big[2] > edges.W and big[3] > edges.H               # larger than the map
    drawn = ref["hm"][0, 2] > 0
    assert drawn[0].any() and drawn[-1].any() and ref["hm"][0, 2].max() == 1           # its window is clipped above and below
    assert edges.oob_class == {(0, 5)} and edges.classes[0, 5] == edges.C
    with pytest.raises(IndexError):
        O.gen_heatmap(edges.boxes[0], edges.classes[0], edges.H, edges.W, edges.C)
    assert ref["reg_mask"][0].tolist() == [1] * 6 + [0] * 122 and ref["wh"][0, 5].tolist() == [10.0, 10.0]
    assert ref["reg_mask"][1].sum() == 0 and not ref["hm"][1].any() and edges.boxes[1].abs().sum() > 0
    # the centres outside the map, one per side and one in (-1, 0), which the oracle alone would keep in column 0
    ctr = (edges.boxes[2, :, :2] + edges.boxes[2, :, 2:]) / 8
    outside = (ctr[:, 0] < 0) | (ctr[:, 0] >= edges.W) | (ctr[:, 1] < 0) | (ctr[:, 1] >= edges.H)
    assert edges.dropped == {(2, k) for k in outside.nonzero().flatten().tolist()} and len(edges.dropped) == 5
    assert ctr[0, 0] < -1 and -1 < ctr[1, 0] < 0 and ctr[2, 1] < -1 and ctr[3, 0] >= edges.W and ctr[4, 1] >= edges.H
    kept = O.gen_heatmap(edges.boxes[2, 1:2], edges.classes[2, 1:2], edges.H, edges.W, edges.C)
    assert kept["reg_mask"][0] == 1 and kept["ind"][0] % edges.W == 0
    assert ref["reg_mask"][2].tolist() == [0] * 5 + [1] + [0] * 122 and ref["hm"][2, [0, 1, 2, 4]].max() == 0
    for c in (tail, wrap):      # every centre inside the map
        cc = (c.boxes[..., :2] + c.boxes[..., 2:]) / 8
        assert (cc >= 0).all() and (cc[..., 0] < c.W).all() and (cc[..., 1] < c.H).all() and not c.dropped and not c.oob_class
    n_tail = tail.boxes.shape[0] * tail.H * tail.W * tail.C
    assert n_tail == 105 and n_tail & 3 and tail.prefill and tail.counts.tolist() == [3] and tail.boxes.shape[1] == 4
    n_wrap = wrap.boxes.shape[0] * wrap.H * wrap.W * wrap.C
    assert n_wrap == 2621440 and n_wrap // 4 > T.ZERO_GRID_CAP * 256 and wrap.prefill and int(wrap.counts.sum()) == 12
    for c in T.TARGET_CASES:
        r = T.target_reference(c)
        B = c.boxes.shape[0]
        assert r["hm"].shape == (B, c.C, c.H, c.W) and r["ind"].shape == (B, 128) and r["wh"].shape == r["reg"].shape == (B, 128, 2)
        assert r["hm"].dtype == np.float32 and r["ind"].dtype == np.int64 and r["reg_mask"].dtype == np.uint8
        assert (r["ind"] >= 0).all() and (r["ind"] < c.H * c.W).all()


# -------------------------------------------------------------------------------------------------------------- reg L1
def test_reg_table():
    assert len(T.REG_CASES) == 12 and len(set(T.REG_CASES)) == 12
    assert {(c.B, c.N) for c in T.REG_CASES} == {(1, 5), (3, 128), (2, 37)} and 1 * 5 < 256 < 3 * 128
    assert {(c.S, c.lo) for c in T.REG_CASES} == {(4, 0), (4, 2), (8, 0), (8, 2)}
    assert (T.REG_H, T.REG_W) == (6, 10) and T.REG_GRAD_SCALES == (1.0, 1024.0)
    HW = T.REG_H * T.REG_W
    for c in T.REG_CASES:
        inp = T.reg_inputs(c)
        assert inp["buf"].shape == (c.B, T.REG_H, T.REG_W, c.S)
        assert inp["ind"][0, 0] == inp["ind"][0, 1] and inp["mask"][0, 0] == inp["mask"][0, 1] == 1
        pix = inp["buf"][0].view(HW, c.S)[inp["ind"][0, 3]]
        assert inp["mask"][0, 3] == 1 and pix[c.lo] == inp["target"][0, 3, 0] and pix[c.lo + 1] != inp["target"][0, 3, 1]
        bad = ((inp["ind"] < 0) | (inp["ind"] >= HW)) & (inp["mask"] != 0)
        assert sorted(map(tuple, bad.nonzero().tolist())) == sorted(inp["oob"]) and len(inp["oob"]) == (2 if c.N > 5 else 1)
        assert inp["ind"][0, 2] == HW and not (inp["ref_mask"][bad]).any()
        assert inp["ref_mask"].sum() == inp["mask"].sum() - len(inp["oob"]) and inp["ref_mask"].sum() >= 3


@pytest.mark.parametrize("case", T.REG_CASES, ids=T.reg_id)
def test_reg_f64_and_f32_oracles_agree(case):
    r64, r32 = T.reg_reference(case), T.reg_reference(case, dtype=torch.float32)
    assert r64["grad"].dtype == torch.float64 and r32["grad"].dtype == torch.float32
    assert r32["loss"] == pytest.approx(r64["loss"], rel=1e-6)
    assert (r32["grad"].double() - r64["grad"]).abs().max().item() < 1e-7
    outside = [ch for ch in range(case.S) if not case.lo <= ch < case.lo + 2]
    assert not r64["grad"][..., outside].any() and r64["grad"].abs().max() > 1e-3
    zero = T.reg_reference(case, zero_mask=True)
    assert zero["loss"] == 0 and not zero["grad"].any()


# -------------------------------------------------------------------------------------------------------------- finite
def test_finite_table():
    small, big, one = T.FINITE_CASES
    assert (small.shape[2:], small.lo, small.hi) == ((1, 4), 0, 2) and (big.shape, big.lo, big.hi) == ((5, 128, 128, 16), 0, 13)
    assert T.finite_numel(big) == 1064960 > T.FINITE_GRID_CAP * 256 and one.hi - one.lo == 1
    assert len(T.FINITE_WAYS) == 6
    for c in T.FINITE_CASES:
        n = T.finite_numel(c)
        for way in T.FINITE_WAYS:
            bufs = T.finite_buffers(c, way)
            assert len(bufs) == (2 if way == "second_bad" else 1)
            sl = [b[..., c.lo:c.hi].reshape(-1) for b in bufs]
            assert T.finite_reference(c, bufs) == (1 if way in ("finite", "bad_outside") else 0), (c, way)
            assert sl[0][1] == T.FLT_MAX and sl[0][n - 2] == -T.FLT_MAX
            bad = (~torch.isfinite(sl[-1])).nonzero().flatten().tolist()
            want = {"finite": [], "bad_outside": [], "nan_first": [0], "inf_last": [n - 1], "ninf_middle": [n // 2], "second_bad": [n // 3]}
            assert bad == want[way], (c, way)
            if way == "second_bad":
                assert torch.isfinite(sl[0]).all()
            if way == "bad_outside":
                outside = [ch for ch in range(c.shape[3]) if not c.lo <= ch < c.hi]
                assert outside and not torch.isfinite(bufs[0][..., outside]).any()
    assert T.finite_numel(big) - 1 >= T.FINITE_GRID_CAP * 256       # only the second stride pass reaches the last element


# -------------------------------------------------------------------------------------------- nothing is left out
def test_gpu_module_runs_every_case():
    """the share of cases that the GPU tests leave out is 0: their parameter lists are the tables"""
    import test_objective_gpu as G

    assert _params(G.test_focal_loss) == T.FOCAL_CASES
    got = _params(G.test_gaussian_targets)
    assert len(got) == len(T.TARGET_CASES) == 3 and all(a is b for a, b in zip(got, T.TARGET_CASES))
    assert _params(G.test_reg_l1_loss) == T.REG_CASES
    assert set(_params(G.test_finite_flag)) >= set(T.FINITE_CASES) | set(T.FINITE_WAYS)
    assert len(_params(G.test_finite_flag)) == len(T.FINITE_CASES) + len(T.FINITE_WAYS)
    assert any(m.name == "gpu" for m in (G.pytestmark if isinstance(G.pytestmark, list) else [G.pytestmark]))
