"""Case table for dec_postprocess_affine_kernel (csrc/unwarp.hip, ops.postprocess_affine) and its numpy oracle
data.warp.unwarp_boxes_reference: the smallest shapes at which the kernel can go wrong.  K in {1, 63, 64, 65, 130} (one lane, the
seam of the 64-lane wave on both sides, a third pass), max_det below, at and above K, B = 1 and B = 3 with three different
parameter rows (a kernel that strides the [B, 6] rows by 4 reads image 1's from the middle of image 0's), sx != sy, translations
of both signs, and every way a row can be kept or dropped.  The conditions the table claims are asserted here, at import, on the
CPU; test_unwarp_host.py checks the oracle itself, test_unwarp_gpu.py the kernel against it, bit for bit."""
import functools
from collections import namedtuple

import numpy as np

from detectron2_centernet_amd.data import warp as W

THRESH = float(np.float32(0.3))
# (sx, sy, tx, ty, orig_w, orig_h) as data.warp.unwarp_params gives them: the worked fix_res answer for a 640 x 480 source,
# and two rows no mapper would make: sx != sy, a scale that is no short binary fraction, translations of both signs
PARAMS = np.array([
    W.unwarp_params(W.test_params(480, 640, "fix_res", (512, 512), 32)[0], (480, 640)),
    np.array([1.3671875, 0.7, 13.5, -7.25, 700.0, 350.0]),
    np.array([1.0 / 3.0, 1.1, -16.0, 9.0, 200.0, 300.0]),
], dtype=np.float64).astype(np.float32)
assert PARAMS[0].tolist() == [1.25, 1.25, 0.0, -80.0, 640.0, 480.0]
assert all(p[0] != p[1] for p in PARAMS[1:]) and len({tuple(p) for p in PARAMS}) == 3
assert {np.sign(p[2]) for p in PARAMS} == {0.0, 1.0, -1.0} and {np.sign(p[3]) for p in PARAMS} >= {1.0, -1.0}
# a stride of 4 would hand image 1 the row (tx0, ty0, w0, h0, sx1, sy1) and image 2 one that starts at sx1's third float
assert not np.array_equal(PARAMS.reshape(-1)[4:10], PARAMS[1]) and not np.array_equal(PARAMS.reshape(-1)[8:14], PARAMS[2])

KEEP_RECIPES = ("inside", "clip_left_top", "clip_right_bottom", "pos_inf_x2", "neg_inf_x1", "inf_span", "inf_score")
DROP_RECIPES = ("low_score", "thresh_tie", "nan_score", "nan_x1", "nan_y2", "left_of_frame", "below_frame", "reversed", "zero_w",
                "zero_h", "pos_inf_x1", "neg_inf_y2")
# rows stated in the network input's pixels, for PARAMS[0] alone: the hand-derived box whose corners land exactly on 0 and on
# (orig_w, orig_h), and boxes that are non-empty until the clip
EXACT_ROWS = {
    "exact_corners": ((0.0, 64.0, 512.0, 448.0, 0.9), True),       # -> (0, 0, 640, 480) with nothing clipped
    "empty_after_clip_x": ((-16.0, 100.0, -4.0, 200.0, 0.9), False),      # -> x in (-20, -5): both clip to 0
    "empty_after_clip_y": ((100.0, 452.0, 200.0, 460.0, 0.9), False),     # -> y in (485, 495): both clip to 480
}

Case = namedtuple("Case", "name K max_det B fill first")      # fill: mixed / kept / dropped; first: PARAMS row of image 0
CASES = [
    Case("one_lane", 1, 1, 1, "kept", 0),
    Case("one_lane_max_above", 1, 5, 3, "mixed", 1),
    Case("below_seam", 63, 63, 1, "mixed", 1),
    Case("seam", 64, 64, 3, "mixed", 0),
    Case("seam_max_below", 64, 10, 1, "mixed", 2),
    Case("past_seam", 65, 65, 3, "mixed", 2),
    Case("past_seam_max_at_seam", 65, 64, 3, "mixed", 0),
    Case("third_pass", 130, 130, 3, "mixed", 0),
    Case("third_pass_max_below", 130, 100, 1, "mixed", 0),
    Case("third_pass_max_above", 130, 200, 3, "mixed", 1),
    Case("all_dropped", 65, 65, 1, "dropped", 1),
    Case("all_kept", 130, 130, 1, "kept", 2),
    Case("contraction", 130, 130, 3, "inside", 1),
]
CASE_IDS = [c.name for c in CASES]
assert {c.K for c in CASES} == {1, 63, 64, 65, 130} and {c.B for c in CASES} == {1, 3}
assert any(c.max_det < c.K for c in CASES) and any(c.max_det == c.K for c in CASES) and any(c.max_det > c.K for c in CASES)


def _row(recipe, p, rng):
    """one detection (x1, y1, x2, y2, score) in the network input's pixels whose image under p is the recipe's box"""
    sx, sy, tx, ty, ow, oh = (float(v) for v in p)
    inf, nan = float("inf"), float("nan")
    if recipe in EXACT_ROWS:
        return EXACT_ROWS[recipe][0]
    X1, Y1 = rng.uniform(2, 0.4 * ow), rng.uniform(2, 0.4 * oh)      # the box wanted in the ORIGINAL frame
    X2, Y2 = X1 + rng.uniform(2, 0.4 * ow), Y1 + rng.uniform(2, 0.4 * oh)
    score = rng.uniform(THRESH + 0.05, 1.0)
    if recipe == "clip_left_top":
        X1, Y1 = -rng.uniform(1, 15), -rng.uniform(1, 10)
    elif recipe == "clip_right_bottom":
        X2, Y2 = ow + rng.uniform(1, 15), oh + rng.uniform(1, 10)
    elif recipe == "pos_inf_x2":
        X2 = inf
    elif recipe == "neg_inf_x1":
        X1 = -inf
    elif recipe == "inf_span":
        Y1, Y2 = -inf, inf
    elif recipe == "inf_score":
        score = inf
    elif recipe == "low_score":
        score = rng.uniform(0.01, THRESH - 0.05)
    elif recipe == "thresh_tie":
        score = THRESH
    elif recipe == "nan_score":
        score = nan
    elif recipe == "nan_x1":
        X1 = nan
    elif recipe == "nan_y2":
        Y2 = nan
    elif recipe == "left_of_frame":
        X1, X2 = -rng.uniform(20, 30), -rng.uniform(1, 10)
    elif recipe == "below_frame":
        Y1, Y2 = oh + rng.uniform(1, 10), oh + rng.uniform(20, 30)
    elif recipe == "reversed":
        X1, X2 = X2, X1
    elif recipe == "zero_w":
        X2 = X1
    elif recipe == "zero_h":
        Y2 = Y1
    elif recipe == "pos_inf_x1":
        X1 = inf
    elif recipe == "neg_inf_y2":
        Y2 = -inf
    elif recipe != "inside":
        raise ValueError(recipe)
    if recipe == "zero_w":      # equal in the network frame, so that they are equal after any rounding
        x1 = x2 = (X1 - tx) / sx
    else:
        x1, x2 = (X1 - tx) / sx, (X2 - tx) / sx
    if recipe == "zero_h":
        y1 = y2 = (Y1 - ty) / sy
    else:
        y1, y2 = (Y1 - ty) / sy, (Y2 - ty) / sy
    return x1, y1, x2, y2, score


def recipes(case):
    """per image the recipe of every row"""
    rng = np.random.RandomState(1000 + 7 * case.K + case.max_det)
    out = []
    for b in range(case.B):
        row = (case.first + b) % len(PARAMS)
        special = list(KEEP_RECIPES + DROP_RECIPES) + (list(EXACT_ROWS) if row == 0 else [])
        if case.fill == "kept":
            names = [KEEP_RECIPES[rng.randint(len(KEEP_RECIPES))] for _ in range(case.K)]
        elif case.fill == "dropped":
            names = [DROP_RECIPES[rng.randint(len(DROP_RECIPES))] for _ in range(case.K)]
        elif case.fill == "inside":
            names = ["inside"] * case.K
        else:
            names = []
            for k in range(case.K):      # kept and dropped rows alternate in runs of random length, across the seams too
                pool = KEEP_RECIPES if rng.randint(2) else DROP_RECIPES
                names.append(pool[rng.randint(len(pool))])
            if case.K >= len(special) + 2:      # every recipe once, from row 2; K = 130: again across the seam at 128
                names[2:2 + len(special)] = special
                if case.K >= 130:
                    names[120:130] = ["inside", "nan_x1", "inside", "thresh_tie", "inside", "left_of_frame", "inside", "inside",
                                      "nan_score", "inside"]
        out.append(names)
    return out


@functools.lru_cache(maxsize=None)
def inputs(case):
    """dict: boxes f32 [B, K, 4], scores f32 [B, K], classes i32 [B, K] (the row's own number: the order is checked with it),
    params f32 [B, 6], recipes, fate bool [B, K]: the rows the recipes mean to be kept (before max_det cuts)"""
    names = recipes(case)
    rng = np.random.RandomState(77 + 13 * case.K + case.B)
    params = np.stack([PARAMS[(case.first + b) % len(PARAMS)] for b in range(case.B)])
    rows = np.array([[_row(r, params[b], rng) for r in names[b]] for b in range(case.B)], dtype=np.float64).astype(np.float32)
    fate = np.array([[(r in KEEP_RECIPES) or (r in EXACT_ROWS and EXACT_ROWS[r][1]) for r in image] for image in names])
    out = {"boxes": np.ascontiguousarray(rows[..., :4]), "scores": np.ascontiguousarray(rows[..., 4]),
           "classes": np.tile(np.arange(case.K, dtype=np.int32), (case.B, 1)), "params": params, "recipes": names, "fate": fate}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(case):
    """per image (boxes [n, 4], scores [n], classes [n]) of data.warp.unwarp_boxes_reference; computed once, read only"""
    inp = inputs(case)
    res = []
    for b in range(case.B):
        r = W.unwarp_boxes_reference(inp["boxes"][b], inp["scores"][b], inp["classes"][b], case.max_det, THRESH, inp["params"][b])
        for a in r:
            a.setflags(write=False)
        res.append(r)
    return res


def two_roundings(x, s, t):
    """f32(f32(x * s) + t) and the fused f32(f64(x) * f64(s) + f64(t)) of f32 arrays"""
    x, s, t = (np.asarray(v, dtype=np.float32) for v in (x, s, t))
    with np.errstate(invalid="ignore", over="ignore"):
        two = ((x * s).astype(np.float32) + t).astype(np.float32)
        fused = (x.astype(np.float64) * s.astype(np.float64) + t.astype(np.float64)).astype(np.float32)
    return two, fused


def contraction_rows(case):
    """per image the numbers of the KEPT rows with a corner, inside the frame, whose fused value differs from the two-rounding
    one: the rows a kernel compiled with a fused multiply-add gets wrong"""
    inp, ref = inputs(case), reference(case)
    out = []
    for b in range(case.B):
        p = inp["params"][b]
        s, t, hi = p[[0, 1, 0, 1]], p[[2, 3, 2, 3]], p[[4, 5, 4, 5]]
        two, fused = two_roundings(inp["boxes"][b], s, t)
        differs = ((two != fused) & np.isfinite(two) & (two > 0) & (two < hi) & (fused > 0) & (fused < hi)).any(axis=1)
        out.append([int(k) for k in ref[b][2] if differs[k]])
    return out


# ------------------------------------------------------------------------------------------- what the table claims, checked
def _check():
    seen = set()
    for case in CASES:
        inp, ref = inputs(case), reference(case)
        seen.update(r for image in inp["recipes"] for r in image[:case.max_det])
        for b in range(case.B):
            want = [k for k in range(min(case.K, case.max_det)) if inp["fate"][b, k]]
            assert ref[b][2].tolist() == want, (case.name, b)      # the oracle keeps exactly the rows the recipes mean, in order
        if case.fill == "dropped":
            assert all(len(r[2]) == 0 for r in ref), case.name
        if case.fill == "kept":
            assert all(len(r[2]) == min(case.K, case.max_det) for r in ref), case.name
    assert seen >= set(KEEP_RECIPES + DROP_RECIPES) | set(EXACT_ROWS), sorted(set(KEEP_RECIPES + DROP_RECIPES) | set(EXACT_ROWS) - seen)
    # the exact rows do what their names say under PARAMS[0]
    p = PARAMS[0]
    s, t = p[[0, 1, 0, 1]], p[[2, 3, 2, 3]]
    moved, _ = two_roundings(np.array(EXACT_ROWS["exact_corners"][0][:4]), s, t)
    assert moved.tolist() == [0.0, 0.0, float(p[4]), float(p[5])]      # exactly 0 and exactly (orig_w, orig_h), unclipped
    for name, axis in (("empty_after_clip_x", 0), ("empty_after_clip_y", 1)):
        moved, _ = two_roundings(np.array(EXACT_ROWS[name][0][:4]), s, t)
        lo, hi = moved[axis], moved[axis + 2]
        assert hi - lo > 0 and moved[3 - axis] - moved[1 - axis] > 0      # a box with an area ...
        assert np.clip(lo, 0, p[4 + axis]) == np.clip(hi, 0, p[4 + axis])      # ... that the clip empties
    # score == thresh is a tie in f32, the comparison the kernel makes
    tie = inputs(CASES[3])
    k = tie["recipes"][0].index("thresh_tie")
    assert tie["scores"][0, k] == np.float32(THRESH) and not tie["fate"][0, k]
    # a contracted kernel cannot pass: enough kept rows differ between the fused and the two-rounding arithmetic
    n = sum(len(rows) for case in CASES for rows in contraction_rows(case))
    assert n >= 8, n


_check()
