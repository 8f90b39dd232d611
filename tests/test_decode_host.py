"""The case tables of decode_cases.py against their own conditions, with the oracle alone and without a GPU: the restated tile
geometry gives the branch each shape is there for, every case is inside the launcher's limits and holds what it promises (peak
counts above or below K, selections that reach the later channel chunks, the layout of the tie blocks, the first-bin maximum, the
share of the map on the clamp floor), the postprocess reference keeps exactly the rows that the recipes mean to be kept, and
nothing is filtered out on the way to the GPU tests."""
import math

import numpy as np
import pytest
import torch

import decode_cases as T


def _params(fn):
    return [p for m in fn.pytestmark if m.name == "parametrize" for p in m.args[1]]


def _group(name):
    return [c for c in T.DECODE_CASES if c.group == name]


# ------------------------------------------------------------------------------------------------------------ geometry
def test_tile_geometry_restated():
    assert (T.DEC_LDS_TILE, T.DEC_TW, T.DEC_CW_MAX, T.DEC_TILE_BYTES, T.DEC_LIST_BYTES) == (61440, 16, 112, 4, 6)
    assert T.dec_geom(9, 21, 80)[:3] == (80, 8, 1)
    assert T.dec_geom(9, 21, 81)[:3] == (84, 4, 1)
    assert T.dec_geom(9, 21, 113)[:3] == (112, 4, 2)
    assert T.dec_geom(9, 21, 225)[:3] == (112, 4, 3)
    for c in T.DECODE_CASES:
        assert T.dec_geom(c.H, c.W, c.C)[:3] == T.GEOMETRY[c.C], c
    # TH = 8 up to 80 classes, TH = 4 for every other class count: the peak list of 8 rows fits up to CW = 80 only, TH 2 and 1
    # cannot be reached with CW <= 112
    assert all(T.dec_geom(8, 16, C).TH == (8 if C <= 80 else 4) for C in range(1, 1000))
    assert 8 * 16 * 80 * 6 <= T.DEC_LDS_TILE < 8 * 16 * 84 * 6 and 10 * 18 * 84 * 4 <= T.DEC_LDS_TILE
    # one thread per (tile column incl. halo, channel vector)
    assert all((T.DEC_TW + 2) * (T.dec_geom(c.H, c.W, c.C).CW // 4) <= 512 for c in T.DECODE_CASES)
    g8, g4 = T.dec_geom(9, 21, 80), T.dec_geom(9, 21, 81)
    assert (g8.tiles_x, g8.tiles_y, g4.tiles_x, g4.tiles_y) == (2, 2, 2, 3) and 9 % 8 and 9 % 4 and 21 % 16


def test_decode_table():
    assert len(T.DECODE_CASES) == len(set(T.DECODE_CASES)) == 28 and len({T.decode_id(c) for c in T.DECODE_CASES}) == 28
    assert [len(_group(g)) for g in ("channels", "ties", "K", "bin0", "floor", "flip")] == [8, 2, 7, 1, 4, 6]
    ch = _group("channels")
    assert [(c.C, c.stride) for c in ch] == [(80, 80), (81, 81), (81, 84), (112, 112), (113, 113), (113, 116), (224, 224), (225, 228)]
    assert all((c.kind, c.B, c.H, c.W, c.K, c.floor, c.flip) == ("spread", 2, 9, 21, 100, 0.0, False) for c in ch)
    # the vector-load path with a partial last vector behind full ones: stride % 4 == 0, C % 4 != 0, more than one vector per pixel
    vec_partial = [c for c in T.DECODE_CASES if c.stride % 4 == 0 and c.C % 4]
    assert {(c.C, c.stride) for c in vec_partial} == {(81, 84), (113, 116), (225, 228)} and all(c.C > 4 for c in vec_partial)
    assert {(c.C, c.stride) for c in ch if c.stride % 4} == {(81, 81), (113, 113)}                 # scalar loads
    for c in T.DECODE_CASES:        # the launcher's limits
        assert c.stride >= c.C >= 1 and 1 <= c.K <= T.DEC_K_MAX and c.K <= c.C * c.H * c.W < 1 << T.DEC_INDEX_BITS, c
        assert c.floor in (0.0, T.HEAT_FLOOR)
        heat, wh, reg = T.decode_inputs(c)
        n = c.B * (2 if c.flip else 1)
        assert heat.shape == (n, c.C, c.H, c.W) and wh.shape == reg.shape == (n, 2, c.H, c.W)
        assert heat.dtype == wh.dtype == reg.dtype == torch.float32 and torch.isfinite(heat).all() and float(heat.min()) > 0
        assert float(heat.min()) >= 2.0 ** -126, "denormal heat value"
        if c.floor:                 # the promise that comes with the floor
            assert float(heat.min()) >= np.float32(c.floor) and float(T.decode_maps(c)[0].min()) >= np.float32(c.floor)
        assert all(t.shape[:2] == (c.B, c.K) for t in T.decode_reference(c))
    ks = _group("K")
    assert [(c.kind, (c.B, c.C, c.H, c.W), c.K) for c in ks] == [("spread", (1, 16, 32, 40), K) for K in (1, 257, 513, 1024)] + \
        [("spread", (1, 8, 12, 20), 1024), ("const2", (1, 116, 3, 3), 1024), ("spread", (2, 112, 12, 16), 513)]
    # final sort widths: the next power of two of the finalists, K <= n <= K - 1 + 2048
    assert [1 << (K - 1).bit_length() for K in (257, 513, 1024)] == [512, 1024, 1024] and (1024 - 1 + 2048) > 2048
    assert max(c.C * c.H * c.W for c in T.DECODE_CASES) == 113 * 24 * 40


@pytest.mark.parametrize("case", T.DECODE_CASES, ids=T.decode_id)
def test_decode_case_holds_what_it_promises(case):
    c, HW = case, case.H * case.W
    heat = T.decode_maps(c)[0]
    pk = T.peaks(c)
    npk = (pk > 0).sum(1)
    rb, rs, rc, ri = T.decode_reference(c)
    g = T.dec_geom(c.H, c.W, c.C)
    last_chunk = (g.cchunks - 1) * g.CW
    if c.group == "channels" or (c.group == "flip" and c.kind == "spread"):
        assert (npk > 10 * c.K).all()
        assert all(len(set(rs[b].tolist())) == c.K for b in range(c.B)), "tied scores among the selected"
        assert (rc.max(1).values >= last_chunk).all(), "an image's selection does not reach the last chunk"
        assert (rc.min(1).values < g.CW).all()
    if c.group == "ties":
        lo, hi = c.arg
        assert npk.tolist() == [c.C * HW] and HW == 95 and sorted(set(heat.flatten().tolist())) == [np.float32(0.1), 0.25]
        assert (heat[:, lo:hi] == 0.25).all() and (heat == 0.25).sum() == (hi - lo) * HW >= c.K
        canon = torch.arange(lo * HW, lo * HW + c.K)
        assert (rs == 0.25).all() and torch.equal(rc[0].long(), canon // HW) and torch.equal(ri[0], canon % HW)
        if c.K == 300:          # 95 + 95 + 95 + 15 positions of classes 110 .. 113: chunks 0 and 1, every tile
            assert torch.bincount(rc[0].long())[110:].tolist() == [95, 95, 95, 15] and lo < g.CW < hi
            assert ri[0, -15:].tolist() == list(range(15))
        else:                   # every tie in chunk 1; chunk 2 is the one strided channel 224
            assert c.K == 1024 and g.CW <= lo and hi - 1 == 2 * g.CW == c.C - 1 and c.stride == 228
            assert int(rc.min()) == 200 and int(rc.max()) == 200 + 1023 // HW < 2 * g.CW
            assert min(g.TH, c.H) * T.DEC_TW * (2 * g.CW - lo) > c.K - 1 + T.DEC_TILE_SLACK      # a tile's ties exceed its budget
    if c.group == "K":
        if (c.C, c.H, c.W) == (16, 32, 40):
            assert npk.tolist() == [2413] and float(rs.min()) > 0
            assert len(set(rs[0].tolist())) >= c.K - 1
        elif (c.C, c.H, c.W) == (8, 12, 20):
            assert npk.tolist() == [242] and c.C * HW == 1920 < 2 * c.K and int((rs == 0).sum()) == 782 == c.K - 242
            nonpeaks = (pk[0] == 0).nonzero().flatten()[:782]
            assert torch.equal(rc[0, 242:].long(), nonpeaks // HW) and torch.equal(ri[0, 242:], nonpeaks % HW)
        elif c.kind == "const2":
            assert c.arg == (0, c.C) and (heat == 0.25).all() and npk.tolist() == [1044] and 1044 - c.K == 20
            assert int(rc.max()) == 113 >= g.CW and torch.equal(ri[0], torch.arange(c.K) % HW)
        else:
            assert (c.C, g.TH, g.cchunks) == (112, 4, 1) and (npk > c.K).all() and float(rs.min()) > 0
    if c.group == "bin0":
        assert 0 < float(heat.min()) and float(heat.max()) < T.DEC_BIN0_BELOW
        assert (npk > c.K).all() and all(len(set(rs[b].tolist())) == c.K for b in range(c.B))
    if c.kind == "trained":
        floor = np.float32(T.HEAT_FLOOR)
        assert float((heat == floor).float().mean()) > 0.5 and float(heat.min()) == floor
        above = (heat > floor).reshape(c.B, -1).sum(1)
        if c.arg[0] == T.DENSE_BLOBS:
            assert c.arg[0] > c.K and ((pk > floor).sum(1) > c.K).all() and float(rs.min()) > floor
        else:
            assert (above < c.K).all() and (above > 0).all() and float(T.decode_inputs(c)[0][0, 0, 0, 1]) == np.float32(0.3)
            assert (rs[:, -1] == floor).all() and (rs[:, 0] > floor).all()
            assert (T.decode_inputs(c)[0][:, -1, -1, -1] == np.float32(0.2)).all()
        assert (rc.max(1).values >= last_chunk).all(), "an image's selection does not reach the last chunk"
        assert g.cchunks == 2 and c.stride == 116
    if c.flip:
        a, wh, reg = T.decode_inputs(c)
        B, m = c.B, c.W // 2
        mw = T.decode_maps(c)[1]
        assert torch.equal(heat[..., 3], (a[:B, ..., 3] + a[B:, ..., c.W - 4]) * 0.5)
        assert torch.equal(mw[..., 3], (wh[:B, ..., 3] + wh[B:, ..., c.W - 4]) * 0.5) and torch.equal(T.decode_maps(c)[2], reg[:B])
        if c.W % 2:             # the middle column merges with itself
            assert torch.equal(heat[..., m], (a[:B, ..., m] + a[B:, ..., m]) * 0.5)
        assert not torch.equal(a[:B], a[B:])


def test_flip_and_floor_variants_come_in_pairs():
    for grp in ("floor", "flip"):
        cs = _group(grp)
        on, off = [c for c in cs if c.floor], [c for c in cs if not c.floor]
        assert len(on) == len(off) and {c._replace(floor=0.0) for c in on} == set(off)
    fl = {(c.kind, c.C, c.stride, c.H, c.W) for c in _group("flip")}
    assert fl == {("spread", 81, 84, 9, 21), ("spread", 113, 113, 9, 21), ("trained", 113, 116, 24, 40)}
    assert all(c.arg == (T.SPARSE_BLOBS, True) for c in _group("flip") if c.kind == "trained")
    assert {c.arg for c in _group("floor")} == {(T.DENSE_BLOBS, False), (T.SPARSE_BLOBS, True)}


# --------------------------------------------------------------------------------------------------------- postprocess
def test_post_table():
    assert T.POST_KS == (1, 63, 64, 65, 100, 1024) and T.POST_B == 3
    assert len(T.POST_CASES) == len(set(T.POST_CASES)) == 24
    for K in T.POST_KS:
        assert [c.max_det for c in T.POST_CASES if c.K == K] == [K, K - 1, 1, K + 5]
    Hi, Wi = T.POST_IMAGE
    assert T.POST_OUT["g5"] == (Hi * 8 // 4, Wi * 6 // 4) and T.POST_OUT["unit"] == T.POST_IMAGE
    oh, ow = T.POST_OUT["inexact"]
    assert float(np.float32(ow / Wi)) != ow / Wi and float(np.float32(oh / Hi)) != oh / Hi
    assert float(np.float32(T.POST_THRESH)) == T.POST_THRESH
    assert set(T.SPECIAL_BLOCK) == set(T.KEEP_RECIPES) | set(T.DROP_RECIPES) and len(T.SPECIAL_BLOCK) == 21
    assert T.SPECIAL_ROWS[0] + 21 <= T.ALT_ROWS[0] < 63 < 64 < T.ALT_ROWS[1] == T.SPECIAL_ROWS[1] and T.SPECIAL_ROWS[1] + 21 <= 100


@pytest.mark.parametrize("case", T.POST_CASES, ids=T.post_id)
def test_post_reference_keeps_the_intended_rows(case):
    K, inp, ref = case.K, T.post_inputs(case), T.post_reference(case)
    seen = min(K, max(case.max_det, 0))
    fate, recipes = inp["fate"], inp["recipes"]
    assert inp["boxes"].shape == (3, K, 4) and inp["scores"].shape == inp["classes"].shape == (3, K) and inp["img_params"].shape == (3, 4)
    for b in range(3):
        oh, ow = inp["out"][b]
        assert inp["img_params"][b].tolist() == [np.float32(ow / T.POST_IMAGE[1]), np.float32(oh / T.POST_IMAGE[0]), ow, oh]
        bb, ss, cc = ref[b]
        assert cc.tolist() == [k for k in range(seen) if fate[b, k]], f"image {b}: the reference keeps other rows than intended"
        assert torch.isfinite(bb).all() and (bb >= 0).all() and (bb[:, 2] <= ow).all() and (bb[:, 3] <= oh).all()
        assert not torch.isnan(ss).any() and (ss > T.POST_THRESH).all()
    scales = [tuple(p[:2]) for p in inp["img_params"].tolist()]
    assert scales[1] == (1.0, 1.0) and (1.5, 2.0) in scales and sorted(inp["out"]) == sorted(T.POST_OUT.values())
    assert len(ref[1][1]) == seen and len(ref[2][1]) == 0                     # all, none
    assert fate[1].all() and not fate[2].any()
    mixed = fate[0]
    if K == 1:
        assert recipes[0] == ["thresh_tie"] and len(ref[0][1]) == 0
        return
    assert recipes[0][0] == "clip_left_top" and set(recipes[0]) == set(T.SPECIAL_BLOCK)
    assert set(recipes[1]) == set(T.KEEP_RECIPES) and set(recipes[2]) <= set(T.DROP_RECIPES) and len(set(recipes[2])) >= 12
    if seen > 1:
        assert 0 < len(ref[0][1]) < seen
    # kept and dropped rows alternate up to and across the seam between rows 63 and 64
    alt = mixed[T.ALT_ROWS[0]:min(K, T.ALT_ROWS[1])].tolist()
    assert len(alt) >= 15 and all(alt[j] != alt[j + 1] for j in range(len(alt) - 1))
    if K > 64:
        assert mixed[63] != mixed[64]
    for lo, hi in ((0, 64), (64, K)):           # both fates on each side of row 64 (K = 65 has a single row behind it)
        if hi - lo > 1:
            assert mixed[lo:hi].any() and not mixed[lo:hi].all()
    # the rows the table is about: what they are, and that the reference drops or keeps them
    rows = {r: recipes[0].index(r) for r in T.SPECIAL_BLOCK}
    box, sc = inp["boxes"][0], inp["scores"][0]
    sx, sy, ow, oh = inp["img_params"][0].tolist()
    k = rows["thresh_tie"]
    assert sc[k] == T.POST_THRESH and 0 < box[k, 0] < box[k, 2] < T.POST_IMAGE[1] and not mixed[k]
    k = rows["nan_x1"]
    assert math.isnan(box[k, 0]) and torch.isfinite(box[k, 1:]).all() and box[k, 2] * sx > 0 and 0 < box[k, 1] < box[k, 3] and \
        sc[k] > T.POST_THRESH and not mixed[k], "one NaN coordinate, an otherwise valid extent: dropped by the reference"
    k = rows["left"]
    assert box[k, 0] < box[k, 2] < 0 and sc[k] > T.POST_THRESH
    k = rows["right"]
    assert T.POST_IMAGE[1] < box[k, 0] < box[k, 2]
    k = rows["reversed"]
    assert 0 < box[k, 2] < box[k, 0] < T.POST_IMAGE[1]
    assert box[rows["zero_w"], 0] == box[rows["zero_w"], 2] and box[rows["zero_h"], 1] == box[rows["zero_h"], 3]
    assert math.isnan(sc[rows["nan_score"]]) and sc[rows["inf_score"]] == math.inf and sc[rows["neg_inf_score"]] == -math.inf
    k = rows["inf_span"]
    assert box[k, 0] == -math.inf and box[k, 2] == math.inf and mixed[k]
    assert box[rows["inf_x1"], 0] == math.inf and box[rows["neg_inf_x2"], 2] == -math.inf
    if case.max_det >= K - 1:
        kept = dict(zip(ref[0][2].tolist(), ref[0][0].tolist()))
        assert kept[rows["inf_span"]][0::2] == [0.0, ow] and kept[rows["clip_left_top"]][:2] == [0.0, 0.0]
        assert kept[rows["clip_right_bottom"]][2:] == [ow, oh]
        assert rows["inf_score"] in kept and rows["nan_x1"] not in kept and rows["thresh_tie"] not in kept


# -------------------------------------------------------------------------------------------- nothing is left out
def test_gpu_module_runs_every_case():
    import test_decode_gpu as G

    got = _params(G.test_decode)
    assert len(got) == len(T.DECODE_CASES) and all(a is b for a, b in zip(got, T.DECODE_CASES))
    got = _params(G.test_postprocess)
    assert len(got) == len(T.POST_CASES) and all(a is b for a, b in zip(got, T.POST_CASES))
    assert any(m.name == "gpu" for m in (G.pytestmark if isinstance(G.pytestmark, list) else [G.pytestmark]))
