"""The case table of dcn_grad_cases.py without a GPU: its float64 references agree with the oracle's restatement of the reference
kernels and with double autograd through oracle.dcnv2_forward; every instantiation the DCN gradient launchers can select has a
row; every row's geometry holds the edge classes it lists, the designed window-edge samples on the side of the margin they were
designed for; and every row, replayed through the library's dry run on stand-in pointers, gives the row's label."""
import ctypes as C

import pytest
import torch

import dcn_grad_cases as G
from dcn_grad_cases import MASK_MODE, ROWS, case_id
from detectron2_centernet_amd import _lib
from detectron2_centernet_amd._lib import F16, F16X3, F32
from oracle import ctdet_oracle as O
from test_kernel_labels_host import BASE, dry_run

COMPUTE = {"f16": F16, "f32": F32, "f16x3": F16X3}
SLICE_EXTRA = 16        # x is a channel slice of a buffer with this many more channels per pixel in the GPU test
OM_STRIDE = 32          # and om a 32-channel buffer


# ------------------------------------------------------------------------------------------ the references themselves
def _problem(mask, seed, B=2, Cin=3, Cout=4, H=5, W=6):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, Cin, generator=g, dtype=torch.float64)
    om = torch.randn(B, H, W, 18 if mask == "none" else 27, generator=g, dtype=torch.float64)
    om[..., :18] *= 2.0                                   # a fair share of samples in the border bands and outside
    om[0, 0, 0, 0], om[0, 0, 0, 1] = 0.0, 0.0             # h_im = w_im = -1 exactly
    om[0, H - 1, W - 1, 16], om[0, H - 1, W - 1, 17] = 0.0, -0.5       # h_im = H exactly
    weight = torch.randn(Cout, Cin, 3, 3, generator=g, dtype=torch.float64)
    dy = torch.randn(B, H, W, Cout, generator=g, dtype=torch.float64)
    return x, om, weight, dy


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _oracle_mask(om, mask):
    if mask == "none":
        return torch.ones(om.shape[0], 9, om.shape[1], om.shape[2], dtype=torch.float64)
    m = _nchw(om[..., 18:27])
    return m if mask == "prob" else torch.sigmoid(m)


@pytest.mark.parametrize("mask", ["logit", "prob", "none"])
def test_references_against_the_oracle(mask):
    x, om, weight, dy = _problem(mask, 11)
    B, H, W, Cin = x.shape
    Cout = weight.shape[0]
    mm = MASK_MODE[mask]
    m = _oracle_mask(om, mask)
    gx, goff, gmask, _, _ = O.dcnv2_backward(_nchw(x), _nchw(om[..., :18]), m, weight, _nchw(dy), with_bias=False)
    dcol = dy @ weight.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin)              # column tap * Cin + c
    dx, dom = G.col2im_ref(dcol, x, om, mm)
    assert (_nchw(dx) - gx).abs().max() <= 1e-12
    assert (_nchw(dom[..., :18]) - goff).abs().max() <= 1e-12
    if mask == "prob":
        assert (_nchw(dom[..., 18:]) - gmask).abs().max() <= 1e-12
    elif mask == "logit":
        assert (_nchw(dom[..., 18:]) - gmask * m * (1 - m)).abs().max() <= 1e-12
    else:
        assert dom.shape[3] == 18
    # exactly on -1 / on H: outside, every gradient exactly zero
    assert torch.equal(dom[0, 0, 0, [0, 1]], torch.zeros(2, dtype=torch.float64))
    assert torch.equal(dom[0, H - 1, W - 1, [16, 17]], torch.zeros(2, dtype=torch.float64))
    cols, _, _ = O.dcnv2_columns(_nchw(x), _nchw(om[..., :18]), m)
    want = cols.view(B, Cin, 9, H, W).permute(0, 3, 4, 2, 1).reshape(B, H, W, 9 * Cin)
    assert (G.cols_ref(x, om, mm) - want).abs().max() <= 1e-12


@pytest.mark.parametrize("mask", ["logit", "prob", "none"])
def test_references_against_double_autograd(mask):
    """through oracle.dcnv2_forward; random offsets are never integers, the two designed outside samples have zero gradient in
    both"""
    x, om, weight, dy = _problem(mask, 12, Cin=32, Cout=5)
    B, H, W, Cin = x.shape
    xg, og = x.clone().requires_grad_(), om.clone().requires_grad_()
    m = _oracle_mask(og, mask)
    y = O.dcnv2_forward(_nchw(xg), _nchw(og[..., :18]), m, weight)
    gx, gom = torch.autograd.grad(y, (xg, og), _nchw(dy))
    dx, dom = G.fused_ref(dy, weight, x, om, MASK_MODE[mask])                   # the chunked column order
    assert (dx - gx).abs().max() <= 1e-12
    assert (dom - gom).abs().max() <= 1e-12
    dcol = dy @ weight.permute(0, 2, 3, 1).reshape(-1, 9 * Cin)
    assert (G.tap_major(G.fused_dcol(dy, weight), Cin, True) - G.tap_major(dcol, Cin, False)).abs().max() <= 1e-12
    cols = G.cols_ref(x, om, MASK_MODE[mask]).view(B, H, W, 9, Cin)
    assert (torch.einsum("bhwtc,octr->bhwor", cols, weight.reshape(-1, Cin, 9, 1))[..., 0] - y.detach().permute(0, 2, 3, 1)).abs().max() <= 1e-12


def test_contribution_counts():
    x, om, weight, dy = _problem("logit", 13)
    n, _ = G.col2im_ref(torch.zeros(2, 5, 6, 27, dtype=torch.float64), x, om, 0, counts=True)
    inside = ~G.classify(G.ROWS[0]._replace(H=5, W=6), om)["outside"]
    assert n.shape[3] == 1 and 0 < n.sum() <= 4 * inside.sum() and n.max() > 4


# ------------------------------------------------------------------------------------------ the table
# every instantiation the launchers of train_bwd.hip (and launch_dcn_cols_window) can select, as its label
INSTANTIATIONS = (
    ["dcn_cols_kernel<f16,mask>", "dcn_cols_kernel<f16,no mask>",
     "dcn_window_rows_kernel<columns only,f16,mask>", "dcn_window_rows_kernel<columns only,f16,no mask>",
     "dcn_cols_f32_kernel<mask>", "dcn_cols_f32_kernel<no mask>",
     "dcn_col2im_coord_kernel<f16,mask>", "dcn_col2im_coord_kernel<f16,no mask>",
     "dcn_col2im_coord_kernel<f32,mask>", "dcn_col2im_coord_kernel<f32,no mask>"]
    + [f"dcn_col2im_window_kernel<{nt} taps,{t}{m}>" for nt in (3, 5, 9) for t in ("f16,", "f32,", "f32,fused dcol,")
       for m in ("mask", "no mask")])


def test_every_instantiation_has_a_row():
    assert len(INSTANTIATIONS) == 28 and {c.label for c in ROWS} == set(INSTANTIATIONS)
    for c in ROWS:
        if "window_kernel<" in c.label and "taps" in c.label:
            assert c.nt == int(c.label.split("<")[1].split(" ")[0]) and ("fused" in c.label) == (c.op == "col2im_fused"), c
            assert ("f16," in c.label) == (c.mode == "f16") and c.mode != "f32", c
        assert ("no mask" in c.label) == (c.mask == "none"), c
    # the mask modes and dom forms of the issue
    cols = {(c.label, c.mask) for c in ROWS if c.op == "cols"}
    assert len(cols) == 9
    gen = [c for c in ROWS if c.op == "col2im" and c.kind == "generic"]
    assert {(c.mode, c.dom_c) for c in gen if c.mask != "none"} >= {("f16", 27), ("f16", 28), ("f16", 32), ("f32", 27), ("f32", 28), ("f32", 32), ("f16x3", 32)}
    assert {c.dom_c for c in gen if c.mask == "none"} == {18, 20, 32} and any(c.mask == "prob" for c in gen)
    win = [c for c in ROWS if c.op == "col2im" and c.kind == "window"]
    for mode in ("f16", "f16x3"):
        assert {(c.Cin, c.chunked) for c in win if c.mode == mode} == {(32, False), (64, True), (96, False)}
    assert {(c.Cin, c.Cout) for c in ROWS if c.op == "col2im_fused"} == {(32, 32), (64, 40)}


def test_rows_are_well_formed():
    assert len(set(ROWS)) == len(ROWS) and len({case_id(c) for c in ROWS}) == len(ROWS)
    for c in ROWS:
        assert c.mode in COMPUTE and c.op in ("cols", "col2im", "col2im_fused") and c.mask in MASK_MODE, c
        assert (c.op == "cols") == (c.dom_c == 0) and (c.dom_c == 0 or 64 >= c.dom_c >= G.om_channels(c)), c
        assert (c.B is None) == (c.nt in (5, 9)), c
        B = G.batch_of(c)
        assert B is not None, c                              # on a 256-CU part no row may skip
        if c.kind == "window":
            assert (c.H, c.W) == (16, 32) and c.Cin % 32 == 0, c
            t = B * 4
            assert c.nt == 0 or c.nt == (3 if 3 * t <= 256 else 5 if 2 * t <= 256 else 9), c
    assert {G.batch_of(c) for c in ROWS if c.nt == 5} == {22} and {G.batch_of(c) for c in ROWS if c.nt == 9} == {33}
    nt5 = next(c for c in ROWS if c.nt == 5)
    assert G.batch_of(nt5, ncu=8) == 1 and G.batch_of(nt5, ncu=7) is None      # NT 5 needs 3 * 4 B > ncu >= 2 * 4 B


@pytest.mark.parametrize("c", ROWS, ids=[case_id(c) for c in ROWS])
def test_row_contains_its_edges(c):
    B = G.batch_of(c)
    om, samples = G.geometry(c, B)
    k = G.classify(c, om)
    for e in c.edges:
        assert bool(k[e].any()), f"no {e} sample"
        assert bool(k[e][0].any()) and bool(k[e][B - 1].any()), f"{e}: not in the first and the last image"
    assert torch.equal(om[..., :18] * 4096.0, torch.round(om[..., :18] * 4096.0))          # position = integer + offset exact in f32
    h, w = G.positions(om, c.H, c.W)
    assert torch.equal(h.float().double(), h) and torch.equal(w.float().double(), w)
    assert bool((k["outside"] & (k["on_minus_one"] | k["on_size"]) == (k["on_minus_one"] | k["on_size"])).all())
    for s in samples:                                        # the designed samples stand where they were put
        assert om[s.b, s.y, s.x, 2 * s.tap] == s.dh and om[s.b, s.y, s.x, 2 * s.tap + 1] == s.dw
    if c.kind != "window":
        return
    sides = set()
    for s in samples:
        if s.inwin is None:
            continue
        at = (s.b, s.y, s.x, s.tap)
        assert bool(k["inwin"][at]) == s.inwin, s
        if s.cls == "window_edge" and not k["outside"][at]:
            on_h, on_w = abs(abs(s.dh) - G.MG) <= G.EPS, abs(abs(s.dw) - G.MG) <= G.EPS
            sides.add(("h" if on_h and not on_w else "w" if on_w and not on_h else "both", s.dh < 0 or s.dw < 0, bool(k["inwin"][at])))
            assert bool(k["leaves"][at]) != s.inwin
    # in h and in w: towards the top / left and the bottom / right, the last sample inside and the first outside the margin
    assert sides >= {(d, neg, inwin) for d in ("h", "w") for neg in (True, False) for inwin in (True, False)}, sorted(sides)
    assert ("both", True, True) in sides and ("both", False, False) in sides
    if B > 1:
        assert {s for s in sides if s[0] == "both"} >= {("both", n, i) for n in (True, False) for i in (True, False)}
    assert bool(k["neg_index_both"].any()) and int(k["neg_index"].sum()) >= 3 * len({0, B - 1})
    row = k["inwin"][0, 3, :G.TW, 4]
    assert row.tolist() == [x % 2 == 0 for x in range(G.TW)] and bool(k["leaves"][0, 3, 1:G.TW:2, 4].all())


# ------------------------------------------------------------------------------------------ labels
def host_label(c, B):
    L = _lib.lib()
    p = C.c_void_p(BASE)
    mm = MASK_MODE[c.mask]
    with _lib.tuning(0), dry_run():
        L.ctdet_set_tuning_flags(0)
        if c.op == "cols":
            rc = L.ctdet_dcn_cols(p, c.Cin + SLICE_EXTRA, p, OM_STRIDE, p, B, c.H, c.W, c.Cin, mm, F16 if c.mode == "f16" else F32, None)
        elif c.op == "col2im":
            dom_f16 = c.mode == "f16" and c.dom_c == 32
            rc = L.ctdet_dcn_col2im_coord(p, p, c.Cin + SLICE_EXTRA, p, OM_STRIDE, p, p, c.dom_c, F16 if dom_f16 else F32, B, c.H, c.W,
                                          c.Cin, mm, int(c.chunked), COMPUTE[c.mode], None)
        else:
            K = (c.Cout + 31) // 32 * 32
            rc = L.ctdet_dcn_col2im_fused(p, K, K, p, p, p, c.Cin + SLICE_EXTRA, p, OM_STRIDE, p, p, c.dom_c, B, c.H, c.W, c.Cin, mm, None)
        assert rc == 0, (c, L.ctdet_last_error())
        return L.ctdet_last_kernel_label().decode()


@pytest.mark.parametrize("c", ROWS, ids=[case_id(c) for c in ROWS])
def test_row_selects_its_kernel(c):
    assert host_label(c, G.batch_of(c, 256)) == c.label, c
