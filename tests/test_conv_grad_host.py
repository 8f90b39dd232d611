"""The case table of conv_grad_cases.py without a GPU: every weight-gradient row, replayed through the library's dry run on
stand-in pointers, gives the row's label, split included; the regime facts a row exists for follow from label and shape by the
arithmetic below; rows are distinct; every label family of the weight-gradient launchers has its rows; and the float64
references of the cases module agree with torch's double autograd of F.conv2d / F.conv_transpose2d."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import conv_grad_cases as G
from conv_grad_cases import ROWS, case_id, out_hw
from detectron2_centernet_amd import _lib
from detectron2_centernet_amd._lib import F16, F16X3, F32, ConvDesc
from test_kernel_labels_host import BASE, dry_run

COMPUTE = {"f16": F16, "f32": F32, "f16x3": F16X3}
SLICE_EXTRA = 16        # the GPU test's wider buffers of the wgrad_oihw rows carry this many more channels per pixel
WGRAD = [c for c in ROWS if c.op in ("wgrad", "wgrad_oihw")]
OTHER = [c for c in ROWS if c.op in ("dgrad", "convT")]


def wgrad_desc(c):
    """the ctdet_conv_desc ops_train.conv_wgrad builds for the row on the GPU test's tensors"""
    Ho, Wo = out_hw(c)
    extra = SLICE_EXTRA if c.op == "wgrad_oihw" else 0
    d = ConvDesc()
    d.B, d.H, d.W, d.Cin, d.in_stride = c.B, c.H, c.W, c.cin_c, c.cin_c + extra
    d.Cout, d.Ho, d.Wo, d.out_stride = kernel_cout(c), Ho, Wo, c.cout_c + extra
    d.R = d.S = c.k
    d.stride, d.pad, d.dil = c.stride, c.pad, c.dil
    d.compute_dtype = COMPUTE[c.mode]
    return d


def kernel_cout(c):
    """the Cout the launch is given: the carried count where the layer pads its output gradient (wgrad_oihw drops the padded
    rows in the kernel), the real count for a plain weight gradient over a wider dY (the full-size test's offset conv)"""
    return c.cout_c if c.op == "wgrad_oihw" else c.Cout


def host_label(c):
    L = _lib.lib()
    d, p = wgrad_desc(c), C.c_void_p(BASE)
    with _lib.tuning(0), dry_run():
        L.ctdet_set_tuning_flags(0)
        if c.op == "wgrad":
            rc = L.ctdet_conv_wgrad(C.byref(d), p, p, p, 1.0, None)
        else:
            rc = L.ctdet_conv_wgrad_oihw(C.byref(d), p, p, p, 0.5, c.k * c.k, c.cin_c, c.Cin, c.Cout, None)
        assert rc == 0, (c, L.ctdet_last_error())
        return L.ctdet_last_kernel_label().decode()


@pytest.mark.parametrize("c", WGRAD, ids=[case_id(c) for c in WGRAD])
def test_row_selects_its_kernel_and_split(c):
    assert host_label(c) == c.label, c


def _facts(c):
    """every regime fact that holds for a weight-gradient row, from its label and shape alone"""
    kind = G.kernel_kind(c)
    split = G.label_split(c.label)[1]
    ranges, total = G.pixel_ranges(c)
    Ho, Wo = out_hw(c)
    M, K, Cout = c.B * Ho * Wo, c.k * c.k * c.cin_c, kernel_cout(c)
    have = set()
    work = [hi - lo for lo, hi in ranges]
    assert sum(work) == total and all(lo <= hi for lo, hi in ranges), c     # the ranges tile the pixels / tiles exactly once
    if any(w == 0 for w in work):
        assert (split - 1) * max(work) >= total
        have.add("empty_wg")
    if c.dil > 1:
        have.add("dilation")
    if c.stride == 2:
        have.add("stride2")
    have.add(f"taps={c.k * c.k}")
    if kind in ("win", "narrow"):
        tx, ty = c.W // 32, c.H // 8
        assert c.H % 8 == 0 and c.W % 32 == 0 and total == c.B * tx * ty
        have.add(f"tiles={total}")
        have.add(f"tiles_per_wg={max(work)}")
        if tx >= 2 and ty >= 2:
            have.add("halo_all_sides")
        if tx >= 3:
            have.add("middle_tile_column")
    if kind == "win":
        assert c.cin_c % 32 == 0 and split == min(max(1, 256 // (c.cin_c // 32 * -(-Cout // 32))), total)
        have.add("swizzle" if split % 8 == 0 else "no_swizzle")
        if Cout % 32:
            have.add("partial_cout_tile" if Cout < 32 else "second_cout_tile_partial")
    if kind == "generic":
        have.add("swizzle" if split % 8 == 0 else "no_swizzle")
        have.add(f"split={split}")
        last = [w for w in work if w][-1]
        have.add(f"last_range={last}")
        if last % 64:
            have.add("ragged_last_range")
        if K % 128:
            have.add("partial_k_tile")
        if Cout % 64:
            have.add("partial_cout_tile")
        pow2 = Ho & (Ho - 1) == 0 and Wo & (Wo - 1) == 0
        have.add("pow2_index" if pow2 else "div_index")
        if M <= 64 and split == 1:
            have.add("single_k_step")
    if kind == "f32":
        if K % 16:
            have.add("k_tail")
        if Cout % 16:
            have.add("cout_tail")
        if any(w % 16 for w in work):
            have.add("range_tail")
        if split < -(-M // 64):             # the 4096-block budget binds, not the 64-pixel minimum of a range
            assert split == 4096 // (-(-K // 16) * -(-Cout // 16))
            have.add("split_from_blocks")
    if c.op == "wgrad_oihw":
        have.add("layout_1x1" if c.k == 1 else "layout_rxs")
        if c.Cin < c.cin_c:
            have.add("cin_dropped")
        if c.Cout < c.cout_c:
            have.add("cout_dropped")
    return have


@pytest.mark.parametrize("c", WGRAD, ids=[case_id(c) for c in WGRAD])
def test_row_reaches_its_regime(c):
    missing = set(c.facts) - _facts(c)
    assert not missing, (c, sorted(_facts(c)))


def test_regimes_of_the_issue_are_present():
    """every regime the table was built for is the fact of a row, in f16 and f16x3 (the f32 kernel's in f32)"""
    for mode in ("f16", "f16x3"):
        facts = {(G.kernel_kind(c), f) for c in WGRAD if c.mode == mode for f in c.facts}
        assert facts >= {("win", "swizzle"), ("win", "tiles_per_wg=2"), ("win", "empty_wg"), ("win", "partial_cout_tile"),
                         ("win", "second_cout_tile_partial"), ("win", "halo_all_sides"), ("win", "middle_tile_column"),
                         ("narrow", "tiles_per_wg=1"), ("narrow", "tiles_per_wg=2"), ("generic", "swizzle"),
                         ("generic", "no_swizzle"), ("generic", "ragged_last_range"), ("generic", "partial_k_tile"),
                         ("generic", "partial_cout_tile"), ("generic", "div_index"), ("generic", "pow2_index"),
                         ("generic", "single_k_step"), ("generic", "dilation"), ("generic", "taps=16"),
                         ("generic", "layout_1x1"), ("generic", "layout_rxs"), ("narrow", "cin_dropped"), ("win", "cout_dropped")}, mode
    facts = {f for c in WGRAD if c.mode == "f32" for f in c.facts}
    assert facts >= {"k_tail", "cout_tail", "range_tail", "split_from_blocks", "stride2", "taps=16", "dilation", "layout_1x1", "layout_rxs", "cin_dropped",
                     "cout_dropped"}


def test_rows_are_well_formed():
    assert len(set(ROWS)) == len(ROWS), "two identical rows"
    assert len({case_id(c) for c in ROWS}) == len(ROWS)
    for c in ROWS:
        assert c.mode in G.MODES and c.op in ("wgrad", "wgrad_oihw", "dgrad", "convT"), c
        assert c.cin_c >= c.Cin and c.cout_c >= c.Cout, c
    for c in OTHER:      # the forward labels these rows name are asserted by the GPU test from the real calls
        labels = (c.label,) if c.op == "dgrad" else c.label
        assert len(labels) == (1 if c.op == "dgrad" else 3), c
        assert all(isinstance(s, str) and s.startswith("conv") and s.endswith(">") for s in labels[:2 if c.op == "convT" else 1]), c
        if c.op == "convT":
            assert G.label_split(labels[2])[0].startswith("conv_wgrad_"), c
        assert c.Cin != c.Cout, c      # a transposition error must show
    for op in ("dgrad", "convT"):
        assert {c.mode for c in OTHER if c.op == op} == set(G.MODES)


def test_every_weight_gradient_label_family_has_rows():
    for mode in ("f16", "f16x3"):
        fams = {G.label_split(c.label)[0] for c in WGRAD if c.mode == mode}
        assert fams == {f.format(m=mode) for f in G.WGRAD_FAMILIES}, (mode, fams)
    assert {G.label_split(c.label)[0] for c in WGRAD if c.mode == "f32"} == {G.F32_FAMILY}
    assert sum(1 for c in WGRAD if c.mode == "f32" and c.op == "wgrad") >= 6


def test_seam_pixels_cover_every_range():
    for c in WGRAD:
        px = set(G.seam_pixels(c))
        Ho, Wo = out_hw(c)
        M = c.B * Ho * Wo
        assert {0, M - 1} <= px
        ranges, _ = G.pixel_ranges(c)
        if G.kernel_kind(c) in ("generic", "f32"):
            for lo, hi in ranges:
                assert lo >= hi or {lo, hi - 1} <= px, (c, lo, hi)
        else:
            assert len(px) >= 4 * c.B * (c.H // 8) * (c.W // 32)


# ------------------------------------------------------------------------------------------ the references themselves
REF_SHAPES = [  # B, H, W, Cin, Cout, k, stride, pad, dil
    (2, 7, 6, 3, 5, 3, 1, 1, 1),
    (1, 9, 8, 4, 2, 3, 2, 1, 1),
    (2, 8, 5, 2, 3, 4, 2, 1, 1),
    (1, 10, 9, 3, 4, 3, 1, 2, 2),
]


@pytest.mark.parametrize("shape", REF_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_references_against_torch_double_autograd(shape):
    B, H, W, Cin, Cout, k, s, p, dil = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(B, Cin, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(Cout, Cin, k, k, generator=g, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, None, s, p, dil)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    dx, dw = torch.autograd.grad(y, (x, w), dy)
    xn, dyn = x.detach().permute(0, 2, 3, 1), dy.permute(0, 2, 3, 1)
    assert (G.wgrad_ref(xn, dyn, k, s, p, dil).permute(0, 3, 1, 2) - dw).abs().max() <= 1e-12
    if dil == 1:
        assert (G.dgrad_ref(dyn, w.detach(), s, p, H, W).permute(0, 3, 1, 2) - dx).abs().max() <= 1e-12
        assert (G.conv_ref(xn, w.detach(), s, p).permute(0, 3, 1, 2) - y.detach()).abs().max() <= 1e-12
        # the transposed conv of the same geometry: weight [Cin_t = Cout, Cout_t = Cin, k, k] over a map of y's size
        xt = torch.randn(B, Cout, y.shape[2], y.shape[3], generator=g, dtype=torch.float64, requires_grad=True)
        wt = torch.randn(Cout, Cin, k, k, generator=g, dtype=torch.float64, requires_grad=True)
        yt = F.conv_transpose2d(xt, wt, None, s, p)
        dyt = torch.randn(yt.shape, generator=g, dtype=torch.float64)
        dxt, dwt = torch.autograd.grad(yt, (xt, wt), dyt)
        ry, rdx, rdw = G.conv_transpose_refs(xt.detach().permute(0, 2, 3, 1), wt.detach(), dyt.permute(0, 2, 3, 1), s, p)
        assert (ry.permute(0, 3, 1, 2) - yt.detach()).abs().max() <= 1e-12
        assert (rdx.permute(0, 3, 1, 2) - dxt).abs().max() <= 1e-12
        assert (rdw - dwt).abs().max() <= 1e-12


def test_impulse_patches_are_the_weight_gradient_of_an_impulse():
    """impulse_patches against wgrad_ref on one-hot dY, exactly (one term per element)"""
    for c in (G._row("f32", "wgrad", "x", 2, 6, 7, 3, 4, 3, stride=2), G._row("f32", "wgrad", "x", 1, 8, 8, 2, 4, 3, pad=2, dil=2)):
        Ho, Wo = out_hw(c)
        x = torch.randint(-8, 9, (c.B, c.H, c.W, c.Cin), generator=torch.Generator().manual_seed(3)).double()
        px = [0, Wo - 1, c.B * Ho * Wo - 1, Ho * Wo // 2]
        dy = torch.zeros(c.B * Ho * Wo, c.Cout, dtype=torch.float64)
        for n, m in enumerate(px):
            dy[m, n] = 1.0
        ref = G.wgrad_ref(x, dy.view(c.B, Ho, Wo, c.Cout), c.k, c.stride, c.pad, c.dil)
        assert torch.equal(ref, G.impulse_patches(x, c, px))
