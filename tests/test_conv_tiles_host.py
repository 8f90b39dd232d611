"""The case table of conv_tile_cases.py against the library's dry run, without a GPU: every row's descriptor, built by the rules
of ops.PackedConv, selects the kernel instantiation the row names; the table covers every label of the recorded workload
(golden/g20_kernel_labels.json) and of EXTRA_LABELS; no two rows are the same."""
import ctypes as C

import pytest

from conv_tile_cases import ENTRY_FN, EXTRA_LABELS, ROWS, case_id
from detectron2_centernet_amd import _lib
from detectron2_centernet_amd._lib import F16, F16X3, F32, ConvDesc
from test_kernel_labels_host import BASE, CORRECTED, ROWS as RECORDED, dry_run

COMPUTE = {"f16": F16, "f32": F32, "f16x3": F16X3}
GUARD_CHANNELS = 8         # the GPU test's output buffer is this much wider than Cout_eff (its write guard)


def round_up(a, b):
    return (a + b - 1) // b * b


def host_desc(c):
    """the ctdet_conv_desc ops.PackedConv.desc() builds for row c on dense inputs and the GPU test's output view"""
    L = _lib.lib()
    deform = c.entry.startswith("dcnv2")
    compute = COMPUTE[c.mode]
    Cin = sum(c.Cin) if isinstance(c.Cin, tuple) else c.Cin
    Cout_eff = round_up(c.Cout, 4)
    K = c.k * c.k * Cin
    cout_align = 64 if (deform and compute == F16) else 1          # what the f16 DCN layers pack with
    tile = max(L.ctdet_conv_cout_tile(Cout_eff), cout_align)
    d = ConvDesc()
    d.B, d.H, d.W, d.Cin, d.in_stride = c.B, c.H, c.W, Cin, Cin
    d.Ho = (c.H + 2 * c.pad - (c.dil * (c.k - 1) + 1)) // c.stride + 1
    d.Wo = (c.W + 2 * c.pad - (c.dil * (c.k - 1) + 1)) // c.stride + 1
    d.Cout, d.out_stride = Cout_eff, Cout_eff + GUARD_CHANNELS
    d.R = d.S = c.k
    d.stride, d.pad, d.dil = c.stride, c.pad, c.dil
    d.Kpad, d.Cout_pad = round_up(K, 32 if compute == F16 else 16), round_up(Cout_eff, tile)
    d.compute_dtype, d.out_dtype = compute, {"f16": F16, "f32": F32}[c.out_dtype]
    d.act = 1 if "relu" in c.epilogue else 0
    d.res_stride = Cout_eff if "residual" in c.epilogue else 0
    d.clamp_lo, d.clamp_hi, d.in_dil = 0.0, 1.0, 1
    d.korder = 1 if (compute == F16 and Cin % 32 == 0 and c.k > 1) else 0
    if (c.entry == "conv2d" and compute == F16X3 and (c.k, c.stride, c.pad, c.dil) == (3, 1, 1, 1) and Cin % 16 == 0):
        korder = L.ctdet_conv_pair_supported(C.byref(d), C.c_void_p(BASE))       # PackedConv._pair_image
        if korder:
            nch = Cin // 16
            d.korder, d.Kpad, d.Cout_pad = korder, (nch // 2 * 288 if korder == 3 else nch * 160), round_up(d.Cout_pad, 32)
    return d


def host_call(c):
    """the row's entry point on stand-in pointers (a dry run never dereferences them)"""
    L = _lib.lib()
    d, p = host_desc(c), C.c_void_p(BASE)
    res = p if "residual" in c.epilogue else None
    if c.entry == "conv2d":
        return L.ctdet_conv2d_fwd(C.byref(d), p, p, p, p, res, p, None)
    if c.entry == "conv1x1_cat":
        n = len(c.Cin)
        return L.ctdet_conv1x1_cat_fwd(C.byref(d), (C.c_void_p * n)(*[BASE] * n), (C.c_int32 * n)(*c.Cin), (C.c_int32 * n)(*c.Cin), n,
                                       p, p, p, res, p, None)
    if c.entry == "dcnv2":
        return L.ctdet_dcnv2_fwd(C.byref(d), p, p, 28, _lib.DCN_MASK_LOGIT, p, p, p, p, None)
    if c.entry == "dcnv2_cols":
        assert L.ctdet_dcnv2_cols_supported(C.byref(d), p, p), "ops.dcnv2(want_cols=True) would not take the cols entry point"
        return L.ctdet_dcnv2_fwd_cols(C.byref(d), p, p, 28, _lib.DCN_MASK_LOGIT, p, p, p, p, p, None)
    assert c.entry == "dcnv2_offset"
    assert L.ctdet_dcnv2_offset_supported(C.byref(d))
    return L.ctdet_dcnv2_offset_fwd(C.byref(d), p, p, p, None, 0, p, p, p, p, None)


@pytest.mark.parametrize("c", ROWS, ids=[case_id(c) for c in ROWS])
def test_row_selects_its_kernel(c):
    L = _lib.lib()
    with _lib.tuning(0), dry_run():
        L.ctdet_set_tuning_flags(0)
        rc = host_call(c)
        assert rc == 0, (c, L.ctdet_last_error())
        assert L.ctdet_last_kernel_label().decode() == c.label, c


def test_rows_are_well_formed():
    assert len(set(ROWS)) == len(ROWS), "two identical rows"
    assert len({case_id(c) for c in ROWS}) == len(ROWS)
    for c in ROWS:
        assert "scale_bias" in c.epilogue and c.epilogue <= {"scale_bias", "residual", "relu"}, c
        assert c.entry in ENTRY_FN and c.mode in COMPUTE and c.out_dtype in ("f16", "f32"), c
        assert c.mode == "f16" or c.out_dtype == "f32", c
    both = sum(1 for c in ROWS if {"residual", "relu"} <= c.epilogue)
    conv_rows = sum(1 for c in ROWS if not c.entry.startswith("dcnv2"))
    assert 0.4 * conv_rows <= both <= 0.6 * conv_rows, (both, conv_rows)      # about half; the DCN entry points take no residual


def test_256_pixel_rows_have_ragged_edges():
    """M is no multiple of the 256-pixel tile, and per family one row's pixel-tile count is no multiple of 8 (the grid is)"""
    families = {}
    for c in ROWS:
        if not any(s in c.label for s in ("_uk_kernel<256x", "_dma_kernel<256x", "_mfma_kernel<256x")) or c.label.startswith("dcn"):
            continue
        d = host_desc(c)
        M = d.B * d.Ho * d.Wo
        assert M % 256, c
        fam = c.label.split("<")[0] + ("/cat" if c.entry == "conv1x1_cat" else "")
        families.setdefault(fam, []).append((M + 255) // 256)
    assert len(families) == 9, sorted(families)      # uniform-K conv, uniform-K cat, generic: f16, f32, f16x3
    for fam, tiles in families.items():
        assert any(t % 8 for t in tiles), (fam, tiles)


def test_table_covers_the_recorded_workload_and_the_extra_labels():
    have = {(ENTRY_FN[c.entry], c.label) for c in ROWS}
    want = set()
    for r in RECORDED:
        if r["fn"] in ENTRY_FN.values():
            d = r["args"][0][1]
            want.add((r["fn"], CORRECTED.get((r["label"], d["B"], d["H"], d["W"], d.get("Cout_pad")), r["label"])))
    assert {fn for fn, _ in want} == set(ENTRY_FN.values())
    assert len(want) >= 60
    assert not want - have, sorted(want - have)
    extra = {(ENTRY_FN[e], label) for e, label in EXTRA_LABELS}
    assert len(extra) == 24
    assert not extra - have, sorted(extra - have)
