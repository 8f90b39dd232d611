"""One row per forward conv kernel instantiation: the smallest shape that makes the launchers of csrc/conv_igemm.hip and
csrc/conv_f32.hip select it, and the label (ctdet_last_kernel_label) they must give for it.

test_conv_tiles_host.py replays every row through the library's dry run (no GPU) and asserts the label, so a row that no longer
reaches its kernel fails there; test_conv_tiles_gpu.py runs every row once and compares it with a float64 reference.

Completeness rule (asserted by the host test): every distinct label golden/g20_kernel_labels.json records for ctdet_conv2d_fwd,
ctdet_conv1x1_cat_fwd, ctdet_dcnv2_fwd, ctdet_dcnv2_fwd_cols and ctdet_dcnv2_offset_fwd (after the CORRECTED map of
test_kernel_labels_host.py) is the label of at least one row of the same entry point, and so is every label of EXTRA_LABELS
(variants the default DLA-34 model does not launch, but ResNet / VoVNet backbones and other class counts do).  A change to a
selector threshold must move the affected rows, not their labels.

How the shapes were chosen
  * 256-pixel tiles of the uniform-K / generic kernels with 32, 64 or 128 couts: ceil(M / 256) * (Cout_pad / tile) >= 512
    (launch_conv_f16_t, launch_conv_f32_t), reached with one image of ~16 k pixels and many couts.  M is never a multiple of 256
    (the last pixel tile is ragged); 120 x 137 = 65 and 137 x 139 = 75 pixel tiles are no multiple of 8 either, so the grid, which
    is rounded up to 8 pixel tiles, holds workgroups that must do nothing.
  * launch_halo_pair2 takes 64-cout tiles from (M / 256) * (Cout_pad / 64) >= 256 (the CU count), launch_halo<128> from 512
    workgroups.
  * everything else depends on channel counts and tile divisibility only and runs on one to four tiles.
Few input channels keep the float64 reference of the large rows at a few GMAC."""
from collections import namedtuple

Case = namedtuple("Case", "mode entry B H W Cin Cout k stride pad dil epilogue out_dtype label")
# mode: "f16" | "f32" | "f16x3" (ops.PackedConv's compute)
# entry: "conv2d" | "conv1x1_cat" | "dcnv2" | "dcnv2_cols" (ops.dcnv2(want_cols=True)) | "dcnv2_offset"
# Cin: channels, or the tuple of source channel counts of conv1x1_cat
# epilogue: subset of {"scale_bias", "residual", "relu"}; out_dtype: "f16" | "f32"
ENTRY_FN = {"conv2d": "ctdet_conv2d_fwd", "conv1x1_cat": "ctdet_conv1x1_cat_fwd", "dcnv2": "ctdet_dcnv2_fwd",
            "dcnv2_cols": "ctdet_dcnv2_fwd_cols", "dcnv2_offset": "ctdet_dcnv2_offset_fwd"}

SB = frozenset({"scale_bias"})
SBR = frozenset({"scale_bias", "relu"})
FULL = frozenset({"scale_bias", "residual", "relu"})


def _out(mode, out_dtype):
    return out_dtype or ("f16" if mode == "f16" else "f32")


def conv(mode, label, B, H, W, Cin, Cout, k=1, stride=1, pad=None, epi=SB, out=None, dil=1):
    return Case(mode, "conv2d", B, H, W, Cin, Cout, k, stride, k // 2 if pad is None else pad, dil, epi, _out(mode, out), label)


def cat(mode, label, B, H, W, cins, Cout, epi=SB, out=None):
    return Case(mode, "conv1x1_cat", B, H, W, tuple(cins), Cout, 1, 1, 0, 1, epi, _out(mode, out), label)


def dcn(mode, label, B, H, W, Cin, Cout, epi=SB, entry="dcnv2"):
    assert "residual" not in epi          # the deformable entry points take no residual
    return Case(mode, entry, B, H, W, Cin, Cout, 3, 1, 1, 1, epi, _out(mode, None), label)


def _uk(mode, bp, bc, form="conv", out=None):
    if mode == "f16":
        return f"conv_igemm_uk_kernel<{bp}x{bc},{form},{_out(mode, out)}>"
    return f"conv_{mode}_uk_kernel<{bp}x{bc}>"


def _generic(mode, bp, bc):
    return f"conv_igemm_dma_kernel<{bp}x{bc},f16>" if mode == "f16" else f"conv_{mode}_mfma_kernel<{bp}x{bc}>"


def _win(mode, k, cin, cout, s):
    if mode == "f16":
        return f"conv_win_kernel<{k}x{k},Cin{cin},Cout{cout},s{s},f16>"
    return f"conv_{mode}_win_kernel<{k}x{k},Cin{cin},Cout{cout},s{s}>"


def _tiled(mode):
    """the uniform-K, concat and generic rows every mode has.  C: the smallest Cin of the uniform-K kernel (f16: 32-channel
    chunks, f32 / f16x3: 16), G: a Cin it does not divide (the generic DMA / MFMA kernels)"""
    C, G = (32, 24) if mode == "f16" else (16, 12)
    rows = [
        # ---- 256 x 128: 65 x 8 = 520 (64 x 8 = 512 for 127 x 129) tiles
        conv(mode, _uk(mode, 256, 128), 1, 120, 137, C, 1024, epi=FULL),
        conv(mode, _uk(mode, 256, 128), 1, 120, 137, C, 1024, k=3),                 # 3x3 / s1 / p1 on a map no halo tile divides
        conv(mode, _uk(mode, 256, 128), 1, 254, 258, C, 1024, k=3, stride=2, epi=FULL),   # -> 127 x 129
        cat(mode, _uk(mode, 256, 128, "cat"), 1, 127, 129, (C, 2 * C, C), 1024, epi=FULL),
        conv(mode, _generic(mode, 256, 128), 1, 120, 137, G, 1024, epi=FULL),
        # ---- 256 x 64 and 256 x 32: 75 x 7 = 525 tiles
        conv(mode, _uk(mode, 256, 64), 1, 137, 139, C, 448),
        conv(mode, _uk(mode, 256, 32), 1, 137, 139, C, 224, epi=FULL),
        cat(mode, _uk(mode, 256, 64, "cat"), 1, 137, 139, (C, C), 448, epi=FULL),
        cat(mode, _uk(mode, 256, 32, "cat"), 1, 137, 139, (C, C), 224),
        conv(mode, _generic(mode, 256, 64), 1, 137, 139, G, 448, epi=FULL),
        conv(mode, _generic(mode, 256, 32), 1, 137, 139, G, 224),
        # ---- one short of the threshold (120 x 137: 65 x 7 = 455 tiles): the 128-pixel tiles
        conv(mode, _uk(mode, 128, 64), 1, 120, 137, C, 448, epi=FULL),
        # ---- 16-cout tiles are always 256 pixels: 6 pixel tiles in a grid of 8
        conv(mode, _uk(mode, 256, 16, out="f32"), 3, 19, 23, C, 4, out="f32"),
        conv(mode, _generic(mode, 256, 16) if mode != "f16" else "conv_igemm_dma_kernel<256x16,f16>", 3, 19, 23, G, 16, k=3, epi=FULL),
        # ---- small grids
        conv(mode, _uk(mode, 128, 32), 2, 9, 13, C, 28, k=3, epi=SBR),
        conv(mode, _generic(mode, 128, 128), 2, 9, 13, G, 128, k=3, epi=FULL),
    ]
    return rows


ROWS = _tiled("f16") + _tiled("f32") + _tiled("f16x3") + [
    # =========================== f16 ===========================
    # the heads' 256 -> 80 conv: one 128-cout tile with 48 padded couts, f32 output; 131070 pixels = 512 tiles
    conv("f16", _uk("f16", 256, 128, out="f32"), 2, 257, 255, 32, 80, out="f32"),
    # 128 x 128: below 512 tiles of 256 pixels, but 65 x 8 = 520 of 128 pixels (fewer: 128 x 64, the row after)
    conv("f16", _uk("f16", 128, 128), 1, 60, 137, 32, 1024),
    cat("f16", _uk("f16", 128, 128, "cat"), 1, 60, 137, (32, 32), 1024, epi=FULL),
    conv("f16", _uk("f16", 128, 64), 2, 9, 13, 32, 128, epi=FULL),
    conv("f16", _uk("f16", 128, 64, out="f32"), 2, 9, 13, 32, 64, k=3, epi=FULL, out="f32"),
    # halo-resident 3x3 / s1 / p1 (maps of 8 x 32-pixel tiles): 128-cout tiles from 512 workgroups on
    conv("f16", "conv3x3_halo_kernel<256x128,f16>", 1, 128, 128, 32, 1024, k=3, epi=FULL),
    conv("f16", "conv3x3_halo_kernel<256x64,f16>", 1, 24, 32, 32, 128, k=3),
    conv("f16", "conv3x3_halo_kernel<256x64,f32>", 1, 24, 32, 32, 64, k=3, epi=FULL, out="f32"),
    # 2 x 2 tiles: every tile has an image border and a neighbour, so the side halo columns hold pixels (on a map one tile
    # wide they are the zero page throughout); the same for the tap-pair kernels below
    conv("f16", "conv3x3_halo_kernel<256x64,f16>", 1, 16, 64, 32, 128, k=3, epi=FULL),
    # two taps per MFMA (Cin % 64 == 0), 8 x 32- and 16 x 16-pixel tiles
    conv("f16", "conv3x3_halo_tap2_kernel<256x64,f16>", 1, 24, 32, 64, 64, k=3, epi=FULL),
    conv("f16", "conv3x3_halo_tap2_kernel<256x32,f32>", 1, 24, 32, 64, 28, k=3, out="f32"),
    conv("f16", "conv3x3_halo_tap2_kernel<256x64,f16>", 1, 16, 64, 64, 64, k=3),
    conv("f16", "conv3x3_halo_tap2_kernel<16x16x64,f16>", 1, 16, 48, 64, 128, k=3),
    conv("f16", "conv3x3_halo_tap2_kernel<16x16x32,f32>", 1, 16, 48, 64, 28, k=3, epi=FULL, out="f32"),
    # narrow inputs on dense pixels: the LDS-window kernels of the DLA base layers
    conv("f16", _win("f16", 7, 8, 16, 1), 2, 16, 64, 8, 16, k=7, epi=SBR),
    conv("f16", _win("f16", 3, 16, 16, 1), 2, 16, 64, 16, 16, k=3, epi=FULL),
    conv("f16", _win("f16", 3, 16, 32, 2), 2, 16, 128, 16, 32, k=3, stride=2, epi=SBR),     # Wo % 64 == 0
    # DCNv2 LDS-window kernels: 8 x 16-pixel tiles, `edge` where the map is not made of them
    dcn("f16", "dcn_window_kernel<128x64,f16>", 1, 16, 32, 32, 64, epi=SBR),
    dcn("f16", "dcn_window_kernel<128x128,f16>", 1, 8, 16, 32, 256),
    dcn("f16", "dcn_window_kernel<128x64,f16,edge>", 2, 6, 10, 32, 64),
    dcn("f16", "dcn_window_kernel<128x128,f16,edge>", 1, 6, 10, 32, 128, epi=SBR),
    dcn("f16", "dcn_window_rows_kernel<128x64,offset conv fused>", 1, 16, 32, 32, 64, epi=SBR, entry="dcnv2_offset"),
    # =========================== f32 ===========================
    conv("f32", _uk("f32", 128, 128), 2, 9, 13, 16, 128, epi=FULL),
    cat("f32", _uk("f32", 128, 128, "cat"), 2, 9, 13, (16, 32), 128),
    conv("f32", _win("f32", 7, 4, 16, 1), 2, 14, 70, 4, 16, k=7, pad=0, epi=SBR),     # a pre-padded image
    conv("f32", _win("f32", 7, 8, 16, 1), 2, 8, 64, 8, 16, k=7),
    conv("f32", _win("f32", 3, 16, 16, 1), 2, 8, 64, 16, 16, k=3, epi=SBR),
    conv("f32", _win("f32", 3, 16, 32, 2), 2, 8, 64, 16, 32, k=3, stride=2),
    dcn("f32", "dcn_f32_window_kernel<8x16,64>", 1, 16, 32, 16, 64, epi=SBR),
    dcn("f32", "dcn_f32_window_kernel<8x16,128>", 1, 8, 16, 16, 128),
    dcn("f32", "dcn_f32_window_kernel<8x16,256>", 1, 8, 16, 16, 256, epi=SBR),
    dcn("f32", "dcn_f32_mfma_kernel<64x64>", 2, 6, 10, 16, 64),
    # =========================== f16x3 ===========================
    conv("f16x3", _uk("f16x3", 128, 128), 2, 9, 13, 16, 128, epi=FULL),
    cat("f16x3", _uk("f16x3", 128, 128, "cat"), 2, 9, 13, (16, 32), 128),
    # tap-pair kernels (3x3 / s1 / p1 on 8 x 32- or 16 x 16-pixel tiles).  korder 3 (Cin % 32 == 0): 64-cout tiles from
    # (M / 256) * (Cout_pad / 64) >= 256 on -- 16 x 16 and 25 x 11 here; one cout tile fewer gives the 32-cout tiles
    conv("f16x3", "conv3x3_halo_pair2_kernel<256x64,f16x3>", 1, 64, 64, 32, 1024, k=3, epi=FULL),
    conv("f16x3", "conv3x3_halo_pair2_kernel<256x32,f16x3>", 1, 64, 64, 32, 960, k=3),
    conv("f16x3", "conv3x3_halo_pair2_kernel<16x16x64,f16x3>", 1, 80, 80, 32, 704, k=3),
    conv("f16x3", "conv3x3_halo_pair2_kernel<16x16x32,f16x3>", 1, 80, 80, 32, 640, k=3, epi=FULL),
    conv("f16x3", "conv3x3_halo_pair2_kernel<16x16x32,f16x3>", 1, 16, 48, 32, 28, k=3),
    # korder 2 (an odd number of 16-channel chunks): 64-cout tiles whatever the grid
    conv("f16x3", "conv3x3_halo_pair_kernel<256x64,f16x3>", 1, 24, 32, 48, 192, k=3, epi=FULL),
    conv("f16x3", "conv3x3_halo_pair_kernel<256x32,f16x3>", 1, 24, 32, 48, 28, k=3),
    conv("f16x3", "conv3x3_halo_pair_kernel<256x64,f16x3>", 1, 16, 64, 48, 192, k=3),
    # 16 dense channels on 64-pixel rows take no pair image: the halo kernel on split operands
    conv("f16x3", "conv3x3_halo_kernel<256x64,f16x3>", 1, 24, 64, 16, 128, k=3, epi=FULL),
    conv("f16x3", _win("f16x3", 7, 8, 16, 1), 2, 8, 64, 8, 16, k=7, epi=SBR),
    conv("f16x3", _win("f16x3", 3, 16, 16, 1), 2, 8, 64, 16, 16, k=3),
    conv("f16x3", _win("f16x3", 3, 16, 32, 2), 2, 8, 64, 16, 32, k=3, stride=2, epi=SBR),
    dcn("f16x3", "dcn_f16x3_window_kernel<8x16,64>", 1, 16, 32, 16, 64, epi=SBR),
    dcn("f16x3", "dcn_f16x3_window_kernel<8x16,128>", 1, 16, 32, 16, 128),
    dcn("f16x3", "dcn_f16x3_window_kernel<8x16,256>", 1, 16, 32, 16, 256, epi=SBR),
    # the same kernels writing the sampled columns (training): one input for the three rows, see the GPU test
    dcn("f16x3", "dcn_f16x3_window_kernel<8x16,64>", 1, 16, 32, 16, 64, epi=SBR, entry="dcnv2_cols"),
    dcn("f16x3", "dcn_f16x3_window_kernel<8x16,128>", 1, 16, 32, 16, 128, entry="dcnv2_cols"),
    dcn("f16x3", "dcn_f16x3_window_kernel<8x16,256>", 1, 16, 32, 16, 256, epi=SBR, entry="dcnv2_cols"),
    dcn("f16x3", "dcn_f16x3_mfma_kernel<64x64>", 2, 6, 10, 16, 64, epi=SBR),
    dcn("f16x3", "dcn_f16x3_window_kernel<8x16,64,offset conv fused>", 1, 16, 32, 32, 64, epi=SBR, entry="dcnv2_offset"),
]

# labels the default model's recorded workload does not contain but that must each have a row (entry point, label)
EXTRA_LABELS = (
    [("conv2d", f"conv_igemm_dma_kernel<256x{bc},f16>") for bc in (32, 64, 128)]
    + [("conv2d", f"conv_{m}_mfma_kernel<256x{bc}>") for m in ("f32", "f16x3") for bc in (32, 64, 128)]
    + [("conv2d", _uk(m, 256, bc)) for m in ("f16", "f32", "f16x3") for bc in (32, 64)]
    + [("conv1x1_cat", _uk(m, 256, bc, "cat")) for m in ("f16", "f32", "f16x3") for bc in (32, 64)]
    + [("conv2d", "conv3x3_halo_kernel<256x128,f16>"),
       ("conv2d", "conv3x3_halo_pair2_kernel<16x16x64,f16x3>"),
       ("conv2d", "conv3x3_halo_pair_kernel<256x64,f16x3>")]
)


def case_id(c):
    cin = "+".join(map(str, c.Cin)) if isinstance(c.Cin, tuple) else str(c.Cin)
    geo = f"k{c.k}s{c.stride}p{c.pad}"
    epi = "".join(s for s, name in (("R", "residual"), ("A", "relu")) if name in c.epilogue)
    return f"{c.mode}-{c.entry}-{c.B}x{c.H}x{c.W}-{cin}to{c.Cout}-{geo}-{c.out_dtype}{'-' + epi if epi else ''}-{c.label}"
