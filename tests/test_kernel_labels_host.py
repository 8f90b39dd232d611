"""Kernel labels and shape predicates of the library, without a GPU: in label mode 2 (dry run) a launcher checks its
arguments, selects the kernel instantiation, names it and returns before the launch, so plain host buffers can stand in for
device pointers (they are never dereferenced)."""
import ctypes as C
import json
import os

import pytest

from detectron2_centernet_amd import _lib
from detectron2_centernet_amd._lib import F16, F16X3, F32, ConvDesc, DlaBaseDesc, HeadDesc

HERE = os.path.dirname(os.path.abspath(__file__))
_BUF = C.create_string_buffer(64)
BASE = (C.addressof(_BUF) + 15) & ~15       # a 16-byte aligned address to stand in for every device pointer

# golden/g20_kernel_labels.json: every distinct launch that the profiled passes of the default DLA-34 benchmark model issue
# (eval engine at batch 64, one training step at batch 16; f16x3, f16 and f32), recorded on an MI355X at the commit before
# the labels moved into the launchers: entry point, arguments (descriptor fields, integers, pointers as their address mod 16
# or null), tuning flags, and the label that ops.py derived from the shapes then.
ROWS = json.load(open(os.path.join(HERE, "golden", "g20_kernel_labels.json")))

# Rows whose recorded label was wrong: (recorded label, B, H, W, Cout_pad) -> the label of what launch_halo_pair2
# (csrc/conv_igemm.hip) launches.  The old derivation printed <256x{min(tile, 64)}> for every korder-3 conv.
CORRECTED = {
    # `if (a.W % 32 != 0)`: a 16-pixel-wide map runs on 16x16-pixel tiles, launch_halo_pair2_t<BC, 4, 1, 16>; 64 images x 8
    # cout tiles = 512 workgroups >= 256 CUs, so not small_grid: 64-cout tiles
    ("conv3x3_halo_pair2_kernel<256x64,f16x3>", 64, 16, 16, 512): "conv3x3_halo_pair2_kernel<16x16x64,f16x3>",
    # the same branch with pick_bc(28) = 32 <= 32: launch_halo_pair2_t<32, 4, 1, 16>
    ("conv3x3_halo_pair2_kernel<256x32,f16x3>", 64, 16, 16, 32): "conv3x3_halo_pair2_kernel<16x16x32,f16x3>",
    ("conv3x3_halo_pair2_kernel<256x32,f16x3>", 16, 16, 16, 32): "conv3x3_halo_pair2_kernel<16x16x32,f16x3>",
    # `small_grid`: (M / 256) * (Cout_pad / 64) = 16 * 8 = 128 < ctdet_device_cu_count() = 256 -> 32-cout tiles, and
    # `a.W % 32 != 0` -> 16x16-pixel tiles: launch_halo_pair2_t<32, 4, 1, 16>
    ("conv3x3_halo_pair2_kernel<256x64,f16x3>", 16, 16, 16, 512): "conv3x3_halo_pair2_kernel<16x16x32,f16x3>",
}

STRUCT = {"ctdet_head_fused_fwd": HeadDesc, "ctdet_head_fused_x3_fwd": HeadDesc,
          "ctdet_dla_base_fwd": DlaBaseDesc, "ctdet_dla_base_x3_fwd": DlaBaseDesc}


def _ptr(align):
    return None if align is None else BASE + align


def _arg(fn, arg):
    kind, v = arg
    if kind == "S":
        s = STRUCT.get(fn, ConvDesc)()
        for name, tp in s._fields_:
            if isinstance(v[name], list):
                field = getattr(s, name)
                for i, e in enumerate(v[name]):
                    field[i] = _ptr(e) if tp._type_ is C.c_void_p else e
            else:
                setattr(s, name, v[name])
        return C.byref(s)
    if kind == "p":
        return C.c_void_p(_ptr(v))
    if kind == "P":
        return (C.c_void_p * len(v))(*[_ptr(e) for e in v])
    if kind == "I":
        return (C.c_int32 * len(v))(*v)
    assert kind == "i"
    return v


class dry_run:
    def __enter__(self):
        assert _lib.lib().ctdet_set_label_mode(2) == 0

    def __exit__(self, *exc):
        _lib.lib().ctdet_set_label_mode(0)


def _label():
    return _lib.lib().ctdet_last_kernel_label().decode()


def test_recorded_launches_keep_their_labels():
    L = _lib.lib()
    assert {r["fn"] for r in ROWS} >= {"ctdet_conv2d_fwd", "ctdet_conv1x1_cat_fwd", "ctdet_dcnv2_fwd", "ctdet_dcnv2_offset_fwd",
                                       "ctdet_head_fused_fwd", "ctdet_head_fused_x3_fwd", "ctdet_dla_base_fwd", "ctdet_dla_base_x3_fwd"}
    used = set()
    for r in ROWS:
        d = r["args"][0][1]
        key = (r["label"], d["B"], d["H"], d["W"], d.get("Cout_pad"))
        want = CORRECTED.get(key, r["label"])
        used.add(key)
        with _lib.tuning(0), dry_run():
            L.ctdet_set_tuning_flags(r["flags"])
            rc = getattr(L, r["fn"])(*[_arg(r["fn"], a) for a in r["args"]], None)
            assert rc == 0, (r, L.ctdet_last_error())
            assert _label() == want, (r["what"], r["fn"], d, r["label"])
    assert set(CORRECTED) <= used      # every correction is a recorded launch


def _conv_desc(B=2, H=8, W=32, Cin=32, Cout=64, compute=F16X3, korder=0, Kpad=None, Cout_pad=64, in_stride=None, in_dil=1, Ho=None,
               Wo=None):
    d = ConvDesc()
    d.B, d.H, d.W, d.Cin, d.in_stride = B, H, W, Cin, in_stride or Cin
    d.Cout, d.Ho, d.Wo, d.out_stride = Cout, Ho or H, Wo or W, Cout
    d.R = d.S = 3
    d.stride = d.pad = d.dil = 1
    d.Kpad, d.Cout_pad = Kpad or 9 * Cin, Cout_pad
    d.compute_dtype, d.out_dtype, d.act = compute, (F16 if compute == F16 else F32), 0
    d.clamp_lo, d.clamp_hi, d.korder, d.in_dil = 0.0, 1.0, korder, in_dil
    return d


def _conv(d, x_align=0):
    p = C.c_void_p(BASE)
    return _lib.lib().ctdet_conv2d_fwd(C.byref(d), C.c_void_p(BASE + x_align), p, p, p, None, p, None)


def test_label_modes():
    L = _lib.lib()
    with dry_run():
        assert _conv(_conv_desc(compute=F16, korder=1)) == 0
        assert _label() == "conv3x3_halo_kernel<256x64,f16>"
        assert _conv(_conv_desc(compute=F16X3)) == 0                  # tap-major split weights: the halo kernel's SP form
        assert _label() == "conv3x3_halo_kernel<256x64,f16x3>"
        assert _conv(_conv_desc(compute=F32, Cin=6, Kpad=64)) == 0    # Cin % 4: no vector loads
        assert _label() == "conv_direct_f32_kernel<conv>"
    # mode 0: nothing is recorded (an empty batch returns before any launch; a rejected call likewise)
    assert L.ctdet_set_label_mode(0) == 0
    assert _conv(_conv_desc(B=0, compute=F16, korder=1, Cin=64)) == 0
    assert _conv(_conv_desc(compute=F16, korder=1, Cin=64, Kpad=7)) != 0
    assert _label() == "conv_direct_f32_kernel<conv>"
    assert L.ctdet_set_label_mode(3) != 0 and b"set_label_mode" in L.ctdet_last_error()


def _head(x3, W):
    d = HeadDesc()
    d.nheads, d.B, d.H, d.W, d.Cin, d.in_stride = 1, 1, 8, W, 32, 32
    d.w2[0] = d.b2[0] = d.y[0] = BASE
    d.y_stride[0], d.cout[0] = 4, 2
    p = C.c_void_p(BASE)
    if x3:
        return _lib.lib().ctdet_head_fused_x3_fwd(C.byref(d), p, p, p, p, None)
    return _lib.lib().ctdet_head_fused_fwd(C.byref(d), p, p, p, None)


@pytest.mark.parametrize("call", [
    lambda: _conv(_conv_desc(korder=3, Kpad=320)),                   # launch_halo_pair2: Kpad != Cin / 32 * 288
    lambda: _conv(_conv_desc(korder=2, Kpad=320, W=48)),             # launch_halo_pair: no 8x32 tiles
    lambda: _conv(_conv_desc(korder=2, Kpad=320), x_align=8),        # launch_conv_f32_t: x not 16-byte aligned
    lambda: _conv(_conv_desc(compute=F16, korder=1, Cout_pad=48)),   # launch_conv_f16_t: Cout_pad does not match the tile
    lambda: _conv(_conv_desc(Ho=9)),                                 # fill_args: output size
    lambda: _head(False, 24),                                        # launch_head_fused: W % 16
    lambda: _head(True, 24),                                         # launch_head_fused_x3: neither tile form
])
def test_rejected_calls_are_rejected_alike_in_a_dry_run(call):
    L = _lib.lib()
    L.ctdet_set_label_mode(0)
    rc0 = call()
    err0 = L.ctdet_last_error()
    with dry_run():
        rc2 = call()
        err2 = L.ctdet_last_error()
    assert rc0 == rc2 == -22 and err0 == err2 and err0


def test_cout_tile():
    assert [_lib.lib().ctdet_conv_cout_tile(c) for c in (4, 16, 28, 64, 80, 128, 768)] == [16, 16, 32, 64, 128, 128, 128]
    assert [_lib.lib().ctdet_conv_cout_tile(c) for c in (192, 160, 256)] == [64, 32, 128]


def _pair(H, W, Cin, in_stride=None, x_align=0, in_dil=1):
    ho = (H - 1) * in_dil + 1
    d = _conv_desc(H=H, W=W, Cin=Cin, in_stride=in_stride, in_dil=in_dil, Ho=ho, Wo=(W - 1) * in_dil + 1)
    return _lib.lib().ctdet_conv_pair_supported(C.byref(d), C.c_void_p(BASE + x_align))


def test_conv_pair_supported():
    """the korder of the pair image an f16x3 3x3 / s1 / p1 conv takes (0: none), for Cin = 16, 32, 48, 64"""
    with _lib.tuning(0):
        _lib.lib().ctdet_set_tuning_flags(0)
        # dense pixels, aligned x
        assert [_pair(8, 32, c) for c in (16, 32, 48, 64)] == [2, 3, 2, 3]         # 8x32 tiles only
        assert [_pair(16, 48, c) for c in (16, 32, 48, 64)] == [0, 3, 0, 3]        # 16x16 tiles only: korder 3 alone has them
        assert [_pair(8, 48, c) for c in (16, 32, 48, 64)] == [0, 0, 0, 0]         # neither tile form
        assert [_pair(16, 64, c) for c in (16, 32, 48, 64)] == [0, 3, 2, 3]        # 16 dense channels on 64-pixel rows: the
        assert [_pair(16, 128, c) for c in (16, 32)] == [0, 3]                     # LDS-window kernel's layer
        # channel slices of a wider buffer
        assert [_pair(16, 64, c, in_stride=c + 16) for c in (16, 32, 48, 64)] == [2, 3, 2, 3]
        assert [_pair(8, 32, c, in_stride=c + 2) for c in (16, 32, 48, 64)] == [0, 0, 0, 0]      # pixel rows not 16-byte multiples
        # x at an 8-byte offset
        assert [_pair(8, 32, c, x_align=8) for c in (16, 32, 48, 64)] == [0, 0, 0, 0]
        assert [_pair(16, 64, c, in_stride=c + 16, x_align=8) for c in (16, 32)] == [0, 0]
        # a zero-stuffed input (the input gradient of a strided conv)
        assert [_pair(8, 32, c, in_dil=2) for c in (16, 32)] == [0, 0]
        # other geometries and modes have no pair image
        d = _conv_desc(H=8, W=32, Cin=32, compute=F32)
        assert _lib.lib().ctdet_conv_pair_supported(C.byref(d), C.c_void_p(BASE)) == 0
        d = _conv_desc(H=8, W=32, Cin=32)
        d.pad, d.Ho, d.Wo = 0, 6, 30
        assert _lib.lib().ctdet_conv_pair_supported(C.byref(d), C.c_void_p(BASE)) == 0
    with _lib.tuning(_lib.TUNE_NO_HALO):
        assert [_pair(8, 32, c) for c in (16, 32, 48, 64)] == [0, 0, 0, 0]
        assert [_pair(16, 48, c) for c in (32, 64)] == [0, 0]


def _heads_ok(compute, H, W, Cin, in_stride=None, x_align=0):
    return _lib.lib().ctdet_head_fused_supported(compute, H, W, Cin, in_stride or Cin, C.c_void_p(BASE + x_align))


def test_head_fused_supported():
    # f16: 8x16-pixel tiles, Cin % 32 == 0
    assert [_heads_ok(F16, h, w, 64) for h, w in ((8, 16), (8, 32), (16, 48), (8, 24), (4, 16), (12, 16))] == [1, 1, 1, 0, 0, 0]
    assert [_heads_ok(F16, 8, 16, c) for c in (16, 32, 48, 64)] == [0, 1, 0, 1]
    assert _heads_ok(F16, 8, 16, 32, in_stride=40) == 1
    # f16x3: 8x32- or 16x16-pixel tiles, Cin % 32 == 0, 16-byte pixel rows from a 16-byte aligned x
    assert [_heads_ok(F16X3, h, w, 64) for h, w in ((8, 32), (16, 16), (16, 48), (8, 48), (8, 16), (4, 32))] == [1, 1, 1, 0, 0, 0]
    assert [_heads_ok(F16X3, 8, 32, c) for c in (16, 32, 48, 64)] == [0, 1, 0, 1]
    assert [_heads_ok(F16X3, 8, 32, 32, in_stride=s) for s in (36, 34)] == [1, 0]
    assert _heads_ok(F16X3, 8, 32, 32, x_align=8) == 0
    assert _heads_ok(F32, 8, 32, 32) == 0
