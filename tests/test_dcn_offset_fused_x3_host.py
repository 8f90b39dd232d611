"""Host side of the f16x3 DCNv2 with the fused offset / mask conv (no GPU: dry-run launches, ctdet_set_label_mode(2)): the label
of the launch, the truth table of ctdet_dcnv2_offset_supported for F16X3, and that what it refuses fails alike in a dry run."""
import ctypes as C

import pytest

from detectron2_centernet_amd import _lib
from detectron2_centernet_amd._lib import F16, F16X3, F32, ConvDesc

_BUF = C.create_string_buffer(64)
BASE = (C.addressof(_BUF) + 15) & ~15       # a 16-byte aligned address to stand in for every device pointer


def desc(B=2, H=16, W=32, Cin=64, Cout=64, Cout_pad=64, in_stride=None, compute=F16X3, korder=0, Kpad=None):
    d = ConvDesc()
    d.B, d.H, d.W, d.Cin, d.in_stride = B, H, W, Cin, in_stride or Cin
    d.Cout, d.Ho, d.Wo, d.out_stride = Cout, H, W, Cout
    d.R = d.S = 3
    d.stride = d.pad = d.dil = 1
    d.Kpad, d.Cout_pad = Kpad or 9 * Cin, Cout_pad
    d.compute_dtype, d.out_dtype, d.act = compute, (F16 if compute == F16 else F32), 1
    d.clamp_lo, d.clamp_hi, d.korder, d.in_dil = 0.0, 1.0, korder, 1
    return d


def ok(**kw):
    return _lib.lib().ctdet_dcnv2_offset_supported(C.byref(desc(**kw)))


def fwd(d, x_align=0, w_off_align=0, om_out=None):
    p = C.c_void_p(BASE)
    return _lib.lib().ctdet_dcnv2_offset_fwd(C.byref(d), C.c_void_p(BASE + x_align), C.c_void_p(BASE + w_off_align), p, om_out, 0,
                                             p, p, p, p, None)


class dry_run:
    def __enter__(self):
        assert _lib.lib().ctdet_set_label_mode(2) == 0

    def __exit__(self, *exc):
        _lib.lib().ctdet_set_label_mode(0)


def test_supported_truth_table_x3():
    with _lib.tuning(0):
        _lib.lib().ctdet_set_tuning_flags(0)
        # the DLA-34 layers in reach (one 64-cout tile covers Cout), at any batch size
        assert [ok(H=h, W=w, Cin=c) for h, w, c in ((128, 128, 64), (64, 64, 128), (32, 32, 256))] == [1, 1, 1]
        assert [ok(B=b) for b in (1, 3, 4, 64)] == [1, 1, 1, 1]
        assert [ok(H=h, W=w) for h, w in ((8, 16), (24, 48), (64, 64), (16, 16))] == [1, 1, 1, 1]
        # Cin in 32-channel chunk pairs
        assert [ok(Cin=c) for c in (16, 32, 48, 64, 96)] == [0, 1, 0, 1, 1]
        # the 8x16 tile
        assert [ok(H=h, W=w) for h, w in ((8, 24), (12, 16), (4, 16), (8, 8))] == [0, 0, 0, 0]
        # one cout tile: 128 and 256 packed rows are two-launch layers
        assert [ok(Cout=c, Cout_pad=cp) for c, cp in ((28, 64), (64, 64), (128, 128), (256, 256), (64, 128))] == [1, 1, 0, 0, 0]
        # pixel rows of 16-byte multiples; tap-major split weights of the DCN itself; f32 output; 3x3 / s1 / p1
        assert [ok(in_stride=s) for s in (64, 80, 66)] == [1, 1, 0]
        assert ok(korder=3, Kpad=576) == 0 and ok(Kpad=640) == 0
        d = desc()
        d.out_dtype = F16
        assert _lib.lib().ctdet_dcnv2_offset_supported(C.byref(d)) == 0
        d = desc()
        d.pad, d.Ho, d.Wo = 0, 14, 30
        assert _lib.lib().ctdet_dcnv2_offset_supported(C.byref(d)) == 0
        assert ok(compute=F32) == 0
        # the f16 form keeps its own rule (chunk-major weights)
        assert ok(compute=F16, korder=1) == 1 and ok(compute=F16, korder=0) == 0
    with _lib.tuning(_lib.TUNE_NO_F32_DCN_WINDOW):
        assert ok() == 0


def test_label_of_the_fused_launch():
    L = _lib.lib()
    with _lib.tuning(0), dry_run():
        L.ctdet_set_tuning_flags(0)
        for h, w, c in ((128, 128, 64), (64, 64, 128), (32, 32, 256), (8, 16, 32)):
            assert fwd(desc(B=64, H=h, W=w, Cin=c)) == 0, L.ctdet_last_error()
            assert L.ctdet_last_kernel_label().decode() == "dcn_f16x3_window_kernel<8x16,64,offset conv fused>"
        # the two-launch DCNv2 of the same layer keeps its label
        p = C.c_void_p(BASE)
        assert L.ctdet_dcnv2_fwd(C.byref(desc(B=64, H=128, W=128)), p, p, 28, 0, p, p, p, p, None) == 0
        assert L.ctdet_last_kernel_label().decode() == "dcn_f16x3_window_kernel<8x16,64>"


@pytest.mark.parametrize("call", [
    lambda: fwd(desc(Cin=48)),                       # Cin % 32
    lambda: fwd(desc(W=24)),                         # W % 16
    lambda: fwd(desc(Cout=256, Cout_pad=256)),       # more than one cout tile
    lambda: fwd(desc(), x_align=8),                  # x not 16-byte aligned
    lambda: fwd(desc(), w_off_align=8),              # the offset conv's pair image not 16-byte aligned
    lambda: fwd(desc(), om_out=C.c_void_p(BASE)),    # the inference form keeps no offsets
])
def test_refused_calls_are_refused_alike_in_a_dry_run(call):
    L = _lib.lib()
    L.ctdet_set_label_mode(0)
    rc0 = call()
    err0 = L.ctdet_last_error()
    with dry_run():
        rc2 = call()
        err2 = L.ctdet_last_error()
    assert rc0 == rc2 == -22 and err0 == err2 and err0
