"""What the dry run says is what runs: for one small call per launch family, the label a profiled call records
(ops.PROFILE) is the label the dry run (label mode 2) gave for the same call, profiling leaves label mode 0 behind, and the
result is bit-identical with and without profiling."""
import pytest
import torch

from detectron2_centernet_amd import _lib

pytestmark = pytest.mark.gpu


def _w(g, *shape):
    fan = shape[1] * shape[2] * shape[3]
    return torch.randn(*shape, generator=g) / fan ** 0.5


def _conv(compute, Cin, Cout, k, H, W, B=1, cat=0, **kw):
    def make(ops, dev):
        g = torch.Generator().manual_seed(Cin + Cout + H)
        dt = torch.float16 if compute == _lib.F16 else torch.float32
        pc = ops.PackedConv(_w(g, Cout, Cin, k, k).to(dev), None, torch.randn(Cout, generator=g).to(dev), stride=1, pad=k // 2,
                            compute=compute, **kw)
        x = torch.randn(B, H, W, Cin, generator=g).to(dt).to(dev)
        if cat:
            xs = [x[..., i * (Cin // cat):(i + 1) * (Cin // cat)].contiguous() for i in range(cat)]
            return lambda: [ops.conv1x1_cat(xs, pc, act=ops.ACT_RELU)]
        return lambda: [ops.conv2d(x, pc, act=ops.ACT_RELU)]
    return make


def _dcn(compute, Cin, Cout, H, W, fused_offset=False):
    def make(ops, dev):
        g = torch.Generator().manual_seed(Cin + Cout + H)
        dt = torch.float16 if compute == _lib.F16 else torch.float32
        kw = {"cout_align": 64} if compute == _lib.F16 else {}
        pc = ops.PackedConv(_w(g, Cout, Cin, 3, 3).to(dev), None, torch.randn(Cout, generator=g).to(dev), stride=1, pad=1,
                            compute=compute, **kw)
        x = torch.randn(1, H, W, Cin, generator=g).to(dt).to(dev)
        if fused_offset:
            po = ops.PackedConv((_w(g, 27, Cin, 3, 3) * 0.3).to(dev), None, (torch.randn(27, generator=g) * 0.3).to(dev), stride=1,
                                pad=1, compute=compute)
            assert ops.dcnv2_offset_supported(x, po, pc)
            return lambda: [ops.dcnv2_offset(x, po, pc, act=ops.ACT_RELU)]
        om = (torch.randn(1, H, W, 28, generator=g) * 0.5).to(dev)
        return lambda: [ops.dcnv2(x, om, pc, act=ops.ACT_RELU)]
    return make


def _heads(compute, H, W):
    def make(ops, dev):
        g = torch.Generator().manual_seed(H + W)
        ph = ops.PackedHeads([_w(g, 256, 32, 3, 3).to(dev) for _ in range(2)], [torch.randn(256, generator=g).to(dev) for _ in range(2)],
                             [_w(g, c, 256, 1, 1).to(dev) for c in (5, 2)], [torch.randn(c, generator=g).to(dev) for c in (5, 2)],
                             [ops.ACT_SIGMOID_CLAMP, ops.ACT_NONE], compute=compute)
        x = torch.randn(1, H, W, 32, generator=g).to(torch.float16 if compute == _lib.F16 else torch.float32).to(dev)
        assert ops.heads_fused_ok(x, compute)
        return lambda: ops.heads_fused(x, ph, clamp=(1e-4, 1 - 1e-4))
    return make


def _base(x3):
    def make(ops, dev):
        g = torch.Generator().manual_seed(7)
        args = []
        for shape in ((16, 3, 7, 7), (16, 16, 3, 3), (32, 16, 3, 3)):
            args += [_w(g, *shape).to(dev), ((torch.rand(shape[0], generator=g) + 0.5).to(dev), torch.randn(shape[0], generator=g).to(dev))]
        pb = (ops.PackedDlaBaseX3 if x3 else ops.PackedDlaBase)(*args)
        img = torch.randint(0, 256, (1, 3, 30, 60), generator=g, dtype=torch.uint8).to(dev)
        return lambda: [ops.dla_base_fused(img, [0.4, 0.45, 0.5], [0.22, 0.23, 0.24], 32, 64, pb)]
    return make


F16, F32, F16X3 = _lib.F16, _lib.F32, _lib.F16X3
# (label the launcher must give, the call): one per launch family of conv_igemm.hip, conv_f32.hip and dla_base.hip
CASES = [
    ("conv3x3_halo_kernel<256x64,f16>", _conv(F16, 32, 64, 3, 8, 32)),
    ("conv3x3_halo_tap2_kernel<256x64,f16>", _conv(F16, 64, 64, 3, 8, 32)),
    ("conv3x3_halo_tap2_kernel<16x16x64,f16>", _conv(F16, 64, 64, 3, 16, 16)),
    ("conv_igemm_uk_kernel<128x64,conv,f16>", _conv(F16, 32, 64, 1, 8, 8)),
    ("conv_igemm_uk_kernel<128x64,cat,f16>", _conv(F16, 64, 64, 1, 8, 8, cat=2)),
    ("conv_igemm_dma_kernel<128x64,f16>", _conv(F16, 16, 64, 3, 8, 24)),
    ("conv_smallc_kernel<Cout16,K160,f16>", _conv(F16, 16, 16, 3, 8, 64)),
    ("conv_win_kernel<3x3,Cin16,Cout16,s1,f16>", _conv(F16, 16, 16, 3, 16, 64)),
    ("dcn_window_kernel<128x64,f16>", _dcn(F16, 32, 64, 8, 16)),
    ("dcn_window_kernel<128x128,f16>", _dcn(F16, 32, 128, 8, 16)),
    ("dcn_window_kernel<128x64,f16,edge>", _dcn(F16, 32, 64, 6, 10)),
    ("dcn_window_rows_kernel<128x64,offset conv fused>", _dcn(F16, 32, 64, 8, 16, fused_offset=True)),
    ("head_fused_kernel<128x256,f16>", _heads(F16, 8, 16)),
    ("dla_base_fused_kernel<u8|f32 -> 32ch,f16>", _base(False)),
    ("conv_f32_mfma_kernel<128x32>", _conv(F32, 8, 32, 3, 8, 8)),
    ("conv_f32_uk_kernel<128x64>", _conv(F32, 32, 64, 1, 8, 8)),
    ("conv_f32_win_kernel<3x3,Cin16,Cout16,s1>", _conv(F32, 16, 16, 3, 8, 64)),
    ("conv_direct_f32_kernel<conv>", _conv(F32, 6, 8, 3, 8, 8)),
    ("dcn_f32_window_kernel<8x16,64>", _dcn(F32, 16, 64, 8, 16)),
    ("dcn_f32_mfma_kernel<64x64>", _dcn(F32, 16, 64, 6, 10)),
    ("conv_direct_f32_kernel<dcn>", _dcn(F32, 8, 8, 6, 10)),
    ("conv3x3_halo_pair_kernel<256x64,f16x3>", _conv(F16X3, 48, 64, 3, 8, 32)),
    ("conv3x3_halo_pair2_kernel<256x32,f16x3>", _conv(F16X3, 32, 64, 3, 8, 32)),        # one pixel tile: a small grid
    ("conv3x3_halo_pair2_kernel<256x64,f16x3>", _conv(F16X3, 32, 64, 3, 64, 64, B=16)),   # 256 pixel tiles
    ("conv3x3_halo_pair2_kernel<16x16x32,f16x3>", _conv(F16X3, 32, 64, 3, 16, 16)),
    ("conv3x3_halo_kernel<256x64,f16x3>", _conv(F16X3, 16, 64, 3, 8, 64)),               # 16 dense channels, 64-pixel rows: no pair image
    ("conv_f16x3_uk_kernel<128x64>", _conv(F16X3, 32, 64, 1, 8, 8)),
    ("conv_f16x3_win_kernel<3x3,Cin16,Cout16,s1>", _conv(F16X3, 16, 16, 3, 8, 64)),
    ("dcn_f16x3_window_kernel<8x16,64>", _dcn(F16X3, 16, 64, 8, 16)),
    ("head_fused_x3_kernel<256x256,f16x3>", _heads(F16X3, 8, 32)),
    ("head_fused_x3_kernel<16x16x256,f16x3>", _heads(F16X3, 16, 16)),
    ("dla_base_x3_kernel<u8|f32 -> 32ch,f16x3>", _base(True)),
]


def _label():
    return _lib.lib().ctdet_last_kernel_label().decode()


@pytest.mark.parametrize("expect,make", CASES, ids=[c[0] for c in CASES])
def test_profiled_label_is_the_dry_run_label(dev, expect, make):
    import detectron2_centernet_amd.ops as ops

    L = _lib.lib()
    run = make(ops, dev)
    plain = [t.clone() for t in run()]
    L.ctdet_set_label_mode(2)
    try:
        run()                              # checks and selection only: nothing is launched, the outputs stay unwritten
        dry = _label()
    finally:
        L.ctdet_set_label_mode(0)
    ops.PROFILE.clear()
    ops.PROFILE_ON = True
    try:
        profiled = run()                   # the same launch PROFILE_REP times into the same buffers
    finally:
        ops.PROFILE_ON = False
    assert len(ops.PROFILE) == 1 and ops.PROFILE[-1][0] == dry == expect
    # label mode 0 again: a launch of another kernel leaves the label alone
    other = CASES[3] if expect != CASES[3][0] else CASES[15]
    other[1](ops, dev)()
    assert _label() == expect
    torch.cuda.synchronize()
    assert len(plain) == len(profiled) and all(torch.equal(a, b) for a, b in zip(plain, profiled))
    ops.PROFILE.clear()
