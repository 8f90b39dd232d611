"""f16x3 DCNv2 with its offset / mask conv computed in the same kernel (ops.dcnv2_offset in F16X3,
dcn_split_window_kernel<2, 64, ..., fused>) against the two-launch path (ops.conv2d + ops.dcnv2).

Where the two-launch path runs the offset conv on the tap-pair kernel (conv3x3_halo_pair2_kernel: maps divisible by 8x32 or
16x16 pixels) the fused kernel repeats that kernel's MFMA accumulations one for one and the outputs must be EQUAL.  On the other
maps (8x16, 24x48 here) the two-launch path takes the halo-split kernel, whose products are grouped differently, so the offsets
differ in their last bits; there the bound is the fused-vs-unfused bound of test_heads_fused_x3_gpu.py,
1e-5 * max(1, |ref|max), and both paths are set against an f64 restatement: the fused one may be no further from it than the
two-launch one (plus that same bound's worth of slack for the comparison's own rounding)."""
import pytest
import torch
import torch.nn.functional as F

from oracle import ctdet_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    import detectron2_centernet_amd.ops as ops

    return ops


def make_layer(ops, dev, Cin, Cout, sigma, seed):
    """DCN weights with a folded BatchNorm (scale, bias) and an offset / mask conv whose output has a standard deviation of about
    `sigma` pixels on unit-normal activations"""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    scale = torch.rand(Cout, generator=g) + 0.5
    bias = torch.randn(Cout, generator=g) * 0.3
    w_off = torch.randn(27, Cin, 3, 3, generator=g) * (sigma / (Cin * 9) ** 0.5)
    b_off = torch.randn(27, generator=g) * 0.2
    p = ops.PackedConv(w.to(dev), scale.to(dev), bias.to(dev), stride=1, pad=1, compute=ops.F16X3)
    p_off = ops.PackedConv(w_off.to(dev), None, b_off.to(dev), stride=1, pad=1, compute=ops.F16X3)
    return (w, scale, bias, w_off, b_off), p, p_off


def two_launch(ops, x, p_off, p, act):
    om = ops.conv2d(x, p_off, out_dtype=torch.float32)
    return ops.dcnv2(x, om, p, act=act)


def pair_kernel_serves(H, W):
    """does the two-launch path run the offset conv on conv3x3_halo_pair2_kernel? (halo_pair_x_ok, korder 3)"""
    return (H % 8 == 0 and W % 32 == 0) or (H % 16 == 0 and W % 16 == 0)


def sample_census(x_nchw, w_off, b_off):
    """(samples outside the +-4 px window of their 8x16 tile, samples with a corner or all of them outside the image), from the
    reference offsets on the CPU"""
    B, _, H, W = x_nchw.shape
    om = F.conv2d(x_nchw.double(), w_off.double(), b_off.double(), 1, 1)
    ys = torch.arange(H).view(1, H, 1).double()
    xs = torch.arange(W).view(1, 1, W).double()
    far = outside = 0
    for t in range(9):
        h_im = ys - 1 + t // 3 + om[:, 2 * t]
        w_im = xs - 1 + t % 3 + om[:, 2 * t + 1]
        valid = (h_im > -1) & (w_im > -1) & (h_im < H) & (w_im < W)
        hl, wl = torch.floor(h_im), torch.floor(w_im)
        wr = hl - (torch.div(ys, 8, rounding_mode="floor") * 8 - 5)
        wc = wl - (torch.div(xs, 16, rounding_mode="floor") * 16 - 5)
        inside = (wr >= 0) & (wr + 1 < 18) & (wc >= 0) & (wc + 1 < 26)
        far += int((valid & ~inside).sum())
        outside += int((~valid | (hl < 0) | (wl < 0) | (hl + 1 > H - 1) | (wl + 1 > W - 1)).sum())
    return far, outside


def ref64(x_nchw, layer):
    w, scale, bias, w_off, b_off = [t.double() for t in layer]
    om = F.conv2d(x_nchw.double(), w_off, b_off, 1, 1)
    y = O.dcnv2_forward(x_nchw.double(), om[:, :18], torch.sigmoid(om[:, 18:27]), w, None, 1, 1, 1)
    return (y * scale.view(1, -1, 1, 1) + bias.view(1, -1, 1, 1)).relu().permute(0, 2, 3, 1)


LAYERS = [(64, 64), (128, 64), (256, 64)]
MAPS = [(8, 16), (24, 48), (64, 64)]


@pytest.mark.parametrize("sigma", [0.5, 3.0])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hw", MAPS)
@pytest.mark.parametrize("layer", LAYERS)
def test_fused_equals_two_launch(ops, dev, layer, hw, B, sigma):
    Cin, Cout = layer
    H, W = hw
    tensors, p, p_off = make_layer(ops, dev, Cin, Cout, sigma, seed=Cin + H + int(10 * sigma))
    x = torch.randn(B, H, W, Cin, generator=torch.Generator().manual_seed(B * H + W))
    if sigma > 1:
        far, outside = sample_census(x.permute(0, 3, 1, 2), tensors[3], tensors[4])
        assert outside > 0, "no sample leaves the image: the zero corners are not exercised"
        # a valid sample of an 8x16 map is always inside the 18x26 window; on the larger maps the slow path must run
        assert far > 0 or (H, W) == (8, 16), "no sample leaves the window: the slow path is not exercised"
    xd = x.to(dev)
    assert ops.dcnv2_offset_supported(xd, p_off, p)
    for act in (ops.ACT_RELU, ops.ACT_NONE):
        y = ops.dcnv2_offset(xd, p_off, p, act=act)
        y2 = two_launch(ops, xd, p_off, p, act)
        assert y.shape == y2.shape == (B, H, W, Cout) and y.dtype == torch.float32
        d = (y - y2).abs().max().item()
        print(f"{Cin}->{Cout} {H}x{W} B={B} sigma={sigma} act={act}: max |fused - two-launch| = {d:.3e}")
        if pair_kernel_serves(H, W):
            assert torch.equal(y, y2), d
        else:
            tol = 1e-5 * max(1.0, y2.abs().max().item())
            assert d <= tol, (d, tol)
            if act == ops.ACT_RELU:
                ref = ref64(x.permute(0, 3, 1, 2), tensors)
                e1 = (y.double().cpu() - ref).abs().max().item()
                e2 = (y2.double().cpu() - ref).abs().max().item()
                print(f"    vs f64: fused {e1:.3e}, two-launch {e2:.3e}")
                tol = 1e-5 * max(1.0, ref.abs().max().item())
                assert e1 <= tol and e2 <= tol and e1 <= e2 + tol, (e1, e2, tol)


def test_graph_replay_is_bit_exact(ops, dev):
    tensors, p, p_off = make_layer(ops, dev, 64, 64, 3.0, seed=11)
    x = torch.randn(4, 32, 64, 64, generator=torch.Generator().manual_seed(12)).to(dev)
    out = torch.empty(4, 32, 64, 64, device=dev)
    ops.dcnv2_offset(x, p_off, p, out=out, act=ops.ACT_RELU)        # warm-up outside the capture (packs the pair image)
    torch.cuda.synchronize()
    eager = out.clone()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            ops.dcnv2_offset(x, p_off, p, out=out, act=ops.ACT_RELU)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(4):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    assert torch.equal(eager, two_launch(ops, x, p_off, p, ops.ACT_RELU))


def test_batch_invariance(ops, dev):
    """an image gives the same output in a batch of 64 and in a batch of 4"""
    tensors, p, p_off = make_layer(ops, dev, 128, 64, 3.0, seed=21)
    x = torch.randn(64, 32, 32, 128, generator=torch.Generator().manual_seed(22)).to(dev)
    y64 = ops.dcnv2_offset(x, p_off, p, act=ops.ACT_RELU)
    for b0 in (0, 28, 60):
        y4 = ops.dcnv2_offset(x[b0:b0 + 4].contiguous(), p_off, p, act=ops.ACT_RELU)
        assert torch.equal(y4, y64[b0:b0 + 4])


def test_fullsize_fused_equals_two_launch(ops, dev):
    """the layer that carries most of the time: 64 x 128 x 128 x 64 -> 64"""
    tensors, p, p_off = make_layer(ops, dev, 64, 64, 1.5, seed=31)
    x = torch.randn(64, 128, 128, 64, generator=torch.Generator().manual_seed(32)).to(dev)
    assert ops.dcnv2_offset_supported(x, p_off, p)
    y = ops.dcnv2_offset(x, p_off, p, act=ops.ACT_RELU)
    assert torch.equal(y, ops.dcnv2_offset(x, p_off, p, act=ops.ACT_RELU))
    y2 = two_launch(ops, x, p_off, p, ops.ACT_RELU)
    assert torch.equal(y, y2), (y - y2).abs().max().item()


def test_predicate_and_selection(ops, dev, monkeypatch):
    """what ops.dcnv2_offset_supported refuses, and that DCN.hip_forward takes the fused call unless switched off"""
    from detectron2_centernet_amd.layers import hipnn
    from detectron2_centernet_amd.layers.deform_conv import DCN

    _, p, p_off = make_layer(ops, dev, 64, 64, 0.5, seed=41)
    x = torch.randn(2, 16, 32, 64, device=dev)
    assert ops.dcnv2_offset_supported(x, p_off, p)
    assert ops.dcnv2_offset_supported(x[:1], p_off, p) and ops.dcnv2_offset_supported(x.repeat(8, 1, 1, 1), p_off, p)
    assert not ops.dcnv2_offset_supported(x[:, :, :24].contiguous(), p_off, p)          # W % 16
    assert not ops.dcnv2_offset_supported(x[:, :12].contiguous(), p_off, p)             # H % 8
    buf = torch.randn(2 * 16 * 32 * 64 + 2, device=dev)
    assert not ops.dcnv2_offset_supported(buf[2:].view(2, 16, 32, 64), p_off, p)        # x at an 8-byte offset
    _, p48, p_off48 = make_layer(ops, dev, 48, 64, 0.5, seed=42)
    assert not ops.dcnv2_offset_supported(torch.randn(2, 16, 32, 48, device=dev), p_off48, p48)      # Cin % 32
    _, p256, p_off64 = make_layer(ops, dev, 64, 256, 0.5, seed=43)
    assert p256.Cout_pad == 256 and not ops.dcnv2_offset_supported(x, p_off64, p256)    # more than one cout tile

    m = DCN(64, 64, (3, 3), 1, 1).to(dev)
    m.conv_offset_mask.weight.data.normal_(0, 0.05)
    m.conv_offset_mask.bias.data.normal_(0, 0.2)
    ctx = hipnn.Ctx(ops.F16X3)
    calls = []
    real = ops.dcnv2_offset
    monkeypatch.setattr(ops, "dcnv2_offset", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    y = m.hip_forward(x, ctx, act=ops.ACT_RELU)
    assert calls == [1]
    monkeypatch.setattr(ops, "DCN_X3_FUSED", False)
    y2 = m.hip_forward(x, ctx, act=ops.ACT_RELU)
    assert calls == [1] and torch.equal(y, y2)
    monkeypatch.setattr(ops, "DCN_X3_FUSED", True)
    monkeypatch.setattr(ops, "RANGE_CHECK", True)
    assert torch.equal(m.hip_forward(x, ctx, act=ops.ACT_RELU), y) and calls == [1]
