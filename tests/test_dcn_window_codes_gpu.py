"""The f16x3 DCNv2 sampler (dcn_split_window_kernel) keeps the window addresses of a lane's pixels in registers for the whole
tile and a wave-uniform bit per tap for "some lane is far"; only a tap whose bit is set re-reads the code table and runs the slow
path.  Every form of the kernel against the f64 restatement (oracle.ctdet_oracle.dcnv2_forward) with the bound
tests/test_dcn_offset_fused_x3_gpu.py uses for this kernel, 1e-5 * max(1, |ref|max), at the smallest shapes at which the registers
can go wrong: one tile (8x16) and four (16x32, every border), batch 1 and 2, one channel chunk (the registers are used once) and
four (re-used), 64 couts (<2,64>: two launches and the fused offset conv), 128 (<1,128>) and 40 (padded), and offsets that are
zero, near (sigma 1 px), mostly far (sigma 6 px), far for ONE lane of a wave's second pixel tile, and outside the image."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import ctdet_oracle as O

pytestmark = pytest.mark.gpu

TH, TW, MG = 8, 16, 4                     # the kernel's tile and the margin of its window around the tile's 3x3 footprint
MAPS = [(8, 16), (16, 32)]
KINDS = ["zero", "sigma1", "sigma6", "single7", "outside"]
COUTS = [64, 128, 40]
FAR_PIXEL = (7, 27)                       # tile row 7, tile column 11: the second pixel tile (p = 1) of wave 3 in <2,64>
FAR_TAP = 4


@pytest.fixture(scope="module")
def ops():
    import detectron2_centernet_amd.ops as ops

    return ops


def far_share(dh, dw, H, W):
    """(share of all samples with a corner more than MG px outside the 3x3 footprint of their pixel's 8x16 tile -- the kernel's
    rule for leaving the window --, number of those that are valid, i.e. that the slow path has to fetch) for offsets
    dh, dw [B, 9, H, W]"""
    ys = torch.arange(H).view(1, 1, H, 1).double()
    xs = torch.arange(W).view(1, 1, 1, W).double()
    tr = (torch.arange(9) // 3).view(1, 9, 1, 1).double()
    ts = (torch.arange(9) % 3).view(1, 9, 1, 1).double()
    h_im, w_im = ys - 1 + tr + dh.double(), xs - 1 + ts + dw.double()
    valid = (h_im > -1) & (w_im > -1) & (h_im < H) & (w_im < W)
    wr = torch.floor(h_im) - (torch.div(ys, TH, rounding_mode="floor") * TH - 1 - MG)
    wc = torch.floor(w_im) - (torch.div(xs, TW, rounding_mode="floor") * TW - 1 - MG)
    inside = (wr >= 0) & (wr + 1 < TH + 2 + 2 * MG) & (wc >= 0) & (wc + 1 < TW + 2 + 2 * MG)
    return (~inside).double().mean().item(), int((valid & ~inside).sum()), int((~valid).sum())


def offsets_of(kind, B, H, W, seed):
    """offset / mask tensor [B, H, W, 27] (dh, dw interleaved per tap, then 9 mask logits)"""
    g = torch.Generator().manual_seed(seed)
    om = torch.zeros(B, H, W, 27)
    om[..., 18:] = torch.randn(B, H, W, 9, generator=g)
    if kind == "sigma1":
        om[..., :18] = torch.randn(B, H, W, 18, generator=g)
    elif kind == "sigma6":
        om[..., :18] = torch.randn(B, H, W, 18, generator=g) * 6.0
    elif kind == "single7":
        if H > TH:                        # row 7 + 7 = 14: inside the image, two rows below the window of tile row 0
            om[B - 1, FAR_PIXEL[0], FAR_PIXEL[1], 2 * FAR_TAP] = 7.0
        else:                             # one tile: nothing valid is far; the same lane, 7 px to the left
            om[B - 1, FAR_PIXEL[0] % H, FAR_PIXEL[1] % W, 2 * FAR_TAP + 1] = -7.0
    elif kind == "outside":               # sigma 1 px, and a third of the samples thrown far outside the image: invalid
        om[..., :18] = torch.randn(B, H, W, 18, generator=g)
        throw = torch.rand(B, H, W, 18, generator=g) < 1.0 / 3
        om[..., :18] += throw.float() * 40.0 * torch.sign(torch.randn(B, H, W, 18, generator=g))
    return om


def check_census(kind, om, H, W):
    dh, dw = om[..., 0:18:2].permute(0, 3, 1, 2), om[..., 1:18:2].permute(0, 3, 1, 2)
    share, far_valid, invalid = far_share(dh, dw, H, W)
    print(f"    {kind}: {share:.3f} of the samples leave the margin, {far_valid} of them valid, {invalid} invalid")
    if kind in ("zero", "sigma1"):
        assert (share == 0.0) if kind == "zero" else (share < 0.01)
    if kind == "sigma6":
        assert 0.10 <= share <= 0.90, share
        assert far_valid > 0 or (H, W) == (TH, TW)         # (a valid sample of a one-tile map is always inside its window)
    if kind == "single7":
        assert far_valid == (1 if H > TH else 0) and round(share * dh.numel()) == (1 if H > TH else 0)
    if kind == "outside":
        assert invalid > dh.numel() // 5


_REF = {}


def layer_and_ref(hw, B, Cin, kind):
    """x, offsets, a 128-cout layer (the 64- and 40-cout layers are its first rows) and the f64 result, computed once"""
    key = (hw, B, Cin, kind)
    if key not in _REF:
        H, W = hw
        seed = 1000 * KINDS.index(kind) + 100 * B + Cin + H
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(B, H, W, Cin, generator=g)
        w = torch.randn(128, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
        scale = torch.rand(128, generator=g) + 0.5
        bias = torch.randn(128, generator=g) * 0.3
        om = offsets_of(kind, B, H, W, seed + 1)
        omc = om.permute(0, 3, 1, 2).double()
        y = O.dcnv2_forward(x.permute(0, 3, 1, 2).double(), omc[:, :18], torch.sigmoid(omc[:, 18:27]), w.double(), None, 1, 1, 1)
        ref = (y * scale.double().view(1, -1, 1, 1) + bias.double().view(1, -1, 1, 1)).permute(0, 2, 3, 1)
        _REF[key] = (x, om, w, scale, bias, ref)
    return _REF[key]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("Cin", [16, 64])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("hw", MAPS)
def test_two_launch_forms_vs_f64(ops, dev, hw, B, Cin, kind):
    H, W = hw
    x, om, w, scale, bias, ref = layer_and_ref(hw, B, Cin, kind)
    check_census(kind, om, H, W)
    xd, omd = x.to(dev), om.to(dev)
    for Cout in COUTS:
        p = ops.PackedConv(w[:Cout].to(dev), scale[:Cout].to(dev), bias[:Cout].to(dev), stride=1, pad=1, compute=ops.F16X3, cout_align=64)
        assert p.Cout_pad == (128 if Cout == 128 else 64)
        y = ops.dcnv2(xd, omd, p, act=ops.ACT_NONE)
        assert y.shape == (B, H, W, Cout) and y.dtype == torch.float32
        r = ref[..., :Cout]
        err = (y.double().cpu() - r).abs().max().item()
        tol = 1e-5 * max(1.0, r.abs().max().item())
        print(f"    {Cin}->{Cout} {H}x{W} B={B} {kind}: max |y - f64| = {err:.3e} (bound {tol:.3e})")
        assert err <= tol, (Cout, err, tol)
        # the training form, which also writes the sampled columns, is the same sampler: equal outputs
        y2, cols = ops.dcnv2(xd, omd, p, act=ops.ACT_NONE, want_cols=True)
        assert cols is not None and torch.equal(y2, y)


def fused_layer(ops, dev, hw, B, Cin, Cout, kind):
    """the fused form computes its own offsets: an offset conv that produces each kind from x"""
    H, W = hw
    seed = 5000 + 1000 * KINDS.index(kind) + 100 * B + Cin + H + Cout
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, Cin, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    scale = torch.rand(Cout, generator=g) + 0.5
    bias = torch.randn(Cout, generator=g) * 0.3
    w_off = torch.zeros(27, Cin, 3, 3)
    b_off = torch.zeros(27)
    w_off[18:] = torch.randn(9, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    if kind in ("sigma1", "sigma6", "outside"):
        sigma = 6.0 if kind == "sigma6" else 1.0
        w_off[:18] = torch.randn(18, Cin, 3, 3, generator=g) * (sigma / (Cin * 9) ** 0.5)
    if kind == "outside":                 # taps 0 and 8 of every pixel leave the image altogether
        b_off[0], b_off[17] = -40.0, 40.0
    if kind == "single7":                 # channel 0 of x is 1 at one pixel and 0 elsewhere; the centre tap of one offset row reads it
        x[..., 0] = 0.0
        if H > TH:
            x[B - 1, FAR_PIXEL[0], FAR_PIXEL[1], 0] = 1.0
            w_off[2 * FAR_TAP, 0, 1, 1] = 7.0
        else:
            x[B - 1, FAR_PIXEL[0] % H, FAR_PIXEL[1] % W, 0] = 1.0
            w_off[2 * FAR_TAP + 1, 0, 1, 1] = -7.0
    p = ops.PackedConv(w.to(dev), scale.to(dev), bias.to(dev), stride=1, pad=1, compute=ops.F16X3, cout_align=64)
    p_off = ops.PackedConv(w_off.to(dev), None, b_off.to(dev), stride=1, pad=1, compute=ops.F16X3)
    xc = x.permute(0, 3, 1, 2).double()
    om = F.conv2d(xc, w_off.double(), b_off.double(), 1, 1)
    y = O.dcnv2_forward(xc, om[:, :18], torch.sigmoid(om[:, 18:27]), w.double(), None, 1, 1, 1)
    ref = (y * scale.double().view(1, -1, 1, 1) + bias.double().view(1, -1, 1, 1)).permute(0, 2, 3, 1)
    return x, om.permute(0, 2, 3, 1).float(), p, p_off, ref


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("Cin", [32, 64])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("hw", MAPS)
def test_fused_form_vs_f64(ops, dev, hw, B, Cin, kind):
    H, W = hw
    for Cout in (64, 40):
        x, om, p, p_off, ref = fused_layer(ops, dev, hw, B, Cin, Cout, kind)
        check_census(kind, om, H, W)
        xd = x.to(dev)
        assert ops.dcnv2_offset_supported(xd, p_off, p)
        y = ops.dcnv2_offset(xd, p_off, p, act=ops.ACT_NONE)
        assert y.shape == (B, H, W, Cout) and y.dtype == torch.float32
        err = (y.double().cpu() - ref).abs().max().item()
        tol = 1e-5 * max(1.0, ref.abs().max().item())
        print(f"    fused {Cin}->{Cout} {H}x{W} B={B} {kind}: max |y - f64| = {err:.3e} (bound {tol:.3e})")
        assert err <= tol, (Cout, err, tol)
        flag = torch.ones(1, dtype=torch.int32, device=dev)                 # the form with the finite test in its epilogue
        y2 = ops.dcnv2_offset(xd, p_off, p, act=ops.ACT_NONE, finite_flag=flag)
        assert torch.equal(y2, y) and flag.item() == 1


def _capture(fn):
    fn()                                   # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    return g


@pytest.mark.parametrize("Cout", [64, 128])
def test_graph_replay_on_two_offset_tensors(ops, dev, Cout):
    """[kernel] captured once and replayed on far offsets, then on zero offsets, then on far ones again: nothing derived from
    one offset tensor (addresses, far bits) may survive into the next replay"""
    hw, B, Cin = (16, 32), 2, 64
    x, _, w, scale, bias, _ = layer_and_ref(hw, B, Cin, "sigma6")             # one x and one layer; only the offsets change
    p = ops.PackedConv(w[:Cout].to(dev), scale[:Cout].to(dev), bias[:Cout].to(dev), stride=1, pad=1, compute=ops.F16X3, cout_align=64)
    xbuf = x.to(dev)
    ombuf = torch.zeros(B, *hw, 27, device=dev)
    out = torch.empty(B, *hw, Cout, device=dev)
    g = _capture(lambda: ops.dcnv2(xbuf, ombuf, p, out=out, act=ops.ACT_NONE))
    xc = x.permute(0, 3, 1, 2).double()
    for kind in ("sigma6", "zero", "single7", "sigma6"):
        om = layer_and_ref(hw, B, Cin, kind)[1]
        ombuf.copy_(om)
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ops.dcnv2(xbuf, ombuf, p, act=ops.ACT_NONE))
        omc = om.permute(0, 3, 1, 2).double()
        y = O.dcnv2_forward(xc, omc[:, :18], torch.sigmoid(omc[:, 18:27]), w[:Cout].double(), None, 1, 1, 1)
        r = (y * scale[:Cout].double().view(1, -1, 1, 1) + bias[:Cout].double().view(1, -1, 1, 1)).permute(0, 2, 3, 1)
        err = (out.double().cpu() - r).abs().max().item()
        assert err <= 1e-5 * max(1.0, r.abs().max().item()), (kind, err)


def test_graph_replay_fused(ops, dev):
    """the fused form, whose offsets come from x: replays on an x with far offsets and on one with a single far lane"""
    hw, B, Cin, Cout = (16, 32), 2, 32, 64
    x6, _, p, p_off, _ = fused_layer(ops, dev, hw, B, Cin, Cout, "sigma6")
    xbuf = x6.to(dev).clone()
    out = torch.empty(B, *hw, Cout, device=dev)
    g = _capture(lambda: ops.dcnv2_offset(xbuf, p_off, p, out=out, act=ops.ACT_NONE))
    gen = torch.Generator().manual_seed(77)
    for x in (x6, x6 * 0.01, torch.randn(B, *hw, Cin, generator=gen), x6):
        xbuf.copy_(x)
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        y = ops.dcnv2_offset(xbuf, p_off, p, act=ops.ACT_NONE)
        assert torch.equal(out, y)
        om = ops.conv2d(xbuf, p_off, out_dtype=torch.float32)
        assert torch.equal(out, ops.dcnv2(xbuf, om, p, act=ops.ACT_NONE))    # 16x32: the pair kernel serves the two-launch path
    assert math.isfinite(out.abs().max().item())
