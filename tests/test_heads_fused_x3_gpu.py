"""f16x3 fused CenterNet heads (ctdet_head_fused_x3_fwd, head_fused_x3_kernel): against an f64 composition of
3x3 + bias + ReLU + 1x1 + bias (+ sigmoid / clamp), against the unfused f16x3 path, and bit-exact across replays and batch
sizes."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CLAMP = (1e-4, 1 - 1e-4)


@pytest.fixture(scope="module")
def ops():
    import detectron2_centernet_amd.ops as ops

    return ops


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def make_heads(Cin, couts, seed, hid_scale=1.0):
    g = torch.Generator().manual_seed(seed)
    w1 = [torch.randn(256, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5 * hid_scale for _ in couts]
    b1 = [torch.randn(256, generator=g) * 0.3 * hid_scale for _ in couts]
    w2 = [torch.randn(c, 256, 1, 1, generator=g) / 16 for c in couts]
    b2 = [torch.randn(c, generator=g) for c in couts]
    return w1, b1, w2, b2


def pack(ops, dev, heads, couts):
    w1, b1, w2, b2 = heads
    acts = [ops.ACT_SIGMOID_CLAMP if i == 0 else ops.ACT_NONE for i in range(len(couts))]
    return ops.PackedHeads([w.to(dev) for w in w1], [b.to(dev) for b in b1], [w.to(dev) for w in w2],
                           [b.to(dev) for b in b2], acts, compute=ops.F16X3)


def ref64(x_nchw, heads, i, first):
    """f64 composition for head i on NCHW x (any device)"""
    w1, b1, w2, b2 = heads
    dev = x_nchw.device
    hid = F.conv2d(x_nchw.double(), w1[i].double().to(dev), b1[i].double().to(dev), 1, 1).relu()
    y = F.conv2d(hid, w2[i].double().to(dev), b2[i].double().to(dev))
    if first:
        y = torch.clamp(torch.sigmoid(y), *CLAMP)
    return y


def check(got_nhwc, ref_nchw, what):
    c = ref_nchw.shape[1]
    got = nchw(got_nhwc[..., :c]).double()
    assert got.shape == ref_nchw.shape
    tol = 1e-5 * max(1.0, ref_nchw.abs().max().item())
    d = (got - ref_nchw.to(got.device)).abs().max().item()
    assert d <= tol, f"{what}: max |err| {d:.3e} > {tol:.3e}"


CASES = [
    # B, H, W, Cin, couts                  (8x32 tiles when W % 32 == 0, else 16x16)
    (2, 16, 32, 64, (80, 2, 2)),
    (1, 16, 16, 32, (1,)),
    (1, 8, 64, 32, (3, 92, 2, 1)),
    (2, 32, 48, 64, (92, 3)),
    (3, 24, 32, 32, (80, 2)),
]


@pytest.mark.parametrize("case", CASES)
def test_heads_fused_x3_vs_f64(ops, dev, case):
    B, H, W, Cin, couts = case
    heads = make_heads(Cin, couts, seed=Cin + 7 * len(couts) + H)
    x = torch.randn(B, Cin, H, W, generator=torch.Generator().manual_seed(H * W + Cin))
    ph = pack(ops, dev, heads, couts)
    outs = ops.heads_fused(nhwc(x).to(dev), ph, clamp=CLAMP)
    for i, c in enumerate(couts):
        assert outs[i].shape == (B, H, W, ops.round_up(c, 4)) and outs[i].dtype == torch.float32
        check(outs[i].cpu(), ref64(x, heads, i, i == 0), f"head {i} (cout {c})")


def test_heads_fused_x3_small_hidden(ops, dev):
    """hidden values around 1e-6: their lo halves are f16 subnormals"""
    couts = (80, 2, 2)
    heads = make_heads(64, couts, seed=3, hid_scale=1e-6)
    x = torch.randn(2, 64, 16, 32, generator=torch.Generator().manual_seed(4))
    ph = pack(ops, dev, heads, couts)
    outs = ops.heads_fused(nhwc(x).to(dev), ph, clamp=CLAMP)
    for i in range(len(couts)):
        check(outs[i].cpu(), ref64(x, heads, i, i == 0), f"head {i}")
    # the hidden magnitudes really are tiny: the output is b2 (+ sigmoid) to within 1e-4
    assert (nchw(outs[1][..., :2].cpu()) - heads[3][1].view(1, 2, 1, 1)).abs().max() < 1e-4


def unfused(ops, dev, heads, couts, x_nhwc):
    """the layer-by-layer f16x3 path of CenterNet._head_outputs: one 3x3 over the concatenated first convs, then a 1x1 per head"""
    w1, b1, w2, b2 = heads
    p = ops.PackedConv(torch.cat(w1, 0).to(dev).contiguous(), None, torch.cat(b1).to(dev), stride=1, pad=1, compute=ops.F16X3)
    hid = ops.conv2d(x_nhwc, p, act=ops.ACT_RELU)
    outs = []
    for i, c in enumerate(couts):
        pf = ops.PackedConv(w2[i].to(dev).contiguous(), None, b2[i].to(dev), compute=ops.F16X3)
        act = ops.ACT_SIGMOID_CLAMP if i == 0 else ops.ACT_NONE
        outs.append(ops.conv2d(hid[..., 256 * i:256 * (i + 1)], pf, act=act, out_dtype=torch.float32, clamp=CLAMP))
    return outs


@pytest.mark.parametrize("case", [CASES[0], CASES[3]])
def test_heads_fused_x3_vs_unfused(ops, dev, case):
    B, H, W, Cin, couts = case
    heads = make_heads(Cin, couts, seed=11)
    x = nhwc(torch.randn(B, Cin, H, W, generator=torch.Generator().manual_seed(12))).to(dev)
    got = ops.heads_fused(x, pack(ops, dev, heads, couts), clamp=CLAMP)
    want = unfused(ops, dev, heads, couts, x)
    for i, c in enumerate(couts):
        tol = 1e-5 * max(1.0, want[i][..., :c].abs().max().item())
        assert (got[i][..., :c] - want[i][..., :c]).abs().max().item() <= tol


def test_heads_fused_x3_graph_replays_bit_exact(ops, dev):
    couts = (80, 2, 2)
    heads = make_heads(64, couts, seed=5)
    x = nhwc(torch.randn(4, 64, 32, 64, generator=torch.Generator().manual_seed(6))).to(dev)
    ph = pack(ops, dev, heads, couts)
    outs = [torch.empty(4, 32, 64, ops.round_up(c, 4), device=dev) for c in couts]
    ops.heads_fused(x, ph, clamp=CLAMP, outs=outs)        # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            ops.heads_fused(x, ph, clamp=CLAMP, outs=outs)
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    first = [o.clone() for o in outs]
    for o in outs:
        o.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(first, outs):
        assert torch.equal(a, b)
    eager = ops.heads_fused(x, ph, clamp=CLAMP)
    for a, b in zip(first, eager):
        assert torch.equal(a, b)


def test_heads_fused_x3_fullsize(ops, dev):
    """the bench shape (64 x 128^2, Cin 64, hm / wh / reg): a few images against f64, all against the unfused path, and
    images 0..3 bit-identical in a batch of 4"""
    couts = (80, 2, 2)
    heads = make_heads(64, couts, seed=9)
    g = torch.Generator(device=dev).manual_seed(10)
    x = torch.randn(64, 128, 128, 64, generator=g, device=dev)
    ph = pack(ops, dev, heads, couts)
    got = ops.heads_fused(x, ph, clamp=CLAMP)
    for b in (0, 37, 63):
        xb = nchw(x[b:b + 1])
        for i in range(len(couts)):
            check(got[i][b:b + 1], ref64(xb, heads, i, i == 0), f"image {b} head {i}")
    want = unfused(ops, dev, heads, couts, x)
    for i, c in enumerate(couts):
        tol = 1e-5 * max(1.0, want[i][..., :c].abs().max().item())
        assert (got[i][..., :c] - want[i][..., :c]).abs().max().item() <= tol
    del want
    small = ops.heads_fused(x[:4].contiguous(), ph, clamp=CLAMP)
    for a, b in zip(got, small):
        assert torch.equal(a[:4], b)
    again = ops.heads_fused(x, ph, clamp=CLAMP)
    for a, b in zip(got, again):
        assert torch.equal(a, b)


def test_heads_fused_x3_rejects_bad_shapes(ops, dev):
    heads = make_heads(32, (2,), seed=1)
    ph = pack(ops, dev, heads, (2,))
    assert not ops.heads_fused_ok(torch.zeros(1, 8, 48, 32, device=dev), ops.F16X3)     # 8x48: neither tile form
    with pytest.raises(RuntimeError, match="8x32 or 16x16"):
        ops.heads_fused(torch.zeros(1, 8, 48, 32, device=dev), ph)
