"""The finite test of the heads' input map folded into the kernel that writes it: ops.dcnv2_offset(..., finite_flag=flag) in
F16X3 (dcn_split_window_kernel<2, 64, ..., fused, finite>).  The reference for the flag is always the scan of the STORED
output, ops.finite_flag(y) (finite_flag_kernel), never the folded code; y itself must equal the call without a flag bit for bit.

Shapes: Cin 32 / 64 (one / two chunk pairs of the offset phase), Cout 64 (the batched epilogue) / 40 (the per-pixel epilogue,
24 padded couts whose packed weight rows are filled with NaN here: they reach the accumulators and must reach neither the
tensor nor the flag), maps 8x16 (one tile) / 16x32 (four tiles), batch 1 / 2."""
import pytest
import torch

from test_dcn_offset_fused_x3_gpu import make_layer

pytestmark = pytest.mark.gpu

CINS, COUTS, MAPS, BATCHES = [32, 64], [64, 40], [(8, 16), (16, 32)], [1, 2]
# one cout in each of the four 16-cout accumulator tiles of a lane (cout_of<4>: tile c holds couts 32 (c / 2) + 8 q + 4 (c % 2) + i),
# all below 40
TILE_COUTS = [1, 13, 34, 38]


@pytest.fixture(scope="module")
def ops():
    import detectron2_centernet_amd.ops as ops

    return ops


def poison_padded_couts(p):
    """NaN into the packed weight rows behind Cout: the accumulators of the padded couts then hold NaN"""
    assert p.w.shape[0] == p.Cout_pad == 64
    if p.Cout_eff < p.Cout_pad:
        p.w[p.Cout_eff:].fill_(float("nan"))


def random_layer(ops, dev, Cin, Cout, seed):
    _, p, p_off = make_layer(ops, dev, Cin, Cout, 0.5, seed)
    poison_padded_couts(p)
    return p, p_off


def planted_layer(ops, dev, Cin, Cout, c, s, seed):
    """make_layer's DCN with zero offsets and mask logits (every sample on its pixel, mask 0.5) and cout c = 0.5 * x[..., 0] * s
    (centre tap, channel 0, BatchNorm scale s, bias 0): with |x| <= 1 and |s| = 3e38 every |value| is <= 1.5e38, and a planted
    x[..., 0] = 4 gives 2 * s = +-inf in the epilogue's multiplication -- the MFMA sums themselves stay finite"""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    scale = torch.rand(Cout, generator=g) + 0.5
    bias = torch.randn(Cout, generator=g) * 0.3
    w[c].zero_()
    w[c, 0, 1, 1] = 1.0
    scale[c], bias[c] = s, 0.0
    p = ops.PackedConv(w.to(dev), scale.to(dev), bias.to(dev), stride=1, pad=1, compute=ops.F16X3)
    p_off = ops.PackedConv(torch.zeros(27, Cin, 3, 3, device=dev), None, torch.zeros(27, device=dev), stride=1, pad=1, compute=ops.F16X3)
    poison_padded_couts(p)
    return p, p_off


def bounded_x(B, H, W, Cin, seed):
    return torch.randn(B, H, W, Cin, generator=torch.Generator().manual_seed(seed)).clamp_(-1.0, 1.0)


def both(ops, x, p_off, p, act):
    """(y of the call with a flag, the flag, y of the call without, the scan of that y)"""
    assert ops.dcnv2_offset_supported(x, p_off, p)
    flag = torch.ones(1, dtype=torch.int32, device=x.device)
    y = ops.dcnv2_offset(x, p_off, p, act=act, finite_flag=flag)
    y0 = ops.dcnv2_offset(x, p_off, p, act=act)
    assert y.shape == y0.shape == (*x.shape[:3], p.Cout_eff)
    return y, int(flag), y0, int(ops.finite_flag(y0))


def same(y, y0):
    """bit equality that also holds where both hold NaN"""
    return torch.equal(y.view(torch.int32), y0.view(torch.int32))


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("hw", MAPS)
@pytest.mark.parametrize("Cout", COUTS)
@pytest.mark.parametrize("Cin", CINS)
def test_finite_everywhere(ops, dev, Cin, Cout, hw, B):
    H, W = hw
    p, p_off = random_layer(ops, dev, Cin, Cout, seed=Cin + Cout + H)
    x = torch.randn(B, H, W, Cin, generator=torch.Generator().manual_seed(B + W)).to(dev)
    for act in (ops.ACT_RELU, ops.ACT_NONE):
        y, flag, y0, scan = both(ops, x, p_off, p, act)
        assert bool(torch.isfinite(y0).all()) and scan == 1
        assert flag == 1 and torch.equal(y, y0)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("hw", MAPS)
@pytest.mark.parametrize("Cout", COUTS)
@pytest.mark.parametrize("Cin", CINS)
def test_inf_from_the_epilogue(ops, dev, Cin, Cout, hw, B):
    """+inf that arises only in the epilogue's scale, once per call: each of the four cout tiles; the first and the last pixel of
    a tile; the first and the last pixel of the last tile of the last image.  -inf: ReLU stores 0 and the flag stays 1."""
    H, W = hw
    places = [(TILE_COUTS[0], 0, 0, 0), (TILE_COUTS[1], 0, 7, 15),
              (TILE_COUTS[2], B - 1, H - 8, W - 16), (TILE_COUTS[3], B - 1, H - 1, W - 1)]
    x0 = bounded_x(B, H, W, Cin, seed=Cin + H + B)
    for c, b, py, px in places:
        p, p_off = planted_layer(ops, dev, Cin, Cout, c, 3e38, seed=c)
        y, flag, y0, scan = both(ops, x0.to(dev), p_off, p, ops.ACT_RELU)          # nothing planted
        assert scan == 1 and flag == 1 and torch.equal(y, y0)
        x = x0.clone()
        x[b, py, px, 0] = 4.0
        for act in (ops.ACT_RELU, ops.ACT_NONE):
            y, flag, y0, scan = both(ops, x.to(dev), p_off, p, act)
            bad = (~torch.isfinite(y0)).nonzero().tolist()
            assert bad == [[b, py, px, c]] and y0[b, py, px, c].item() == float("inf"), (bad, (b, py, px, c))
            assert scan == 0 and flag == 0 and same(y, y0), (c, b, py, px, act)
        # the same place with -inf
        p, p_off = planted_layer(ops, dev, Cin, Cout, c, -3e38, seed=c)
        y, flag, y0, scan = both(ops, x.to(dev), p_off, p, ops.ACT_RELU)
        assert y0[b, py, px, c].item() == 0.0 and bool(torch.isfinite(y0).all())
        assert scan == 1 and flag == 1 and torch.equal(y, y0)
        y, flag, y0, scan = both(ops, x.to(dev), p_off, p, ops.ACT_NONE)
        assert y0[b, py, px, c].item() == float("-inf")
        assert scan == 0 and flag == 0 and same(y, y0)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("hw", MAPS)
@pytest.mark.parametrize("Cout", COUTS)
@pytest.mark.parametrize("Cin", CINS)
def test_nan_in_the_input(ops, dev, Cin, Cout, hw, B):
    H, W = hw
    p, p_off = random_layer(ops, dev, Cin, Cout, seed=Cin + Cout + W)
    x = torch.randn(B, H, W, Cin, generator=torch.Generator().manual_seed(B + H))
    x[B - 1, H // 2, W // 2] = float("nan")
    x = x.to(dev)
    y, flag, y0, scan = both(ops, x, p_off, p, ops.ACT_NONE)
    assert bool(torch.isnan(y0).any()), "no NaN reached the output: the case is not exercised"
    assert scan == 0 and flag == 0 and same(y, y0)
    y, flag, y0, scan = both(ops, x, p_off, p, ops.ACT_RELU)           # whatever is stored decides
    print(f"{Cin}->{Cout} {H}x{W} B={B} NaN input, ReLU: {int((~torch.isfinite(y0)).sum())} non-finite values stored, scan {scan}, flag {flag}")
    assert flag == scan and same(y, y0)


def test_replay_resets_the_flag(ops, dev):
    """[flag = 1; dcnv2_offset(x, flag)] captured once; replayed on an x holding inf, then on a finite x in the same buffer"""
    p, p_off = random_layer(ops, dev, 64, 64, seed=5)
    good = torch.randn(2, 16, 32, 64, generator=torch.Generator().manual_seed(6)).to(dev)
    bad = good.clone()
    bad[1, 9, 17] = float("inf")
    x = good.clone()
    out = torch.empty(2, 16, 32, 64, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.dcnv2_offset(x, p_off, p, out=out, act=ops.ACT_NONE, finite_flag=flag)     # warm-up outside the capture (packs the pair image)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            flag.fill_(1)
            ops.dcnv2_offset(x, p_off, p, out=out, act=ops.ACT_NONE, finite_flag=flag)
    torch.cuda.current_stream().wait_stream(s)
    for src, want in ((bad, 0), (good, 1), (bad, 0), (good, 1)):
        x.copy_(src)
        g.replay()
        torch.cuda.synchronize()
        assert int(ops.finite_flag(out)) == want          # the scan of what the replay stored
        assert int(flag) == want
        assert same(out, ops.dcnv2_offset(src, p_off, p, act=ops.ACT_NONE))


def _engine_step(model, imgs):
    model._engines = {}
    model.infer_batch_tensor(imgs)
    model.infer_batch_tensor(imgs)          # a replay
    eng = list(model._engines.values())[-1]
    assert eng.sparse and eng.graph is not None
    return eng, [t.clone() for t in eng.dec[:3]] + [t.clone() for t in eng._post()]


def test_engine_with_and_without_the_fold(tmp_path, dev, ops, monkeypatch):
    from test_model_gpu import images, make_model

    model, _ = make_model(tmp_path, "f16x3", seed=3)
    model.score_threshold = 0.0
    model.wh[2].bias.data.fill_(3.0)      # boxes of non-degenerate size
    imgs = images(2, 64, 128, seed=7).to(dev)
    monkeypatch.setattr(ops, "FINITE_FOLD", False)
    eng0, res0 = _engine_step(model, imgs)
    monkeypatch.setattr(ops, "FINITE_FOLD", True)
    eng1, res1 = _engine_step(model, imgs)
    assert len(res0) == len(res1) == 7               # dec: boxes, scores, classes; _post: boxes, scores, classes, counts
    for a, b in zip(res0, res1):
        assert torch.equal(a, b)
    assert int(res1[-1].min()) >= 0 and bool(eng0.finite) and bool(eng1.finite)
    for eng in (eng0, eng1):
        assert set(eng.graph_nodes) <= {"kernel", "empty"}, eng.graph_nodes
    assert eng1.graph_nodes["kernel"] == eng0.graph_nodes["kernel"] - 1, (eng0.graph_nodes, eng1.graph_nodes)
    # where y's producer is not the fused kernel, the scan of y stays
    monkeypatch.setattr(ops, "DCN_X3_FUSED", False)
    eng2, res2 = _engine_step(model, imgs)
    monkeypatch.setattr(ops, "FINITE_FOLD", False)
    eng3, res3 = _engine_step(model, imgs)
    # the same launches either way (the flag made before the backbone is the one the scans go on with), the offset convs on top
    assert eng2.graph_nodes["kernel"] == eng3.graph_nodes["kernel"] > eng0.graph_nodes["kernel"], (eng2.graph_nodes, eng3.graph_nodes)
    for a, b in zip(res2, res3):
        assert torch.equal(a, b)
