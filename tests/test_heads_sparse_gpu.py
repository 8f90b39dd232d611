"""Sparse f16x3 heads (ctdet_head_sparse_x3_fwd, head_sparse_x3_kernel): the wh / reg heads at the decoded peaks only.
Against an f64 composition of 3x3 + bias + ReLU + 1x1 + bias and against the dense fused kernel gathered at the same pixels;
the box expressions against ops.decode with maps; the map-free decode; and the eval engine with and without the sparse step.

Bound: the one the dense path meets in test_model_gpu.py::test_heads_match_oracle[f16x3], 2e-4 * max(1, max |ref|), for
both kernels against f64; sparse against dense then differs by at most the sum of the two measured distances -- and, since
the kernel accumulates in the dense kernel's order for the pixel, not at all."""
import pytest
import torch

from test_heads_fused_x3_gpu import make_heads, nchw, nhwc, ref64

pytestmark = pytest.mark.gpu

DR = 4.0


@pytest.fixture(scope="module")
def ops():
    import detectron2_centernet_amd.ops as ops

    return ops


def pack2(ops, dev, heads):
    w1, b1, w2, b2 = heads
    return ops.PackedHeads([w.to(dev) for w in w1], [b.to(dev) for b in b1], [w.to(dev) for w in w2], [b.to(dev) for b in b2],
                           [ops.ACT_NONE, ops.ACT_NONE], compute=ops.F16X3)


def hand_inds(B, K, H, W, seed):
    """[B,K] int32: the four corners, a pixel on each edge, two interior pixels, one pixel three times, then random pixels"""
    special = [0, W - 1, (H - 1) * W, H * W - 1,                        # corners
               W // 2, (H - 1) * W + W // 3, (H // 2) * W, (H // 3) * W + W - 1,      # top, bottom, left, right edge
               (H // 2) * W + W // 2, 5 * W + 3,                         # interior
               7 * W + 9, 7 * W + 9, 7 * W + 9]                          # the same pixel under three "classes"
    assert B * K >= len(special)
    g = torch.Generator().manual_seed(seed)
    flat = torch.randint(0, H * W, (B * K,), generator=g, dtype=torch.int32)
    flat[:len(special)] = torch.tensor(special, dtype=torch.int32)
    flat = flat[torch.randperm(B * K, generator=g)]                      # every image gets some of them
    return flat.view(B, K).contiguous()


def gather(m_nhwc, inds):
    """m [B,H,W,C], inds [B,K] -> [B,K,C]"""
    B, H, W, Cc = m_nhwc.shape
    return torch.gather(m_nhwc.reshape(B, H * W, Cc), 1, inds.long()[..., None].expand(-1, -1, Cc))


def torch_boxes(whreg, inds, W, dr=DR):
    """dec_final_kernel's box expressions, one f32 operation each"""
    xs = (inds % W).float() + whreg[..., 2]
    ys = torch.div(inds, W, rounding_mode="floor").float() + whreg[..., 3]
    w, h = whreg[..., 0], whreg[..., 1]
    return torch.stack([(xs - w / 2) * dr, (ys - h / 2) * dr, (xs + w / 2) * dr, (ys + h / 2) * dr], -1)


def maps_and_refs(ops, dev, NB, H, W, seed):
    """(y NHWC on dev, heads, pack, dense kernel maps [NB,H,W,4] = (wh, reg), f64 maps [NB,H,W,4])"""
    heads = make_heads(64, (2, 2), seed=seed)
    x = torch.randn(NB, 64, H, W, generator=torch.Generator().manual_seed(seed + 1))
    y = nhwc(x).to(dev)
    ph = pack2(ops, dev, heads)
    d = ops.heads_fused(y, ph)
    dense = torch.cat([d[0][..., :2], d[1][..., :2]], -1)
    xd = x.to(dev)
    ref = torch.cat([nhwc(ref64(xd, heads, 0, False)), nhwc(ref64(xd, heads, 1, False))], -1)
    return y, ph, dense, ref


def check_whreg(got, dense_g, ref_g, what):
    """got / dense_g f32 [B,K,4], ref_g f64 [B,K,4]: per head, both within the dense path's bound of f64, and of each other
    within the sum of their distances"""
    for name, sl in (("wh", slice(0, 2)), ("reg", slice(2, 4))):
        r = ref_g[..., sl]
        tol = 2e-4 * max(1.0, r.abs().max().item())
        ds = (got[..., sl].double() - r).abs().max().item()
        dd = (dense_g[..., sl].double() - r).abs().max().item()
        sd = (got[..., sl].double() - dense_g[..., sl].double()).abs().max().item()
        print(f"{what} {name}: sparse-f64 {ds:.3e}  dense-f64 {dd:.3e}  sparse-dense {sd:.3e}  (bound {tol:.3e})")
        assert ds <= tol and dd <= tol, (what, name, ds, dd, tol)
        assert sd <= ds + dd, (what, name, sd, ds, dd)
    assert torch.equal(got, dense_g), what      # the dense kernel's products in the dense kernel's order


@pytest.mark.parametrize("case", [(2, 16, 32, 7), (2, 16, 32, 100), (2, 16, 16, 7), (2, 16, 16, 100)])
def test_sparse_heads_vs_dense_and_f64(ops, dev, case):
    """K = 7 / 100: no multiple of the 32-peak tile; B*K = 200: six full workgroups and a partial seventh"""
    B, H, W, K = case
    y, ph, dense, ref = maps_and_refs(ops, dev, B, H, W, seed=H + W + K)
    inds = hand_inds(B, K, H, W, seed=K).to(dev)
    whreg, boxes = ops.heads_sparse(y, ph, inds, DR)
    assert whreg.shape == (B, K, 4) and boxes.shape == (B, K, 4)
    check_whreg(whreg, gather(dense, inds), gather(ref, inds), f"{case}")
    # the same pixel gives the same numbers wherever it sits in a tile
    for ib, vb in zip(inds.cpu(), whreg.cpu()):
        first = {}
        for j in range(K):
            assert torch.equal(vb[j], vb[first.setdefault(int(ib[j]), j)])
    assert torch.equal(boxes, torch_boxes(whreg, inds, W))


def test_sparse_heads_full_size_grid(ops, dev):
    """B = 64, K = 100 on a 16x16 map: the grid of the headline step (6,400 peaks, 200 workgroups)"""
    B, H, W, K = 64, 16, 16, 100
    y, ph, dense, ref = maps_and_refs(ops, dev, B, H, W, seed=3)
    inds = hand_inds(B, K, H, W, seed=5).to(dev)
    whreg, boxes = ops.heads_sparse(y, ph, inds, DR)
    check_whreg(whreg, gather(dense, inds), gather(ref, inds), "64x100")
    assert torch.equal(boxes, torch_boxes(whreg, inds, W))


def test_box_assembly_equals_decode_with_maps(ops, dev):
    """the decode's boxes are torch_boxes of the map values at its inds, bit for bit; the sparse kernel's boxes are torch_boxes of
    its own four numbers: the same expressions, so the same boxes whenever the four numbers agree"""
    from test_hip_ops import _rand_heat
    B, H, W, K = 2, 16, 32, 100
    y, ph, dense, _ = maps_and_refs(ops, dev, B, H, W, seed=21)
    heat = nhwc(_rand_heat(B, 8, H, W, seed=22)).to(dev)
    boxes_d, _, _, inds = ops.decode(heat, dense[..., :2], dense[..., 2:], K, DR)
    assert torch.equal(boxes_d, torch_boxes(gather(dense, inds), inds, W))
    whreg, boxes_s = ops.heads_sparse(y, ph, inds, DR)
    assert torch.equal(boxes_s, torch_boxes(whreg, inds, W))
    assert torch.allclose(boxes_s, boxes_d, atol=1e-4, rtol=1e-6)


def test_sparse_heads_flip(ops, dev):
    """2B = 4 images: wh = (wh[b, y, x] + wh[b + B, y, W-1-x]) * 0.5, reg = image b's; peaks at x = 0 and x = W - 1 included"""
    B, H, W, K = 2, 16, 32, 37
    y, ph, dense, ref = maps_and_refs(ops, dev, 2 * B, H, W, seed=31)
    inds = hand_inds(B, K, H, W, seed=32).to(dev)
    xs = inds % W
    assert bool((xs == 0).any()) and bool((xs == W - 1).any())
    minds = inds - xs + (W - 1 - xs)

    def merged(m):
        p, q = gather(m[:B], inds), gather(m[B:], minds)
        return torch.cat([(p[..., :2] + q[..., :2]) * 0.5, p[..., 2:]], -1)

    whreg, boxes = ops.heads_sparse(y, ph, inds, DR, flip=True)
    check_whreg(whreg, merged(dense), merged(ref), "flip")
    assert torch.equal(boxes, torch_boxes(whreg, inds, W))
    # ... and the plain kernel on the plain half gives the plain half's reg, bit for bit
    plain, _ = ops.heads_sparse(y[:B], ph, inds, DR)
    assert torch.equal(plain[..., 2:], whreg[..., 2:])


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("shape", [(2, 80, 32, 48), (2, 4, 16, 16), (1, 8, 128, 128)])
def test_map_free_decode(ops, dev, shape, flip):
    """wh = reg = None: scores, classes and inds as with maps"""
    from test_hip_ops import _rand_heat
    B, Cc, H, W = shape
    NB = 2 * B if flip else B
    heat = nhwc(_rand_heat(NB, Cc, H, W, seed=sum(shape))).to(dev)
    g = torch.Generator().manual_seed(2)
    whreg = torch.rand(NB, H, W, 4, generator=g).to(dev)
    K = 100
    _, s0, c0, i0 = ops.decode(heat, whreg[..., :2], whreg[..., 2:], K, DR, heat_floor=ops.SIGMOID_CLAMP_FLOOR, flip=flip)
    _, s1, c1, i1 = ops.decode(heat, None, None, K, DR, heat_floor=ops.SIGMOID_CLAMP_FLOOR, flip=flip, check_status=True)
    assert torch.equal(s0, s1) and torch.equal(c0, c1) and torch.equal(i0, i1)


def test_sparse_heads_reject_bad_arguments(ops, dev):
    heads3 = make_heads(64, (80, 2, 2), seed=1)
    w1, b1, w2, b2 = heads3
    ph3 = ops.PackedHeads([w.to(dev) for w in w1], [b.to(dev) for b in b1], [w.to(dev) for w in w2], [b.to(dev) for b in b2],
                          [ops.ACT_NONE] * 3, compute=ops.F16X3)
    y = torch.zeros(1, 16, 16, 64, device=dev)
    inds = torch.zeros(1, 4, dtype=torch.int32, device=dev)
    with pytest.raises(AssertionError):
        ops.heads_sparse(y, ph3, inds, DR)
    # the map-free decode needs somewhere to leave the peaks
    lib = ops._lib.lib()
    heat = torch.rand(1, 16, 16, 4, device=dev)
    ws = ops.DecodeWorkspace(1, 16, 16, 4, 4, dev)
    sc, cl = torch.empty(1, 4, device=dev), torch.empty(1, 4, dtype=torch.int32, device=dev)
    rc = lib.ctdet_decode(ops._ptr(heat), 4, None, 0, None, 0, 1, 16, 16, 4, 4, DR, 0.0, ops._ptr(ws.buf), None, ops._ptr(sc),
                          ops._ptr(cl), None, None)
    assert rc != 0 and b"inds required" in lib.ctdet_last_error()


# ------------------------------------------------------------------------------------------ the eval engine
def _engine_model(tmp_path, seed=3):
    from test_model_gpu import make_model
    model, cfg = make_model(tmp_path, "f16x3", seed=seed)
    model.score_threshold = 0.0
    model.wh[2].bias.data.fill_(3.0)      # boxes of non-degenerate size
    return model


def _imgs(dev, seed=7):
    from test_model_gpu import images
    return images(2, 64, 128, seed=seed).to(dev)       # map 16 x 32


def _step(model, imgs, flip):
    """one first call and one replay; (engine, cloned dec of the first call, cloned dec of the replay)"""
    model._engines = {}
    model.infer_batch_tensor(imgs, flip=flip)
    eng = list(model._engines.values())[-1]
    first = [t.clone() for t in eng.dec]
    model.infer_batch_tensor(imgs, flip=flip)
    return eng, first, [t.clone() for t in eng.dec]


@pytest.mark.parametrize("flip", [False, True])
def test_engine_sparse_equals_dense(tmp_path, dev, ops, monkeypatch, flip):
    model = _engine_model(tmp_path)
    imgs = _imgs(dev)
    eng, first, second = _step(model, imgs, flip)
    assert eng.sparse and eng.graph is not None
    assert eng.graph_nodes.get("kernel", 0) > 0 and set(eng.graph_nodes) <= {"kernel", "empty"}, eng.graph_nodes
    for a, b in zip(first, second):                     # the replay is bit-equal to the first call
        assert torch.equal(a, b)
    out = eng.out
    assert eng.out is out and all(x is y for x, y in zip(eng.out, out))      # cached: the same tensors
    sparse_out = [t.clone() for t in out]
    monkeypatch.setattr(ops, "HEADS_SPARSE", False)
    deng, dfirst, _ = _step(model, imgs, flip)
    assert not deng.sparse
    assert torch.equal(first[1], dfirst[1]) and torch.equal(first[2], dfirst[2]) and torch.equal(first[3], dfirst[3])
    print("engine", "flip" if flip else "plain", "max box difference", (first[0] - dfirst[0]).abs().max().item())
    assert torch.allclose(first[0], dfirst[0], atol=1e-4, rtol=1e-6)
    for i in range(3):                                  # hm is the step's own; wh / reg come from the dense kernel on demand
        assert torch.equal(sparse_out[i], deng.out[i]), i
    # a later step drops the cached maps
    monkeypatch.setattr(ops, "HEADS_SPARSE", True)
    eng2, _, _ = _step(model, _imgs(dev, seed=8), flip)
    o1 = eng2.out[1]
    model.infer_batch_tensor(imgs, flip=flip)
    assert eng2.out[1] is not o1 and torch.equal(eng2.out[1], sparse_out[1])


def test_engine_sparse_reports_non_finite(tmp_path, dev, ops):
    """the finite flag of a sparse step covers the peaks' wh / reg and the heads' input map"""
    imgs = _imgs(dev)
    model = _engine_model(tmp_path, seed=2)
    assert len(model.infer_batch_tensor(imgs)) == 2
    with torch.no_grad():
        model.wh[2].weight[0, 0, 0, 0] = float("inf")
    model._engines = {}
    with pytest.raises(FloatingPointError, match="not finite"):
        model.infer_batch_tensor(imgs)
    assert list(model._engines.values())[-1].sparse

    # a blow-up away from every peak.  Peaks: a heat map that sits on the clamp floor everywhere (zero hm weights, bias
    # -100; NaN logits clamp to the floor too) decodes to class 0, pixels 0..99: rows 0..3 of the 16 x 32 map.  Blow-up: the
    # last backbone layer (DCNv2 with zero offsets, mask 0.5, + BatchNorm + ReLU) gets an output channel 0 that is
    # 3e38 * (4 * sum(above) - 4000 * sum(below)) / 2 over its non-negative input: +inf in the bottom row, where `below` is
    # the zero padding, and relu(-inf) = 0 everywhere else
    model = _engine_model(tmp_path, seed=2)
    with torch.no_grad():
        model.hm[2].weight.zero_()
        model.hm[2].bias.fill_(-100.0)
        node = model.backbone.ida_up.node_2
        node.conv.conv_offset_mask.weight.zero_()
        node.conv.conv_offset_mask.bias.zero_()
        node.conv.weight[0].zero_()
        node.conv.weight[0, :, 0, 1] = 4.0
        node.conv.weight[0, :, 2, 1] = -4000.0
        node.conv.bias[0] = 0.0
        bn = node.actf[0]
        bn.running_mean[0], bn.running_var[0], bn.weight[0], bn.bias[0] = 0.0, 1.0, 3e38, 0.0
    with pytest.raises(FloatingPointError, match="not finite"):
        model.infer_batch_tensor(imgs)
    eng = list(model._engines.values())[-1]
    assert eng.sparse
    y0 = eng._y[..., 0]
    assert bool(torch.isinf(y0[:, 15]).all()) and bool(torch.isfinite(eng._y[:, :15]).all())     # the bottom row alone
    assert int(eng.dec[3].max()) < 100                                # every peak in rows 0..3
    assert bool(torch.isfinite(eng.whreg).all()) and bool(torch.isfinite(eng.dec[0]).all())       # the peaks saw nothing
