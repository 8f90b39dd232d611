"""Flip test-time augmentation on the GPU.

  * the flip-merge decode against the plain decode of maps merged beforehand with torch, bit for bit;
  * the three kernels that produce the mirrored network input (preprocess, fused DLA base f16 and f16x3) against their plain
    forms fed a host-mirrored, left-padded image;
  * the flip engine end to end against the CPU oracle's flip test (oracle/model_ref.py forwards on x and x.flip(3), merged
    here), DLA-34 in the three precisions, one ResNet and one VoVNet config;
  * the wrapper, the export split and the plain path next to a flip engine.

Tolerances: everything that is a re-arrangement of the same f32 operations is compared with torch.equal.  The merged heat
map against the oracle carries HM_TOL of tests/test_model_gpu.py for the mode: a mean of two maps that each lie within the
bound lies within it."""
import numpy as np
import pytest
import torch

from oracle import ctdet_oracle as O
from oracle import model_ref as MR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    import detectron2_centernet_amd.ops as ops

    return ops


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2)


# ---------------------------------------------------------------------------------------------- decode
def _heat(kind, B2, H, W, C, floor, g):
    """[2B,H,W,C] f32 heat maps in the clamp range: `spread` sigmoid of wide logits (almost every value distinct), `plateau`
    a trained network's map, most of it exactly on the clamp floor (ties that the index rule has to order, also after the
    merge: floor + floor stays the floor) with scattered values above it"""
    if kind == "spread":
        logits = torch.randn(B2, H, W, C, generator=g) * 2.5 - 2.0
    else:
        logits = torch.full((B2, H, W, C), -12.0)
        n = max(2, H * W * C // 60)
        idx = torch.randint(0, B2 * H * W * C, (n,), generator=g)
        logits.view(-1)[idx] = torch.randn(n, generator=g) * 3.0
    return torch.clamp(torch.sigmoid(logits), floor, 1 - 1e-4)


DECODE_CASES = [
    # C, H, W, B, heat pixel stride (0 = dense), kind
    (1, 9, 11, 2, 0, "spread"), (1, 56, 88, 1, 4, "plateau"), (1, 128, 128, 2, 0, "plateau"),
    (3, 9, 11, 3, 4, "plateau"), (3, 56, 88, 2, 0, "spread"), (3, 128, 128, 1, 8, "spread"),
    (80, 9, 11, 2, 0, "plateau"), (80, 56, 88, 2, 84, "spread"), (80, 128, 128, 2, 0, "plateau"),
    (80, 128, 128, 1, 0, "spread"), (80, 56, 88, 1, 0, "plateau"),
]


@pytest.mark.parametrize("floor_on", [False, True])
@pytest.mark.parametrize("case", DECODE_CASES)
def test_decode_flip_equals_decode_of_merged_maps(ops, dev, case, floor_on):
    """ops.decode(flip=True) on 2B images == ops.decode on (a + b.flip(2)) * 0.5 merged by torch: scores, classes, indices
    and boxes bit for bit; partial tiles, 1 / 3 / 80 classes, channel-slice views, with and without the floor promise, spread
    maps and maps that sit on the floor"""
    C, H, W, B, stride, kind = case
    floor = ops.SIGMOID_CLAMP_FLOOR if floor_on else 0.0
    g = torch.Generator().manual_seed(C * 1000 + H + W + B)
    K = 100
    heat = _heat(kind, 2 * B, H, W, C, ops.SIGMOID_CLAMP_FLOOR, g)
    if kind == "plateau":
        assert (heat == np.float32(1e-4)).float().mean() > 0.5
    whreg = torch.cat([torch.rand(2 * B, H, W, 2, generator=g) * 20, torch.rand(2 * B, H, W, 2, generator=g)], dim=3).to(dev)
    if stride:
        buf = torch.full((2 * B, H, W, stride), 0.5, device=dev)      # the channels behind the slice must not matter
        buf[..., :C] = heat.to(dev)
        hm = buf[..., :C]
    else:
        hm = heat.to(dev)
    wh, reg = whreg[..., 0:2], whreg[..., 2:4]
    # the merge as the issue states it: one f32 add, one multiply by 0.5
    hm_m = ((hm[:B] + hm[B:].flip(2)) * 0.5).contiguous()
    wh_m = ((wh[:B] + wh[B:].flip(2)) * 0.5).contiguous()
    reg_m = reg[:B].contiguous()
    assert hm_m.min().item() >= np.float32(1e-4)      # the mean respects the clamp floor
    ws = ops.DecodeWorkspace(B, H, W, C, K, dev)
    want = ops.decode(hm_m, wh_m, reg_m, K, 4.0, heat_floor=floor, check_status=True)
    got = ops.decode(hm, wh, reg, K, 4.0, workspace=ws, heat_floor=floor, flip=True)
    rc = ops._lib.lib().ctdet_decode_status(ws.buf.data_ptr(), B, H, W, C, K, None)
    assert rc == 0, ops._lib.lib().ctdet_last_error()
    for name, a, b in zip(("boxes", "scores", "classes", "inds"), got, want):
        assert a.shape == b.shape and a.shape[0] == B
        assert torch.equal(a, b), f"{name} differ: C={C} {H}x{W} B={B} stride={stride} {kind} floor={floor}"
    # and the oracle agrees on what is selected (it returns min(K, C*H*W) entries; those of score 0 -- a map with fewer than
    # K peaks -- are ties among non-peaks, whose order torch.topk leaves open)
    rb, rs, rcl, ri = O.ctdet_decode(nchw(hm_m.cpu()), nchw(wh_m.cpu()), nchw(reg_m.cpu()), down_ratio=4, K=K)
    n, pos = rs.shape[1], rs > 0
    assert pos.any() and torch.equal(got[1].cpu()[:, :n][pos], rs[pos])
    assert torch.equal(got[2].cpu()[:, :n][pos], rcl[pos]) and torch.equal(got[3].cpu().long()[:, :n][pos], ri[pos])


def test_decode_flip_without_reg_and_odd_width(ops, dev):
    """reg = None (boxes centred on the cell) and an odd width, where the middle column merges with itself"""
    g = torch.Generator().manual_seed(11)
    B, H, W, C = 2, 13, 17, 5
    hm = _heat("spread", 2 * B, H, W, C, 1e-4, g).to(dev)
    wh = (torch.rand(2 * B, H, W, 2, generator=g) * 9).to(dev)
    got = ops.decode(hm, wh, None, 40, 4.0, flip=True, check_status=True)
    want = ops.decode(((hm[:B] + hm[B:].flip(2)) * 0.5).contiguous(), ((wh[:B] + wh[B:].flip(2)) * 0.5).contiguous(), None, 40, 4.0)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- mirrored input
# means of the form k / 255: the byte k normalises to exactly 0, so an image padded on the LEFT with k is, for the plain
# kernels, the same network input as the mirrored padded tensor (whose padding is zero after normalisation)
PAD_BYTES = (104, 114, 120)
MEAN = [k / 255 for k in PAD_BYTES]
STD = [0.289, 0.274, 0.278]


def _host_mirrored(img, Wp):
    """[B,3,H,W] -> [B,3,H,Wp]: column x = column Wp-1-x of the image, the pad byte where that is >= W"""
    B, _, H, W = img.shape
    out = torch.empty(B, 3, H, Wp, dtype=img.dtype)
    for c in range(3):
        out[:, c] = PAD_BYTES[c]
    out[..., Wp - W:] = img.flip(3)
    return out


def test_pad_bytes_normalise_to_zero():
    for k, m in zip(PAD_BYTES, MEAN):
        assert np.float32(k) / np.float32(255.0) - np.float32(m) == 0.0


SIZES = [(2, 64, 64), (2, 33, 45), (1, 97, 131), (2, 160, 224), (1, 50, 96)]      # multiples of 32 and not; (97, 131) has
                                                                                  # interior windows on both halves


@pytest.mark.parametrize("dt", [torch.uint8, torch.float32])
@pytest.mark.parametrize("size", SIZES)
def test_preprocess_mirror(ops, dev, size, dt):
    B, H, W = size
    Hp, Wp = (H + 31) // 32 * 32, (W + 31) // 32 * 32
    g = torch.Generator().manual_seed(H * W)
    img = torch.randint(0, 256, (B, 3, H, W), generator=g).to(dt)
    mir = _host_mirrored(img, Wp).to(dev)
    img = img.to(dev)
    for odt, ch, border in ((torch.float16, 8, 0), (torch.float32, 8, 0), (torch.float32, 4, 0), (torch.float16, 8, 3),
                            (torch.float32, 4, 3), (torch.float32, 8, 1)):
        def buf(n):
            return torch.zeros(n, Hp + 2 * border, Wp + 2 * border, ch, dtype=odt, device=dev)
        plain = ops.preprocess(img, MEAN, STD, Hp, Wp, out=buf(B), border=border)
        got = ops.preprocess(img, MEAN, STD, Hp, Wp, out=buf(B), border=border, mirror=True)
        what = f"{size} {dt} -> {odt} x{ch} border {border}"
        assert torch.equal(got, plain.flip(2)), what                                     # the plain output, mirrored
        fed = ops.preprocess(mir, MEAN, STD, Hp, Wp, out=buf(B), border=border)           # plain kernel, host-mirrored image
        assert torch.equal(got, fed), what
        both = ops.preprocess(img, MEAN, STD, Hp, Wp, out=buf(2 * B), border=border, mirror="both")
        assert torch.equal(both[:B], plain) and torch.equal(both[B:], got), what
        if Wp > W and border == 0:
            assert not got[:, :, :Wp - W].any() and got[:, :H, Wp - W:, :3].any()      # zero padding on the left


def _base_operands(ops, dev, x3, g):
    ws = [torch.randn(16, 3, 7, 7, generator=g) / 147 ** 0.5, torch.randn(16, 16, 3, 3, generator=g) / 12,
          torch.randn(32, 16, 3, 3, generator=g) / 12]
    if not x3:
        ws = [w.half().float() for w in ws]
    sb = [(torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3) for c in (16, 16, 32)]
    args = []
    for w, (sc, bi) in zip(ws, sb):
        args += [w.to(dev), (sc.to(dev), bi.to(dev))]
    return (ops.PackedDlaBaseX3 if x3 else ops.PackedDlaBase)(*args)


@pytest.mark.parametrize("x3", [False, True])
@pytest.mark.parametrize("dt", [torch.uint8, torch.float32])
@pytest.mark.parametrize("size", SIZES)
def test_dla_base_mirror(ops, dev, size, dt, x3):
    """dla_base_fused_kernel / dla_base_x3_kernel, MIRROR forms: computed from the caller's images in place == the plain
    kernel on the host-mirrored, left-padded image (torch.equal: the same network input, the same arithmetic), main and
    pooled output; `both` = the plain half then the mirrored half"""
    B, H, W = size
    Hp, Wp = (H + 31) // 32 * 32, (W + 31) // 32 * 32
    g = torch.Generator().manual_seed(H * W + 7)
    pb = _base_operands(ops, dev, x3, g)
    img = torch.randint(0, 256, (B, 3, H, W), generator=g).to(dt)
    mir = _host_mirrored(img, Wp).to(dev)
    img = img.to(dev)
    odt = torch.float32 if x3 else torch.float16

    def pool(n):
        return torch.full((n, Hp // 4, Wp // 4, 32), -1.0, dtype=odt, device=dev)
    pw, pp, pg, pbo = pool(B), pool(B), pool(B), pool(2 * B)
    want = ops.dla_base_fused(mir, MEAN, STD, Hp, Wp, pb, pooled=pw)
    plain = ops.dla_base_fused(img, MEAN, STD, Hp, Wp, pb, pooled=pp)
    got = ops.dla_base_fused(img, MEAN, STD, Hp, Wp, pb, pooled=pg, mirror=True)
    assert got.shape == want.shape and torch.equal(got, want) and torch.equal(pg, pw)
    assert want.float().std().item() > 1e-2
    both = ops.dla_base_fused(img, MEAN, STD, Hp, Wp, pb, pooled=pbo, mirror="both")
    assert both.shape[0] == 2 * B
    assert torch.equal(both[:B], plain) and torch.equal(pbo[:B], pp)
    assert torch.equal(both[B:], got) and torch.equal(pbo[B:], pg)


# ---------------------------------------------------------------------------------------------- end to end
def _merge_cpu(eng_out, B):
    """the engine's 2B maps (NHWC, device) -> merged logical-NCHW CPU maps of B images"""
    hm, wh, reg = [nchw(t.float().cpu()) for t in eng_out]
    assert hm.shape[0] == 2 * B
    return (hm[:B] + hm[B:].flip(3)) * 0.5, (wh[:B] + wh[B:].flip(3)) * 0.5, reg[:B]


def _oracle_flip_hm(forward, sd, imgs, cfg, div):
    """CenterNet's flip test composed from oracle forwards on the network input x and on x.flip(3)"""
    x, _ = O.preprocess(imgs, cfg.MODEL.PIXEL_MEAN, cfg.MODEL.PIXEL_STD, div)
    with torch.no_grad():
        z1, z2 = forward(sd, x), forward(sd, x.flip(3))
    h1 = torch.clamp(torch.sigmoid(z1["hm"]), 1e-4, 1 - 1e-4)
    h2 = torch.clamp(torch.sigmoid(z2["hm"]), 1e-4, 1 - 1e-4)
    return (h1 + h2.flip(3)) * 0.5


def _check_flip_step(ops, model, cfg, sd, forward, imgs, maps, dec, tol, div, what):
    from test_model_gpu import MIN_HM_STD
    B = len(imgs)
    hm, wh, reg = _merge_cpu(maps, B)
    # decode of the engine's own maps, merged on the CPU, by the oracle: bit for bit
    rb, rs, rc, ri = O.ctdet_decode(hm, wh, reg, down_ratio=4, K=100)
    boxes, scores, classes, inds = [t.cpu() for t in dec]
    assert scores.shape[0] == B
    assert torch.equal(scores, rs) and torch.equal(classes, rc) and torch.equal(inds.long(), ri), what
    assert torch.allclose(boxes, rb, atol=1e-4, rtol=1e-6), what
    # ... and by the plain HIP decode of the maps merged with torch on the device: boxes too
    dhm, dwh, dreg = maps
    again = ops.decode(((dhm[:B] + dhm[B:].flip(2)) * 0.5).contiguous(), ((dwh[:B] + dwh[B:].flip(2)) * 0.5).contiguous(),
                       dreg[:B].contiguous(), 100, 4.0, heat_floor=ops.SIGMOID_CLAMP_FLOOR)
    for a, b in zip(dec, again):
        assert torch.equal(a, b), what
    # the merged heat map against the oracle's flip test
    hm_ref = _oracle_flip_hm(forward, sd, imgs, cfg, div)
    assert hm.shape == hm_ref.shape
    assert hm_ref.std().item() > MIN_HM_STD, "degenerate heat map: the comparison would be meaningless"
    err = (hm - hm_ref).abs().max().item()
    print(what, "merged heat map max err vs the oracle's flip test", err, "tol", tol)
    assert err <= tol, (what, err)


def _images(B, H, W, seed, kind="u8"):
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (B, 3, H, W), generator=g, dtype=torch.uint8)
    return img.float() if kind == "f32" else img


def _run_cases(ops, monkeypatch, dev, model, cfg, sd, forward, tol, div, cases, ragged, what):
    model.score_threshold = 0.0
    for B, H, W, kind in cases:
        img = _images(B, H, W, H + W, kind)
        out = model.infer_batch_tensor(img.to(dev), flip=True)
        assert len(out) == B and out[0]["instances"].image_size == (H, W)
        eng = list(model._engines.values())[-1]
        assert eng.flip and eng.key[-1] == "flip" and eng.img_params.shape[0] == B and eng.out[1].shape[0] == 2 * B
        assert eng.graph_nodes.get("kernel", 0) > 0 and set(eng.graph_nodes) <= {"kernel", "empty"}, eng.graph_nodes
        _check_flip_step(ops, model, cfg, sd, forward, [i for i in img], eng.out, eng.dec, tol, div, f"{what} {B}x{H}x{W} {kind}")
    # a ragged list batch: the eager path, per-image (mirrored) preprocess into the padded 2B batch
    seen = {}
    real = ops.decode

    def spy(hm, wh, reg, *a, **k):
        seen["maps"] = (hm, wh, reg)
        seen["dec"] = real(hm, wh, reg, *a, **k)
        seen["flip"] = k.get("flip", False)
        return seen["dec"]
    monkeypatch.setattr(ops, "decode", spy)
    imgs = [_images(1, h, w, h * w)[0] for h, w in ragged]
    out = model._forward_eval([{"image": im} for im in imgs], flip=True)
    monkeypatch.setattr(ops, "decode", real)
    assert seen["flip"] and len(out) == len(imgs)
    for o, (h, w) in zip(out, ragged):
        assert o["instances"].image_size == (h, w)
    _check_flip_step(ops, model, cfg, sd, forward, imgs, seen["maps"], seen["dec"], tol, div, f"{what} ragged {ragged}")


@pytest.mark.parametrize("precision", ["f32", "f16x3", "f16"])
def test_flip_engine_dla34_matches_oracle_flip_test(tmp_path, dev, ops, monkeypatch, precision):
    """DLA-34: sizes that are not multiples of 32 (the mirrored padding on the left, inside the fused base kernel where that
    runs), a multiple of 32, f32 images, a ragged list"""
    from test_model_gpu import HM_TOL, cpu_state_dict, make_model
    model, cfg = make_model(tmp_path, precision, seed=5)
    _run_cases(ops, monkeypatch, dev, model, cfg, cpu_state_dict(model), MR.centernet_forward, HM_TOL[precision], 32,
               [(2, 97, 131, "u8"), (1, 160, 96, "f32"), (3, 33, 33, "u8")], [(50, 70), (64, 96)], f"dla34 {precision}")


def test_flip_engine_resnet_matches_oracle_flip_test(tmp_path, dev, ops, monkeypatch):
    from test_model_gpu import HM_TOL
    from test_resnet_gpu import RES18_YAML, _make
    model, cfg, sd = _make(tmp_path, "f32", RES18_YAML)
    sdf = {k: v.float() for k, v in sd.items()}

    def forward(sd_, x):      # the ResNet-18 oracle forward of test_resnet18_centernet_eval_matches_oracle
        y = MR.deconv_layers(sd_, "deconv_layers", MR.resnet_features(sd_, "backbone", x, blocks=(2, 2, 2), bottleneck=False))
        return MR.centernet_heads(MR.Net(sd_), y)
    _run_cases(ops, monkeypatch, dev, model, cfg, sdf, forward, HM_TOL["f32"], 16,
               [(2, 90, 120, "u8"), (1, 96, 128, "f32")], [(40, 70), (64, 50)], "resnet18 f32")


def test_flip_engine_vovnet_matches_oracle_flip_test(tmp_path, dev, ops, monkeypatch):
    import os
    import sys
    from detectron2_centernet_amd.config import get_cfg
    from detectron2_centernet_amd.data.catalog import register_synthetic
    from detectron2_centernet_amd.modeling import build_model
    from test_model_gpu import HM_TOL
    from test_vovnet_gpu import BASE, VOV_YAML
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    from weights import fill_state_dict
    (tmp_path / "Base-CenterNet.yaml").write_text(BASE)
    (tmp_path / "ctdet_vovnet2_19_slim_1x.yaml").write_text(VOV_YAML)
    cfg = get_cfg()
    cfg.merge_from_file(str(tmp_path / "ctdet_vovnet2_19_slim_1x.yaml"))
    cfg.MODEL.CENTERNET.HIP_PRECISION = "f32"
    register_synthetic("bulb_train", num_classes=80)
    model = build_model(cfg).eval()
    sd = fill_state_dict({k: v.cpu() for k, v in model.state_dict().items()}, seed=31)
    model.load_state_dict({k: v.to(model.device) for k, v in sd.items()})
    sdf = {k: v.float() for k, v in sd.items()}
    _run_cases(ops, monkeypatch, dev, model, cfg, sdf, MR.centernet_vovnet_forward, HM_TOL["f32"], 16,
               [(2, 90, 120, "u8"), (1, 96, 128, "f32")], [(40, 70), (64, 50)], "vovnet19-slim f32")


# ---------------------------------------------------------------------------------------------- wrapper and neighbours
def _same(a, b, exact=True, score_tol=0.0):
    """exact: bit for bit.  Otherwise (the export split, whose host-side detector_postprocess and 8-channel input layout
    differ from the engine's kernels): same detections in the same order, boxes within 1e-3 px like the plain split's test,
    scores within score_tol"""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        ix, iy = x["instances"], y["instances"]
        assert ix.image_size == iy.image_size and len(ix) == len(iy)
        assert torch.equal(ix.pred_classes, iy.pred_classes)
        if exact:
            assert torch.equal(ix.scores, iy.scores) and torch.equal(ix.pred_boxes.tensor, iy.pred_boxes.tensor)
        else:
            ds = (ix.scores - iy.scores).abs().max().item()
            db = (ix.pred_boxes.tensor - iy.pred_boxes.tensor).abs().max().item()
            print("export split vs engine: max score diff", ds, "max box diff", db)
            assert ds <= score_tol and db <= 1e-3, (ds, db)


def _tta_cfg(cfg, min_sizes=(), flip=True):
    cfg = cfg.clone()
    cfg.TEST.AUG.ENABLED, cfg.TEST.AUG.MIN_SIZES, cfg.TEST.AUG.FLIP = True, tuple(min_sizes), flip
    return cfg


def test_wrapper_export_and_plain_path(tmp_path, dev):
    from detectron2_centernet_amd.evaluation.evaluator import inference_on_dataset
    from detectron2_centernet_amd.export import CenterNetModel
    from detectron2_centernet_amd.modeling import CenterNetWithTTA
    from test_model_gpu import make_model
    model, cfg = make_model(tmp_path, "f16", seed=4)
    model.score_threshold = 0.0
    model.wh[-1].bias.data.fill_(3.0)          # boxes of non-degenerate size
    img = _images(2, 80, 100, 9)
    batch = [{"image": img[0], "height": 160, "width": 200}, {"image": img[1]}]

    # the plain path with no flip engine alive
    plain0 = model(batch)
    assert len(model._engines) == 1
    # the flip engine: first call (eager warm-up + capture + replay), then replays
    first = model._forward_eval(batch, flip=True)
    assert len(model._engines) == 2                                  # the two engines of one shape live side by side
    keys = list(model._engines)
    assert keys[1] == keys[0] + ("flip",)
    eng = model._engines[keys[1]]
    assert eng.graph is not None and eng.graph_nodes.get("kernel", 0) > 0 and set(eng.graph_nodes) <= {"kernel", "empty"}
    assert len(first) == 2 and first[0]["instances"].image_size == (160, 200) and len(first[0]["instances"]) > 0
    _same(model._forward_eval(batch, flip=True), first)                # a graph replay gives what the first call gave
    _same(model.forward_async(batch, flip=True).result(), first)
    # the flip test changes the result (the comparison below would otherwise pass on a wrapper that ignores FLIP)
    assert not torch.equal(first[1]["instances"].scores, plain0[1]["instances"].scores)
    # plain and flip steps interleaved: the plain outputs stay what they were, bit for bit
    _same(model(batch), plain0)
    _same(model._forward_eval(batch, flip=True), first)
    _same(model(batch), plain0)
    assert len(model._engines) == 2

    # the wrapper == the engine; FLIP off == the plain path; one MIN_SIZES entry resizes first
    tta = CenterNetWithTTA(_tta_cfg(cfg), model)
    _same(tta(batch), first)
    _same(tta.forward_async(batch).result(), first)
    _same(CenterNetWithTTA(_tta_cfg(cfg, flip=False), model)(batch), plain0)
    _same(CenterNetWithTTA(_tta_cfg(cfg, min_sizes=(80,)), model)(batch), first)      # already at the test size
    small = [{"image": _images(1, 40, 50, 3)[0]}]
    res = CenterNetWithTTA(_tta_cfg(cfg, min_sizes=(80,)), model)(small)
    assert res[0]["instances"].image_size == (40, 50)                  # boxes back in the original frame
    up = CenterNetWithTTA(_tta_cfg(cfg, min_sizes=(80,)), model)._inputs(small)
    assert tuple(up[0]["image"].shape) == (3, 80, 100)
    _same(res, model._forward_eval(up, flip=True))
    # inference_on_dataset drives the wrapper like a model (eval mode, forward_async, one batch in flight)
    seen = []

    class _Ev:
        def reset(self):
            pass

        def process(self, inputs, outputs):
            seen.append(outputs)

        def evaluate(self):
            return {"n": len(seen)}
    assert inference_on_dataset(tta, [batch, batch, batch], _Ev()) == {"n": 3}
    for o in seen:
        _same(o, first)
    model.train()
    with pytest.raises(RuntimeError, match="inference-time"):
        tta(batch)
    model.eval()

    # the serving split with flip=True on a ragged batch (like the plain split's test: in the f16 mode the layer-by-layer base
    # of the split and the fused base kernel of the engine round differently, so same-size batches are compared in f32 below)
    ragged = [{"image": _images(1, 96, 128, 5)[0], "height": 192, "width": 256}, {"image": _images(1, 80, 100, 6)[0]}]
    em = CenterNetModel(cfg, model, flip=True)
    inputs = em.convert_inputs(ragged)
    assert tuple(inputs["images"].shape) == (4, 3, 96, 128) and inputs["im_info"].tolist() == [[96, 128], [80, 100]]
    res = em.inference(inputs)
    assert tuple(res["hm"].shape) == (4, 80, 24, 32)
    want = tta(ragged)
    assert len(want[0]["instances"]) > 0 and want[0]["instances"].image_size == (192, 256)
    _same(em.convert_outputs(ragged, inputs, res), want, exact=False)      # the same kernels on the same input: equal scores
    _same(em(ragged), want, exact=False)


def test_export_split_flip_equals_the_flip_engine(tmp_path, dev):
    """f32 mode (no fused base: the split and the engine run the same kernels): CenterNetModel(flip=True) == the captured flip
    engine on a same-size batch"""
    from detectron2_centernet_amd.export import CenterNetModel
    from detectron2_centernet_amd.modeling import CenterNetWithTTA
    from test_model_gpu import HM_TOL, make_model
    model, cfg = make_model(tmp_path, "f32", seed=4)
    model.score_threshold = 0.0
    model.wh[-1].bias.data.fill_(3.0)
    img = _images(2, 80, 100, 9)
    batch = [{"image": img[0], "height": 160, "width": 200}, {"image": img[1]}]
    want = CenterNetWithTTA(_tta_cfg(cfg), model)(batch)
    eng = list(model._engines.values())[-1]
    assert eng.flip and eng.graph is not None and len(want[0]["instances"]) > 0
    # the engine's stem reads 4-channel pixels, the split's 8-channel ones: another summation order.  Each is an f32-mode
    # evaluation, within HM_TOL["f32"] of the fp32 oracle, so within twice that of the other
    _same(CenterNetModel(cfg, model, flip=True)(batch), want, exact=False, score_tol=2 * HM_TOL["f32"])


def test_flip_engine_reports_non_finite_maps_of_the_mirrored_half(tmp_path, dev):
    """the finite flag covers both halves: a blow-up that only the mirrored pass sees is reported"""
    from test_model_gpu import make_model
    model, cfg = make_model(tmp_path, "f16", seed=2, calibrated=False)
    img = _images(1, 64, 64, 1)
    model.infer_batch_tensor(img.to(dev), flip=True)
    eng = list(model._engines.values())[-1]
    assert eng.flip and bool(eng.finite.all()) and eng.out[1].shape[0] == 2
    eng.out[1][1, 0, 0, 0] = float("inf")      # wh of the mirrored pass, after the step: the flag of the same buffers
    import detectron2_centernet_amd.ops as ops
    assert not bool(ops.finite_flag(eng.out[1], eng.out[2]).bool().all())
