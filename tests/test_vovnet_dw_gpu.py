"""Depthwise VoVNet-19 bodies (`V-19-slim-dw-eSE`, `V-19-dw-eSE`) on the HIP kernels: the depthwise 3x3 kernels against f64
torch (forward, input and weight gradient, determinism, a never-cleared workspace), the backbone against the reference's own
module (G19), CenterNet eval through the captured engine and the training step against the f64 composition of
tests/vovnet_dw_ref.py with the oracle's deconv layers, heads and losses, the captured trainer against an eager one, and the
full BASELINE-sized eval and training step."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vovnet_dw_ref as R
from oracle import ctdet_oracle as O
from oracle import model_ref as MR

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SLIM = "V-19-slim-dw-eSE"


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _dw64(x, w, stride):
    return F.conv2d(x.double(), w.double(), None, stride, 1, 1, w.shape[0])


def _check_fwd(got, x, w, stride, f16):
    """f32: |y - y64| <= 1e-6 (|W| * |X|) elementwise; f16: against the f64 result of the f16-rounded inputs, one f16 output
    rounding plus 1e-3 (|W| * |X|)"""
    ref = _dw64(x, w, stride)
    mag = _dw64(x.abs(), w.abs(), stride)
    err = (got.double() - ref).abs()
    bound = (1e-3 * mag + ref.abs() * 2.0 ** -11 + 2.0 ** -24) if f16 else 1e-6 * mag
    assert (err <= bound).all(), (err - bound).max().item()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_dwconv3x3_forward_matches_f64(dev, dtype):
    import detectron2_centernet_amd.ops as ops
    g = torch.Generator().manual_seed(190)
    f16 = dtype == torch.float16
    for ci, C in enumerate((64, 80, 96, 112, 128, 224)):
        for H, W in ((5, 7), (33, 47), (128, 128)):
            if H == 128 and C not in (64, 224):
                continue
            for stride in (1, 2):
                B = 1 + (ci + H) % 3
                x = torch.randn(B, C, H, W, generator=g)
                w = torch.randn(C, 1, 3, 3, generator=g) * 0.4
                if f16:
                    x = x.half().float()
                y = ops.dwconv3x3(nhwc(x).to(dtype).to(dev), w.to(dev), stride)
                assert y.dtype == dtype and y.shape == (B, (H - 1) // stride + 1, (W - 1) // stride + 1, C)
                _check_fwd(nchw(y.float().cpu()), x, w, stride, f16)
    # channel-slice views on input and output (16-element offsets keep the 16-byte alignment in both dtypes)
    C, H, W = 96, 33, 47
    x = torch.randn(2, C, H, W, generator=g)
    x = x.half().float() if f16 else x
    w = torch.randn(C, 1, 3, 3, generator=g) * 0.4
    xb = torch.randn(2, H, W, C + 48, generator=g).to(dtype).to(dev)
    xb[..., 16:16 + C] = nhwc(x).to(dtype).to(dev)
    for stride in (1, 2):
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        ob = torch.full((2, Ho, Wo, C + 32), 7.0, dtype=dtype, device=dev)
        y = ops.dwconv3x3(xb[..., 16:16 + C], w.to(dev), stride, out=ob[..., 16:16 + C])
        assert y.data_ptr() == ob[..., 16:16 + C].data_ptr()
        _check_fwd(nchw(ob[..., 16:16 + C].float().cpu()), x, w, stride, f16)
        assert (ob[..., :16] == 7.0).all() and (ob[..., 16 + C:] == 7.0).all()     # nothing written outside the slice


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_dwconv3x3_gradients_match_f64(dev, dtype):
    """DwConv3x3Fn backward: dX (the forward kernel with the taps rotated) within 1e-6 (|W| * |dY|) (f16: plus one output
    rounding and 1e-3 (|W| * |dY|)), dW (scaled by PARAM_GRAD_MULT like every parameter gradient) within 1e-5 sum |dY| |X|
    -- the f16 products are exact in f32, so the f16 bound is the same; two launches are bit-identical, a NaN-filled
    workspace changes nothing (every slot is written), `into` adds to the slot"""
    from detectron2_centernet_amd import ops_train
    g = torch.Generator().manual_seed(191)
    f16 = dtype == torch.float16
    mult = ops_train.PARAM_GRAD_MULT
    for (B, C, H, W) in ((1, 64, 5, 7), (2, 96, 33, 47), (3, 224, 33, 47), (2, 80, 128, 128)):
        x = torch.randn(B, C, H, W, generator=g)
        dy = torch.randn(B, C, H, W, generator=g)
        w = torch.randn(C, 1, 3, 3, generator=g) * 0.4
        if f16:
            x, dy = x.half().float(), dy.half().float()
        xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
        F.conv2d(xr, wr, None, 1, 1, 1, C).backward(dy.double())
        xh = nhwc(x).to(dtype).to(dev).requires_grad_(True)
        wh = w.to(dev).requires_grad_(True)
        y = ops_train.DwConv3x3Fn.apply(xh, wh, 1)
        y.backward(nhwc(dy).to(dtype).to(dev))
        # dX = conv_transpose(dY, W): the magnitude bound is the same adjoint on |dY|, |W|
        mag = F.conv_transpose2d(dy.abs().double(), w.abs().double(), None, 1, 1, 0, C)
        err = (nchw(xh.grad.float().cpu()).double() - xr.grad).abs()
        bound = (1e-3 * mag + xr.grad.abs() * 2.0 ** -11 + 2.0 ** -24) if f16 else 1e-6 * mag
        assert (err <= bound).all(), ("dx", B, C, H, W, (err - bound).max().item())
        dwm = torch.nn.grad.conv2d_weight(x.abs().double(), w.shape, dy.abs().double(), 1, 1, 1, C)
        dwg = wh.grad.cpu().double() / mult
        assert ((dwg - wr.grad).abs() <= 1e-5 * dwm).all(), ("dw", B, C, H, W, ((dwg - wr.grad).abs() / dwm).max().item())
        # determinism and the never-cleared workspace
        xd, dyd = nhwc(x).to(dtype).to(dev), nhwc(dy).to(dtype).to(dev)
        a = ops_train.dwconv3x3_wgrad(xd, dyd, scale=1.0)
        b = ops_train.dwconv3x3_wgrad(xd, dyd, scale=1.0)
        assert torch.equal(a, b)
        from detectron2_centernet_amd import _lib
        nb = _lib.lib().ctdet_dwconv3x3_wgrad_workspace_bytes(B, H, W, C, 0 if f16 else 1)
        ws = torch.full((nb // 4,), float("nan"), device=dev)
        c = ops_train.dwconv3x3_wgrad(xd, dyd, scale=1.0, workspace=ws)
        assert torch.equal(a, c) and not torch.isnan(ws).any()
        into = torch.ones(C, 1, 3, 3, device=dev)
        assert ops_train.dwconv3x3_wgrad(xd, dyd, scale=1.0, into=into) is None
        assert torch.equal(into, 1.0 + a)
    # the stride-2 backward is not built: the autograd node says so instead of computing something else
    xh = torch.randn(1, 9, 9, 64, device=dev, requires_grad=True)
    y = ops_train.DwConv3x3Fn.apply(xh, torch.randn(64, 1, 3, 3, device=dev), 2)
    with pytest.raises(NotImplementedError):
        y.sum().backward()


def _backbone(body, precision, dev, seed=None, tmp_path=None):
    from detectron2_centernet_amd.config import get_cfg
    from detectron2_centernet_amd.data.catalog import register_synthetic
    from detectron2_centernet_amd.modeling import build_model
    cfg = get_cfg()
    cfg.merge_from_file(R.write_cfg(tmp_path, body))
    cfg.MODEL.CENTERNET.HIP_PRECISION = precision
    register_synthetic("bulb_train", num_classes=80)
    model = build_model(cfg)
    if seed is not None:
        sd = R.dw_state_dict({k: v.cpu() for k, v in model.state_dict().items()}, seed=seed)
        model.load_state_dict({k: v.to(model.device) for k, v in sd.items()})
    return model, cfg


@pytest.mark.parametrize("precision", ["f32", "f16x3", "f16"])
def test_dw_backbones_match_reference_module(tmp_path, dev, precision):
    """both bodies on the HIP kernels against the reference module's stage outputs (G19), same weights: f32 / f16x3 within 1e-5
    of the largest output, f16 within 5e-3"""
    from detectron2_centernet_amd import ops
    from detectron2_centernet_amd.layers import hipnn
    gz = np.load(os.path.join(GOLDEN, "g19_vovnet19_dw.npz"))
    for body, tag, seed in ((SLIM, "slim", 191), ("V-19-dw-eSE", "dw", 192)):
        model, _ = _backbone(body, precision, dev, tmp_path=tmp_path)
        bb = model.backbone.eval()
        sd = R.dw_state_dict({k: v.cpu() for k, v in bb.state_dict().items()}, seed=seed)   # make_g19's keys: no prefix
        bb.load_state_dict({k: v.to(dev) for k, v in sd.items()})
        ctx = hipnn.Ctx({"f32": ops.F32, "f16x3": ops.F16X3, "f16": ops.F16}[precision])
        x = torch.from_numpy(gz["x"]).to(dev)
        with torch.no_grad():
            outs = bb.hip_forward(hipnn.to_nhwc(x, ctx, pad_to=8), ctx)
        for s in ("stage2", "stage3", "stage4", "stage5"):
            ref = torch.from_numpy(gz[f"{tag}_{s}"])
            got = nchw(outs[s][..., :ref.shape[1]].float().cpu())
            err = ((got - ref).abs().max() / ref.abs().max()).item()
            print(precision, body, s, f"{err:.2e}")
            assert err <= (5e-3 if precision == "f16" else 1e-5), (body, s, err)


@pytest.mark.parametrize("precision", ["f32", "f16x3", "f16"])
def test_dw_centernet_eval_matches_f64(tmp_path, dev, precision):
    """`ctdet_vovnet2_19_slim_1x.yaml` with CONV_BODY V-19-slim-dw-eSE through the captured eval engine: heat map against the
    f64 composition (f32 / f16x3 5e-5, f16 1e-3), the decode of the HIP heat map bit-exact with the oracle's, kernels-only
    graph"""
    model, cfg = _backbone(SLIM, precision, dev, seed=31, tmp_path=tmp_path)
    model.eval()
    model.score_threshold = 0.0
    g = torch.Generator().manual_seed(6)
    img = torch.randint(0, 256, (2, 3, 90, 120), generator=g, dtype=torch.uint8)      # padded to 96 x 128
    out = model([{"image": img[b]} for b in range(2)])
    eng = next(iter(model._engines.values()))
    assert eng.graph is not None
    assert eng.graph_nodes.get("kernel", 0) > 0 and set(eng.graph_nodes) <= {"kernel", "empty"}, eng.graph_nodes
    hm, wh, reg = [t.float().cpu().permute(0, 3, 1, 2) for t in eng.out]
    assert hm.shape == (2, 80, 24, 32)
    x, _ = O.preprocess([i for i in img], cfg.MODEL.PIXEL_MEAN, cfg.MODEL.PIXEL_STD, 16)
    sd = {k: v.detach().double().cpu() for k, v in model.state_dict().items()}
    with torch.no_grad():
        z = R.centernet_forward(sd, x.double(), SLIM)
    hm_ref = torch.clamp(torch.sigmoid(z["hm"]), 1e-4, 1 - 1e-4).float()
    assert hm_ref.std().item() > 3e-3
    err = (hm - hm_ref).abs().max().item()
    print(precision, "dw heat map err", err)
    assert err <= (1e-3 if precision == "f16" else 5e-5)
    rb, rs, rc, ri = O.ctdet_decode(hm, wh, reg, down_ratio=4, K=100)
    boxes, scores, classes, inds = [t.cpu() for t in eng.dec]
    assert torch.equal(scores, rs) and torch.equal(classes, rc) and torch.equal(inds.long(), ri)
    for b in range(2):
        inst = out[b]["instances"]
        bb, ss, cc = O.inference_single_image(rb[b], rs[b], rc[b], 100, 0.0)
        bb, keep = O.detector_postprocess(bb, (90, 120), 90, 120)
        assert torch.equal(inst.scores.cpu(), ss[keep]) and torch.equal(inst.pred_classes.cpu(), cc[keep])


def _inputs(n, size):
    from detectron2_centernet_amd.data.catalog import synthetic_sample
    from detectron2_centernet_amd.structures import Boxes, Instances
    inputs = []
    for i in range(n):
        smp = synthetic_sample(i, size=size, num_classes=80, max_boxes=6)
        inst = Instances((size, size))
        inst.gt_boxes, inst.gt_classes = Boxes(smp["boxes"]), smp["classes"]
        inputs.append({"image": smp["image"], "instances": inst})
    return inputs


@pytest.mark.parametrize("precision", ["f32", "f16x3", "f16"])
def test_dw_training_step_matches_f64(tmp_path, dev, precision):
    """the training step of the dw config (FREEZE_AT 2: stem + stage2 on the inference kernels; stage3 / stage4 as autograd
    nodes: reduction 1x1, DwConv3x3Fn, FrozenConvFn, eSE) against f64 autograd of the composition: losses 1e-4 relative
    (f16: 1e-2), gradient cosine >= 0.99999 (f16: 0.999) for the dw, pw, reduction and eSE fc weights of stage3 / stage4"""
    model, cfg = _backbone(SLIM, precision, dev, seed=19, tmp_path=tmp_path)
    sd0 = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    model.train()
    inputs = _inputs(2, 128)
    losses = model(inputs)
    sum(losses.values()).backward()
    trainable = {n for n, p in model.named_parameters() if p.requires_grad}
    sd = {k: (v.double().clone().requires_grad_(True) if k in trainable else v.double().clone()) for k, v in sd0.items()}
    x_ref, _ = O.preprocess([d["image"] for d in inputs], cfg.MODEL.PIXEL_MEAN, cfg.MODEL.PIXEL_STD, 16)
    z = R.centernet_forward(sd, x_ref.double(), SLIM, training=True)
    targets = [O.gen_heatmap(d["instances"].gt_boxes.tensor, d["instances"].gt_classes, 32, 32, 80) for d in inputs]
    ref = MR.centernet_losses(z, targets, [1.0])
    sum(ref.values()).backward()
    ltol = 1e-2 if precision == "f16" else 1e-4
    for k in ("hm_loss", "wh_loss", "off_loss"):
        got, want = losses[k].item(), ref[k].item()
        print(precision, k, got, want)
        assert abs(got - want) <= ltol * abs(want), (k, got, want)
    ctol = 0.999 if precision == "f16" else 0.99999
    seen = {"dw_conv3x3": 0, "pw_conv1x1": 0, "reduction_0/conv": 0, "ese.fc": 0}
    worst = (1.0, "")
    for name, p in model.named_parameters():
        if name.startswith(("backbone.stem", "backbone.stage2")):
            assert not p.requires_grad and p.grad is None, name          # frozen: no gradient at all
            continue
        if not name.startswith(("backbone.stage3", "backbone.stage4")):
            continue
        kind = next((k for k in seen if k in name), None)
        if kind is None:
            continue
        gref = sd[name].grad
        assert p.grad is not None and gref is not None and gref.abs().max() > 0, name
        cos = F.cosine_similarity(p.grad.double().cpu().flatten(), gref.flatten(), dim=0).item()
        worst = min(worst, (cos, name))
        assert cos >= ctol, (name, cos)
        seen[kind] += 1
    print(precision, "worst gradient cosine", worst, seen)
    assert seen == {"dw_conv3x3": 6, "pw_conv1x1": 6, "reduction_0/conv": 2, "ese.fc": 4}, seen


def test_dw_trainer_graph_matches_eager(tmp_path, dev):
    """SimpleTrainer with the default captured step (eager, eager, capture + replay, replay) against an all-eager trainer from
    the same state: kernels-only graphs, losses of every step and the parameters afterwards within 1e-5 relative (a fixed
    bound)"""
    from detectron2_centernet_amd.engine.bench_train import synthetic_batch
    from detectron2_centernet_amd.engine.train_loop import SimpleTrainer
    res = {}
    for mode in ("eager", "graph"):
        model, cfg = _backbone(SLIM, "f32", dev, seed=23, tmp_path=tmp_path)
        model.train()
        cfg.SOLVER.IMS_PER_BATCH = 2
        tr = SimpleTrainer(model, None, cfg)
        tr.use_hip_graph = mode == "graph"
        p0 = tr.optimizer.flat_param.clone()
        w = getattr(model.backbone.stage3.OSA3_1.layers[0], "OSA3_1_0/dw_conv3x3").weight
        w0 = w.detach().clone()
        batch = synthetic_batch(2, 128, 0, dev)
        hist = [{k: float(v) for k, v in tr.run_step_tensors(*batch).items()} for _ in range(4)]
        if mode == "graph":
            assert tr.graph_state == "captured", tr._graphs
            for g in (g for g in tr._graphs.values() if g["graph"] is not None):
                assert g["nodes"].get("kernel", 0) > 0 and set(g["nodes"]) <= {"kernel", "empty"}, g["nodes"]
        res[mode] = (hist, tr.optimizer.flat_param.detach().clone(), p0, w.detach().clone(), w0)
    (he, pe, p0, we, w0), (hg, pg, _, wg, _) = res["eager"], res["graph"]
    for a, b in zip(he, hg):
        for k in a:
            assert math.isfinite(a[k]) and abs(a[k] - b[k]) <= 1e-5 * abs(a[k]), (k, he, hg)
    assert (pe - p0).abs().max() > 0 and (we - w0).abs().max() > 0      # the step trains, the dw weights included
    assert (pg - pe).abs().max().item() <= 1e-5 * pe.abs().max().item()
    assert (wg - we).abs().max().item() <= 1e-5 * we.abs().max().item()


def test_dw_fullsize_eval_f16x3_matches_f32(tmp_path, dev):
    """BASELINE's eval size (64 x 3 x 512 x 512) with the slim dw body: f16x3 heat map within 5e-5 of the f32 mode's, the
    decode of the HIP map bit-exact with the oracle's, scores sorted; kernels-only graphs"""
    import bench
    images = bench.synthetic_images(64, 512, 0, dev)
    maps = {}
    for precision in ("f32", "f16x3"):
        model, _ = _backbone(SLIM, precision, dev, seed=64, tmp_path=tmp_path)
        model.eval()
        model.score_threshold = 0.0
        model.wh[2].bias.data.fill_(4.0)
        with torch.no_grad():
            model.infer_batch_tensor(images)
        eng = next(e for e in model._engines.values() if e.B == 64)
        assert eng.graph_nodes.get("kernel", 0) > 0 and set(eng.graph_nodes) <= {"kernel", "empty"}, eng.graph_nodes
        maps[precision] = ([t.float().cpu().permute(0, 3, 1, 2).contiguous() for t in eng.out], [t.cpu() for t in eng.dec])
        del model, eng
        torch.cuda.empty_cache()
    (h32, _, _), _ = maps["f32"]
    (hm, wh, reg), (boxes, scores, classes, inds) = maps["f16x3"]
    assert hm.shape == (64, 80, 128, 128) and torch.isfinite(wh).all() and torch.isfinite(reg).all()
    err = (hm - h32).abs().max().item()
    print("full-size dw f16x3 vs f32 heat map", err)
    assert err <= 5e-5
    rb, rs, rc, ri = O.ctdet_decode(hm, wh, reg, down_ratio=4, K=100)
    assert torch.equal(scores, rs) and torch.equal(classes, rc) and torch.equal(inds.long(), ri)
    assert (scores[:, :-1] >= scores[:, 1:]).all()
    assert inds.min() >= 0 and inds.max() < 128 * 128


def test_dw_fullsize_training_step_captured(tmp_path, dev):
    """one captured f16x3 training step at 16 x 512 x 512 (eager, eager, then capture + replay): kernels only, finite losses"""
    from detectron2_centernet_amd.engine.bench_train import synthetic_batch
    from detectron2_centernet_amd.engine.train_loop import SimpleTrainer
    model, cfg = _backbone(SLIM, "f16x3", dev, seed=16, tmp_path=tmp_path)
    model.train()
    cfg.SOLVER.IMS_PER_BATCH = 16
    tr = SimpleTrainer(model, None, cfg)
    batch = synthetic_batch(16, 512, 0, dev)
    for _ in range(3):
        vals = {k: float(v) for k, v in tr.run_step_tensors(*batch).items()}
        assert all(math.isfinite(v) for v in vals.values()), vals
    assert tr.graph_state == "captured", tr._graphs
    for g in (g for g in tr._graphs.values() if g["graph"] is not None):
        assert g["nodes"].get("kernel", 0) > 0 and set(g["nodes"]) <= {"kernel", "empty"}, g["nodes"]
