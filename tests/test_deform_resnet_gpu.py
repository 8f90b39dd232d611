"""The deformable ResNet-50 CenterNet (ctdet_res_50_1x + MODEL.RESNETS.DEFORM_ON_PER_STAGE [False, True, True, True]) on the
HIP kernels, modulated (DCNv2, sigmoid of the raw offset conv in the kernel) and not (DCNv1, the mask-free kernels):
  * zero offsets: the model equals plain R50 with the same weights (modulated: with conv2 halved, mask = sigmoid(0));
  * non-zero offsets: eval against an f64 composition of oracle.model_ref pieces with oracle.dcnv2_forward (below), with the
    bounds of test_resnet50_centernet_eval_matches_oracle;
  * a training step (FrozenBN and BN norms) against torch autograd through that composition, with the bounds of
    test_resnet50_training_step_matches_oracle, conv2_offset gradients included."""
import os
import shutil
import sys

import pytest
import torch
import torch.nn.functional as F

from oracle import ctdet_oracle as O
from oracle import model_ref as MR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEFORM = [False, True, True, True]


def _make(tmp_path, precision, deform=True, modulated=False, norm="FrozenBN"):
    from detectron2_centernet_amd.config import get_cfg
    from detectron2_centernet_amd.data.catalog import register_synthetic
    from detectron2_centernet_amd.modeling import build_model
    sys.path.insert(0, GOLDEN)
    from weights import fill_state_dict

    for n in ("Base-CenterNet.yaml", "ctdet_res_50_1x.yaml"):
        shutil.copy(os.path.join(GOLDEN, "g16_configs", n), tmp_path / n)
    cfg = get_cfg()
    cfg.merge_from_file(str(tmp_path / "ctdet_res_50_1x.yaml"))
    cfg.MODEL.CENTERNET.HIP_PRECISION = precision
    cfg.MODEL.RESNETS.NORM = norm
    if deform:
        cfg.MODEL.RESNETS.DEFORM_ON_PER_STAGE = DEFORM
        cfg.MODEL.RESNETS.DEFORM_MODULATED = modulated
    register_synthetic("bulb_train", num_classes=80)
    model = build_model(cfg).eval()
    sd = fill_state_dict({k: v.cpu() for k, v in model.state_dict().items()}, seed=21)
    return model, cfg, sd


def _load(model, sd):
    model.load_state_dict({k: v.to(model.device) for k, v in sd.items()})


def _offset_weights(sd, scale, seed=4):
    """conv2_offset weights that move samples by a few pixels (fill_state_dict's scale would throw them off the map)"""
    g = torch.Generator().manual_seed(seed)
    for k in list(sd):
        if ".conv2_offset." in k:
            fan = sd[k][0].numel() if k.endswith("weight") else 1
            sd[k] = torch.randn(sd[k].shape, generator=g) * (scale / fan ** 0.5 if k.endswith("weight") else 0.5)
    return sd


def _heads(model, img):
    model.score_threshold = 0.0
    model([{"image": img[b]} for b in range(img.shape[0])])
    eng = next(iter(model._engines.values()))
    assert eng.graph_nodes.get("kernel", 0) > 0 and set(eng.graph_nodes) <= {"kernel", "empty"}, eng.graph_nodes
    return [t.float().cpu().permute(0, 3, 1, 2) for t in eng.out]


# ---------------------------------------------------------------- f64 composition (oracle.model_ref pieces + dcnv2_forward)
def _norm(sd, p, x, training):
    if training and (p + ".num_batches_tracked") in sd:       # trainable BatchNorm: batch statistics
        return F.batch_norm(x, None, None, sd[p + ".weight"], sd[p + ".bias"], True, 0.1, 1e-5)
    return MR.frozen_bn(sd, p, x)


def _conv_norm(sd, p, x, stride=1, pad=0, training=False):
    return _norm(sd, p + ".norm", F.conv2d(x, sd[p + ".weight"], None, stride, pad), training)


def deform_bottleneck(sd, p, x, stride, modulated, training=False, taps=None):
    """resnet.py:215-320 (DeformBottleneckBlock), STRIDE_IN_1X1: the stride on conv1"""
    out = F.relu(_conv_norm(sd, p + ".conv1", x, stride, training=training))
    om = F.conv2d(out, sd[p + ".conv2_offset.weight"], sd[p + ".conv2_offset.bias"], 1, 1)
    off = om[:, :18]
    mask = torch.sigmoid(om[:, 18:27]) if modulated else torch.ones_like(om[:, :9])
    out = F.relu(_norm(sd, p + ".conv2.norm", O.dcnv2_forward(out, off, mask, sd[p + ".conv2.weight"]), training))
    if taps is not None and p.endswith("res3.0"):
        taps["res3.0.conv2"] = out
    out = _conv_norm(sd, p + ".conv3", out, training=training)
    sc = _conv_norm(sd, p + ".shortcut", x, stride, training=training) if (p + ".shortcut.weight") in sd else x
    return F.relu(out + sc)


def plain_bottleneck(sd, p, x, stride, training=False):
    out = F.relu(_conv_norm(sd, p + ".conv1", x, stride, training=training))
    out = F.relu(_conv_norm(sd, p + ".conv2", out, 1, 1, training=training))
    out = _conv_norm(sd, p + ".conv3", out, training=training)
    sc = _conv_norm(sd, p + ".shortcut", x, stride, training=training) if (p + ".shortcut.weight") in sd else x
    return F.relu(out + sc)


def centernet_dconv_forward(sd, x, modulated, training=False):
    y = MR.deconv_layers(sd, "deconv_layers", _res4_ref(sd, x, modulated, training), training)
    return MR.centernet_heads(MR.Net(sd), y)


def _res4_ref(sd, x, modulated, training=False, taps=None):
    """res4 of the f64 composition; taps: a dict that receives the outputs of the blocks named in TAPS"""
    x = F.relu(MR._conv_norm(sd, "backbone.stem.conv1", x, 2, 3))
    x = F.max_pool2d(x, kernel_size=3, stride=2, padding=1)
    for si, nblk in enumerate((3, 4, 6)):
        for bi in range(nblk):
            stride = 2 if (bi == 0 and si > 0) else 1
            name = f"backbone.res{si + 2}.{bi}"
            if DEFORM[si]:
                x = deform_bottleneck(sd, name, x, stride, modulated, training and si > 0, taps)
            else:
                x = plain_bottleneck(sd, name, x, stride, training and si > 0)
            if taps is not None and name[len("backbone."):] in TAPS:
                taps[name[len("backbone."):]] = x
    if taps is not None:
        taps["res4"] = x
    return x


# ---------------------------------------------------------------------------------------------------------- tests
# Backbone features, max error relative to their largest magnitude, at three taps: the deformable 3x3 of the first deformable
# block (res3.0.conv2: DCN + folded norm + ReLU, before the residual path dilutes what the offsets do), that block's output
# and res4.  f32 / f16x3 against f64: rounding of f32 sums (measured <= 2.5e-7); f16 stores every activation in f16 (2^-11
# relative per store: one ulp of the largest value is 4.9e-4 of it), which accumulates over the blocks (measured <= 6e-4 at
# res3.0, <= 1e-3 at res4).
FEAT_TOL = {"f32": {"res3.0.conv2": 2e-6, "res3.0": 2e-6, "res4": 2e-6},
            "f16x3": {"res3.0.conv2": 2e-6, "res3.0": 2e-6, "res4": 2e-6},
            "f16": {"res3.0.conv2": 1e-3, "res3.0": 1e-3, "res4": 2e-3}}
# zero offsets against plain R50: the two paths agree bit for bit for DCNv1; modulated (mask 1/2 in the kernel against halved
# weights) they differ in the last bits (measured 1.4e-7 in f16x3, 1.0e-6 in f16); f16: a fifth of one f16 ulp of the largest
# value
ZERO_TOL = {"f32": 2e-6, "f16x3": 2e-6, "f16": 1e-4}
SENSITIVITY = 10      # a control that must fail the bound: the effect it removes is at least this many bounds
TAPS = ("res3.0.conv2", "res3.0", "res4")


def _feats(model, x):
    """backbone features of the preprocessed NCHW batch x on the model's kernels (its precision), block by block: {tap: NCHW f64}"""
    from detectron2_centernet_amd.layers import hipnn

    from detectron2_centernet_amd import ops

    ctx = model._ctx
    bb = model.backbone
    out = {}
    dcnv2 = ops.dcnv2

    def tap_dcn(*a, **kw):      # the first deformable 3x3's output (DeformBottleneckBlock.hip_forward calls ops.dcnv2)
        y = dcnv2(*a, **kw)
        out.setdefault("res3.0.conv2", y.double().cpu().permute(0, 3, 1, 2))
        return y

    ops.dcnv2 = tap_dcn
    try:
        with torch.no_grad():
            y = bb.stem.hip_forward(hipnn.to_nhwc(x.to(model.device), ctx, pad_to=8), ctx)
            for stage, name in bb.stages_and_names:
                for i, block in enumerate(stage):
                    y = block.hip_forward(y, ctx)
                    if f"{name}.{i}" in TAPS:
                        out[f"{name}.{i}"] = y.double().cpu().permute(0, 3, 1, 2)
    finally:
        ops.dcnv2 = dcnv2
    out["res4"] = y.double().cpu().permute(0, 3, 1, 2)
    return out


def _res4(model, x):
    return _feats(model, x)["res4"]


def _rel(a, b):
    return (a - b).abs().max().item() / b.abs().max().item()


def _zero_offsets(sd):
    return {k: (torch.zeros_like(v) if ".conv2_offset." in k else v) for k, v in sd.items()}


@pytest.mark.parametrize("modulated", [False, True])
@pytest.mark.parametrize("precision", ["f32", "f16x3", "f16"])
def test_zero_offset_equals_plain_r50(tmp_path, dev, precision, modulated):
    """conv2_offset zeroed: every sample sits on the grid, so the deformable 3x3 IS the plain 3x3 (DCNv1) or the plain 3x3 at
    half weight (modulated: mask = sigmoid(0)).  res4 features and heads against plain R50 with the same weights; two controls
    show the bound is tight enough to see the offsets (random conv2_offset weights) and the mask (conv2 not halved)."""
    model, cfg, sd = _make(tmp_path, precision, modulated=modulated)
    sd = _zero_offsets(sd)
    _load(model, sd)
    plain, _, _ = _make(tmp_path, precision, deform=False)
    sdp = {k: v for k, v in sd.items() if ".conv2_offset." not in k}
    half = {k: (v * 0.5 if (".conv2.weight" in k and k.startswith(("backbone.res3", "backbone.res4"))) else v)
            for k, v in sdp.items()}
    _load(plain, half if modulated else sdp)
    g = torch.Generator().manual_seed(7)
    img = torch.randint(0, 256, (2, 3, 96, 128), generator=g, dtype=torch.uint8)
    x, _ = O.preprocess([i for i in img], cfg.MODEL.PIXEL_MEAN, cfg.MODEL.PIXEL_STD, 16)
    f_def, f_plain = _feats(model, x), _feats(plain, x)
    tol = ZERO_TOL[precision]
    err = max(_rel(f_def[t], f_plain[t]) for t in ("res3.0", "res4"))
    got, want = _heads(model, img), _heads(plain, img)
    htol = {"hm": 2e-5, "wh": 4e-4, "reg": 4e-4} if precision != "f16" else {"hm": 2e-3, "wh": 4e-2, "reg": 4e-2}
    herr = {n: (a - b).abs().max().item() / (1.0 if n == "hm" else max(1.0, b.abs().max().item()))
            for a, b, n in zip(got, want, ("hm", "wh", "reg"))}
    # controls: the same comparison with non-zero offsets, and (modulated) against plain R50 with conv2 not halved
    _load(model, _offset_weights(dict(sd), 1.0))
    ctl_off = _rel(_feats(model, x)["res3.0"], f_plain["res3.0"])
    ctl_mask = None
    if modulated:
        _load(plain, sdp)
        ctl_mask = _rel(f_def["res3.0"], _feats(plain, x)["res3.0"])
    print(precision, modulated, "res4 rel err", err, "heads", herr, "controls: offsets", ctl_off, "mask", ctl_mask)
    assert err <= tol, err
    for n in herr:
        assert herr[n] <= htol[n], (n, herr[n])
    assert ctl_off > SENSITIVITY * tol, ctl_off
    assert ctl_mask is None or ctl_mask > SENSITIVITY * tol, ctl_mask


@pytest.mark.parametrize("size", [128, 256])
@pytest.mark.parametrize("modulated", [False, True])
@pytest.mark.parametrize("precision", ["f32", "f16x3", "f16"])
def test_deform_r50_eval_matches_f64_composition(tmp_path, dev, precision, modulated, size):
    """offsets of a few pixels: res4 features and heads against the f64 composition; the control (the composition with the
    offsets zeroed) must miss the features by many bounds, so the bound sees what the offsets do"""
    model, cfg, sd = _make(tmp_path, precision, modulated=modulated)
    sd = _offset_weights(sd, 4.0)
    _load(model, sd)
    g = torch.Generator().manual_seed(size)
    img = torch.randint(0, 256, (2, 3, size, size), generator=g, dtype=torch.uint8)
    hm, wh, reg = _heads(model, img)
    x, _ = O.preprocess([i for i in img], cfg.MODEL.PIXEL_MEAN, cfg.MODEL.PIXEL_STD, 16)
    feat = _feats(model, x)
    sdd = {k: v.double() if v.dtype.is_floating_point else v for k, v in sd.items()}
    f_ref, f_ctl = {}, {}
    with torch.no_grad():
        z = MR.centernet_heads(MR.Net(sdd), MR.deconv_layers(sdd, "deconv_layers", _res4_ref(sdd, x.double(), modulated, taps=f_ref)))
        _res4_ref(_zero_offsets(sdd), x.double(), modulated, taps=f_ctl)
    err = {t: _rel(feat[t], f_ref[t]) for t in TAPS}
    ctl = _rel(f_ctl["res3.0.conv2"], f_ref["res3.0.conv2"])
    hm_ref = torch.clamp(torch.sigmoid(z["hm"]), 1e-4, 1 - 1e-4)
    err_hm = (hm.double() - hm_ref).abs().max().item()
    err_wh = (wh.double() - z["wh"]).abs().max().item() / max(1.0, z["wh"].abs().max().item())
    err_reg = (reg.double() - z["reg"]).abs().max().item() / max(1.0, z["reg"].abs().max().item())
    print(precision, modulated, size, "res4 rel err", err, "control", ctl, "heatmap err", err_hm, "wh rel", err_wh,
          "reg rel", err_reg)
    for t in TAPS:
        assert err[t] <= FEAT_TOL[precision][t], (t, err)
    assert ctl > SENSITIVITY * FEAT_TOL[precision]["res3.0.conv2"], ctl
    if precision != "f16":
        assert err_hm <= 1e-5 and err_wh <= 2e-4 and err_reg <= 2e-4
    else:
        assert err_hm <= 1e-3 and err_wh <= 2e-2 and err_reg <= 2e-2


@pytest.mark.parametrize("norm", ["FrozenBN", "BN"])
@pytest.mark.parametrize("modulated", [False, True])
@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_deform_r50_training_step_matches_autograd(tmp_path, dev, precision, modulated, norm):
    """f32 and the default training mode f16x3, with the bounds both meet in test_resnet50_training_step_matches_oracle /
    test_full_training_step_f16x3_matches_fp32_oracle (losses 1e-3, every gradient cos >= 0.999, norm ratio within 1 %)"""
    from detectron2_centernet_amd.data.catalog import synthetic_sample
    from detectron2_centernet_amd.structures import Boxes, Instances

    model, cfg, sd0 = _make(tmp_path, precision, modulated=modulated, norm=norm)
    sd0 = _offset_weights(sd0, 1.0)
    _load(model, sd0)
    model.train()
    inputs = []
    for i in range(2):
        smp = synthetic_sample(i, size=128, num_classes=80, max_boxes=6)
        inst = Instances((128, 128))
        inst.gt_boxes, inst.gt_classes = Boxes(smp["boxes"]), smp["classes"]
        inputs.append({"image": smp["image"], "instances": inst})
    losses = model(inputs)
    sum(losses.values()).backward()
    trainable = {n for n, p in model.named_parameters() if p.requires_grad}
    assert any(".conv2_offset." in n for n in trainable)
    sd = {k: (v.double().clone().requires_grad_(True) if k in trainable else
              (v.double().clone() if v.dtype.is_floating_point else v.clone())) for k, v in sd0.items()}
    x_ref, _ = O.preprocess([d["image"] for d in inputs], cfg.MODEL.PIXEL_MEAN, cfg.MODEL.PIXEL_STD, 16)
    z = centernet_dconv_forward(sd, x_ref.double(), modulated, training=True)
    targets = [O.gen_heatmap(d["instances"].gt_boxes.tensor, d["instances"].gt_classes, 32, 32, 80) for d in inputs]
    ref = MR.centernet_losses({k: v.float() for k, v in z.items()}, targets, [1.0])
    sum(ref.values()).backward()
    for k in ("hm_loss", "wh_loss", "off_loss"):
        got, want = losses[k].item(), ref[k].item()
        print(precision, modulated, norm, k, got, want)
        assert abs(got - want) <= 1e-3 * max(1.0, abs(want)), (k, got, want)
    worst, name_of = 1.0, ""
    for name, p in model.named_parameters():
        if not p.requires_grad:
            assert p.grad is None
            continue
        gref = sd[name].grad
        assert p.grad is not None and gref is not None, name
        if gref.abs().max() == 0:
            continue
        cos = torch.nn.functional.cosine_similarity(p.grad.double().cpu().flatten(), gref.flatten(), dim=0).item()
        ratio = (p.grad.double().cpu().norm() / gref.norm()).item()
        if cos < worst:
            worst, name_of = cos, name
        assert 0.99 < ratio < 1.01, (name, ratio)
        assert cos >= 0.999, (name, cos)
    print(precision, modulated, norm, "worst gradient cosine", worst, name_of)


# ---------------------------------------------------------------------------------------------------------- full size
def _bench_model(precision, seed, modulated=False):
    """bench.py's ResNet-50 model (its config text and init: ~1 px conv2_offset offsets) with DEFORM_ON_PER_STAGE"""
    import tempfile

    import bench
    from detectron2_centernet_amd.config import get_cfg
    from detectron2_centernet_amd.data.catalog import register_synthetic
    from detectron2_centernet_amd.modeling import build_model

    d = tempfile.mkdtemp(prefix="ctdet_cfg_")
    with open(os.path.join(d, "Base-CenterNet.yaml"), "w") as f:
        f.write(bench.BASE_YAML)
    with open(os.path.join(d, "ctdet_res_50_1x.yaml"), "w") as f:
        f.write(bench.RES50_YAML)
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(d, "ctdet_res_50_1x.yaml"))
    cfg.MODEL.CENTERNET.HIP_PRECISION = precision
    cfg.MODEL.DEVICE = "cuda:0"
    cfg.MODEL.RESNETS.DEFORM_ON_PER_STAGE = DEFORM
    cfg.MODEL.RESNETS.DEFORM_MODULATED = modulated
    register_synthetic("bulb_train", num_classes=80)
    torch.manual_seed(seed)
    model = build_model(cfg)
    g = torch.Generator().manual_seed(seed + 1)
    for name, m in model.named_modules():
        if name.endswith("conv2_offset"):
            m.weight.data.copy_((torch.randn(m.weight.shape, generator=g) * (0.5 / (m.weight.shape[1] * 9) ** 0.5)).to(m.weight.device))
            m.bias.data.copy_((torch.randn(m.bias.shape, generator=g) * 0.5).to(m.bias.device))
    model.wh[-1].bias.data.fill_(3.0)
    for m in model.deconv_layers.modules():
        if isinstance(m, torch.nn.ConvTranspose2d):
            m.weight.data.normal_(0, (2.0 / (m.weight.shape[0] * 4)) ** 0.5)
    return model, cfg


def test_fullsize_deform_r50_training_step_16x512_f16x3(dev):
    """R50-dconv (DCNv1), 16 x 3 x 512 x 512, f16x3: five steps eagerly and five under the trainer's captured HIP graph.  Losses
    finite, the captured graph holds kernel nodes only, the replayed trajectory is the eager one (the bounds of
    test_fullsize_dla34_training_step_16x512 in f16x3), and the conv2_offset parameters move."""
    import math

    from detectron2_centernet_amd.engine.bench_train import synthetic_batch
    from detectron2_centernet_amd.engine.train_loop import SimpleTrainer

    res = {}
    for mode in ("eager", "graph"):
        model, cfg = _bench_model("f16x3", seed=3)
        cfg.SOLVER.IMS_PER_BATCH = 16
        tr = SimpleTrainer(model, None, cfg)
        tr.use_hip_graph = mode == "graph"
        offs = [m.conv2_offset.weight for m in model.backbone.modules() if hasattr(m, "conv2_offset")]
        assert len(offs) == 10 and all(w.requires_grad for w in offs)
        off0 = [w.detach().clone() for w in offs]
        p0 = tr.optimizer.flat_param.clone()
        batch = synthetic_batch(16, 512, 0, dev)
        hist = [sum(float(v) for v in tr.run_step_tensors(*batch).values()) for _ in range(5)]
        assert all(math.isfinite(h) for h in hist), hist
        assert tr.graph_state == ("captured" if mode == "graph" else "eager"), tr.graph_state
        for g in (g for g in tr._graphs.values() if g["graph"] is not None):
            assert g["nodes"].get("kernel", 0) > 0 and set(g["nodes"]) <= {"kernel", "empty"}, g["nodes"]
        for w, w0 in zip(offs, off0):
            assert (w.detach() - w0).abs().max().item() > 0
        res[mode] = (hist, (tr.optimizer.flat_param - p0), tr.optimizer.flat_mom.clone())
        del tr, model, offs
        torch.cuda.empty_cache()
    (he, de, me), (hg, dg, mg) = res["eager"], res["graph"]
    print("losses eager", he, "graph", hg)
    assert he[-1] != he[0]
    for a, b in zip(he, hg):
        assert abs(a - b) <= 1e-5 * abs(a), (he, hg)
    assert de.abs().max() > 0 and (de - dg).abs().max().item() <= 2e-2 * de.abs().max().item()
    assert (me - mg).abs().max().item() <= 2e-2 * me.abs().max().item()


@pytest.mark.parametrize("modulated", [False, True])
def test_fullsize_deform_r50_eval_8x800(dev, modulated):
    """8 x 3 x 800 x 800: res3 / res4 are 100^2 / 50^2 maps, off the 8x16 tile grid (the ragged DCN kernels).  f16x3 outputs
    finite and equal to the f32 run within the bounds the f32 run meets against the oracle (heat map 1e-5 absolute, wh / reg
    2e-4 relative); res4 features within 2x the feature bound of the small-map tests (both runs round) -- relative to the
    largest feature magnitude, with 8x more pixels per channel than there."""
    import bench
    from detectron2_centernet_amd.layers import hipnn

    images = bench.synthetic_images(8, 800, 0, dev)
    out, feats = {}, {}
    for precision in ("f32", "f16x3"):
        model, cfg = _bench_model(precision, seed=5, modulated=modulated)
        model.eval()
        model.score_threshold = 0.0
        with torch.no_grad():
            model.infer_batch_tensor(images)
        eng = next(e for e in model._engines.values() if e.B == 8)
        out[precision] = [t.float().cpu().permute(0, 3, 1, 2) for t in eng.out]
        x, _ = O.preprocess([images[i].cpu() for i in range(2)], cfg.MODEL.PIXEL_MEAN, cfg.MODEL.PIXEL_STD, 16)
        feats[precision] = _res4(model, x)
        del model, eng
        torch.cuda.empty_cache()
    hm, wh, reg = out["f16x3"]
    assert hm.shape == (8, 80, 200, 200) and feats["f32"].shape[2:] == (50, 50)
    for t in out["f16x3"] + out["f32"]:
        assert torch.isfinite(t).all()
    hm32, wh32, reg32 = out["f32"]
    e_hm = (hm - hm32).abs().max().item()
    e_wh = (wh - wh32).abs().max().item() / max(1.0, wh32.abs().max().item())
    e_reg = (reg - reg32).abs().max().item() / max(1.0, reg32.abs().max().item())
    e_f = _rel(feats["f16x3"], feats["f32"])
    print(modulated, "f16x3 vs f32: hm", e_hm, "wh", e_wh, "reg", e_reg, "res4", e_f)
    assert e_hm <= 1e-5 and e_wh <= 2e-4 and e_reg <= 2e-4
    assert e_f <= 2 * FEAT_TOL["f32"]["res4"]

