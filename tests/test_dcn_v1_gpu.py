"""DCNv1 (mask mode CTDET_DCN_MASK_NONE) on the HIP kernels: the mask-free variants of every DCN kernel in f32, f16x3 and f16.

The offset rows carry 18 channels followed by NaN (row stride 20 or 24): a finite, correct result shows that no kernel reads
beyond channel 17.  Forward: against the oracle's DCNv2 with an all-ones mask in f64, and BIT-identical to the modulated
kernels of the same route fed an all-ones probability mask (x * 1.0 is exact, so the two variants must compute the same
sums in the same order).  Backward (DCNFn): dx, d(offset) and dW against the oracle's restated backward with mask = 1, and
zeros in every d(om) channel from 18 on -- on the LDS-window scatter, the atomics-only scatter and, in f16x3, the fused
d(columns) scatter."""
import pytest
import torch

from oracle import ctdet_oracle as O

pytestmark = pytest.mark.gpu

# (precision, B, Cin = Cout, H, W, offset std, om row stride): 16x16 / 32x32 / 64x64 take the LDS-window kernels, 8x8 and
# 13x21 the ragged / gather forms
CASES = [
    ("f32", 1, 64, 16, 16, 2.0, 20), ("f32", 2, 128, 13, 21, 7.0, 24), ("f32", 1, 256, 8, 8, 0.0, 20),
    ("f16x3", 2, 64, 32, 32, 0.0, 20), ("f16x3", 1, 256, 8, 8, 4.0, 24), ("f16x3", 1, 128, 64, 64, 1.0, 20),
    ("f16x3", 1, 64, 13, 21, 3.0, 20),
    ("f16", 2, 64, 16, 16, 3.0, 20), ("f16", 1, 128, 32, 32, 5.0, 24), ("f16", 1, 256, 13, 21, 2.0, 20),
    ("f16", 1, 64, 64, 64, 0.5, 20),
]
# bounds of the existing DCNv2 tests per precision (test_dcn_boundary_gpu / test_train_x3_gpu), relative to max(1, |ref|)
FWD_TOL = {"f32": 2e-5, "f16x3": 2e-5, "f16": 8e-3}
BWD_TOL = {"f32": (2e-5, 8e-5, 2e-5), "f16x3": (1e-4, 1e-4, 3e-5), "f16": (8e-3, 3.2e-2, 8e-3)}   # dx, d(offset), dW


@pytest.fixture()
def mode(request):
    import detectron2_centernet_amd.ops as ops
    import detectron2_centernet_amd.ops_train as ot

    prec = request.param
    prev = ot.F32_COMPUTE
    ot.F32_COMPUTE = ops.F16X3 if prec == "f16x3" else ops.F32
    yield prec
    ot.F32_COMPUTE = prev


def _close(got, ref, tol, what):
    got = got.double().cpu()
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    err = (got - ref.double()).abs().max().item()
    scale = max(1.0, ref.abs().max().item())
    assert err <= tol * scale, f"{what}: max err {err} (scale {scale})"


def _data(prec, B, C, H, W, std, stride, seed):
    g = torch.Generator().manual_seed(seed)
    q = (lambda t: t.half().float()) if prec == "f16" else (lambda t: t)
    x = q(torch.randn(B, C, H, W, generator=g))
    w = q(torch.randn(C, C, 3, 3, generator=g) / (C * 9) ** 0.5)
    off = torch.randn(B, 18, H, W, generator=g) * std
    go = q(torch.randn(B, C, H, W, generator=g) * 0.1)
    return x, w, off, go


def _om_v1(off, stride, dev):
    """[B, H, W, stride] f32: the 18 offsets, NaN beyond"""
    B, _, H, W = off.shape
    om = torch.full((B, H, W, stride), float("nan"))
    om[..., :18] = off.permute(0, 2, 3, 1)
    return om.to(dev)


def _om_ones(off, dev):
    """the modulated kernels' operand with an all-ones probability mask: [B, H, W, 28]"""
    B, _, H, W = off.shape
    om = torch.zeros(B, H, W, 28)
    om[..., :18] = off.permute(0, 2, 3, 1)
    om[..., 18:27] = 1.0
    return om.to(dev)


def _dt(prec):
    return torch.float16 if prec == "f16" else torch.float32


@pytest.mark.parametrize("mode,B,C,H,W,std,stride", CASES, indirect=["mode"])
def test_dcn_v1_forward(dev, mode, B, C, H, W, std, stride):
    import detectron2_centernet_amd.ops as ops

    prec = mode
    x, w, off, _ = _data(prec, B, C, H, W, std, stride, seed=C + H + W)
    comp = {"f32": ops.F32, "f16x3": ops.F16X3, "f16": ops.F16}[prec]
    p = ops.PackedConv(w.to(dev), None, None, stride=1, pad=1, compute=comp, cout_align=64 if prec == "f16" else None)
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev).to(_dt(prec))
    om1 = _om_v1(off, stride, dev)
    y = ops.dcnv2(xd, om1, p, mask_is_prob=ops.DCN_MASK_NONE)
    y_ones = ops.dcnv2(xd, _om_ones(off, dev), p, mask_is_prob=ops.DCN_MASK_PROB)
    torch.cuda.synchronize()
    assert torch.isnan(om1[..., 18:]).all()
    assert torch.equal(y, y_ones), f"mask-free and ones-mask kernels differ by {(y.float() - y_ones.float()).abs().max().item()}"
    ref = O.dcnv2_forward(x.double(), off.double(), torch.ones(B, 9, H, W, dtype=torch.float64), w.double())
    _close(y[..., :C].float().permute(0, 3, 1, 2), ref, FWD_TOL[prec], f"{prec} forward {B}x{C} {H}x{W} std {std}")


# the fused d(columns) scatter is the f16x3 mode's
BWD_CASES = [c + (r,) for c in CASES for r in ("window", "atomics", "fused") if r != "fused" or c[0] == "f16x3"]


@pytest.mark.parametrize("mode,B,C,H,W,std,stride,route", BWD_CASES, indirect=["mode"])
def test_dcn_v1_backward(dev, mode, B, C, H, W, std, stride, route, monkeypatch):
    import detectron2_centernet_amd._lib as _lib
    import detectron2_centernet_amd.ops as ops
    import detectron2_centernet_amd.ops_train as ot

    prec = mode
    x, w, off, go = _data(prec, B, C, H, W, std, stride, seed=3 * C + H + W)
    monkeypatch.setattr(ot, "FUSE_DCOL", route == "fused")
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev).to(_dt(prec)).requires_grad_(True)
    omd = _om_v1(off, stride, dev).requires_grad_(True)
    wd = w.to(dev).requires_grad_(True)
    flags = _lib.TUNE_NO_COL2IM_WINDOW if route == "atomics" else 0
    with _lib.tuning(flags):
        y = ot.DCNFn.apply(xd, omd, wd, None, ops.DCN_MASK_NONE, 1.0)
        y.backward(go.permute(0, 2, 3, 1).contiguous().to(dev).to(y.dtype))
        torch.cuda.synchronize()
    gi, goff, _, gw, _ = O.dcnv2_backward(x.double(), off.double(), torch.ones(B, 9, H, W, dtype=torch.float64), w.double(),
                                          go.double(), with_bias=False)
    tdx, toff, tdw = BWD_TOL[prec]
    what = f"{prec} {route} {B}x{C} {H}x{W} std {std}"
    _close(xd.grad.float().permute(0, 3, 1, 2), gi, tdx, f"dx {what}")
    _close(omd.grad[..., :18].permute(0, 3, 1, 2), goff, toff, f"d(offset) {what}")
    assert omd.grad.shape[3] == stride and torch.equal(omd.grad[..., 18:], torch.zeros_like(omd.grad[..., 18:])), what
    _close(wd.grad, gw, tdw, f"dW {what}")


@pytest.mark.parametrize("frozen_w", [False, True])
def test_dcn_v1_frozen_bn_form(dev, frozen_w):
    """FrozenDCNFn (FrozenBN affine folded into the DCN epilogue, + ReLU), DCNv1 and modulated: forward and gradients against the
    oracle in f64 (relu(dcn * scale + bias); the backward restated with dY = dz * (z > 0) * scale), and against DCNFn followed
    by the same affine in torch.  frozen_w: the weight takes no gradient, and none is computed or returned."""
    import detectron2_centernet_amd.ops as ops
    import detectron2_centernet_amd.ops_train as ot

    prev = ot.F32_COMPUTE
    ot.F32_COMPUTE = ops.F32
    try:
        for mm in (ops.DCN_MASK_NONE, ops.DCN_MASK_LOGIT):
            g = torch.Generator().manual_seed(11 + mm)
            B, C, H, W = 2, 64, 16, 16
            x = torch.randn(B, H, W, C, generator=g)
            w = torch.randn(C, C, 3, 3, generator=g) / (C * 9) ** 0.5
            om = torch.randn(B, H, W, 20 if mm == ops.DCN_MASK_NONE else 28, generator=g) * 2.0
            if mm == ops.DCN_MASK_NONE:
                om[..., 18:] = float("nan")
            scale, bias = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
            dz = torch.randn(B, H, W, C, generator=g)
            outs = []
            for frozen in (True, False):
                xd, omd = x.to(dev).requires_grad_(True), om.to(dev).requires_grad_(True)
                wd = w.to(dev).requires_grad_(not frozen_w)
                if frozen:
                    z = ot.FrozenDCNFn.apply(xd, omd, wd, scale.to(dev), bias.to(dev), True, mm)
                else:
                    z = torch.relu(ot.DCNFn.apply(xd, omd, wd, None, mm, None) * scale.to(dev) + bias.to(dev))
                z.backward(dz.to(dev))
                assert (wd.grad is None) == frozen_w
                outs.append([t.detach().double().cpu() if t is not None else None for t in (z, xd.grad, omd.grad, wd.grad)])
            for a, b, name in zip(outs[0], outs[1], ("z", "dx", "dom", "dW")):
                if a is not None:
                    _close(a, b, 2e-5, f"mode {mm} {name} vs DCNFn")
            # independent reference
            z_hip, dx_hip, dom_hip, dw_hip = outs[0]
            xr, omr, wr = x.permute(0, 3, 1, 2).double(), om.permute(0, 3, 1, 2).double(), w.double()
            off = omr[:, :18]
            mask = torch.sigmoid(omr[:, 18:27]) if mm == ops.DCN_MASK_LOGIT else torch.ones(B, 9, H, W, dtype=torch.float64)
            s4, b4 = scale.double().view(1, -1, 1, 1), bias.double().view(1, -1, 1, 1)
            z_ref = torch.relu(O.dcnv2_forward(xr, off, mask, wr) * s4 + b4)
            _close(z_hip.permute(0, 3, 1, 2), z_ref, 2e-5, f"mode {mm} z vs oracle")
            gy = dz.permute(0, 3, 1, 2).double() * (z_hip.permute(0, 3, 1, 2) > 0).double() * s4
            gi, goff, gm, gw, _ = O.dcnv2_backward(xr, off, mask, wr, gy, with_bias=False)
            _close(dx_hip.permute(0, 3, 1, 2), gi, 2e-5, f"mode {mm} dx vs oracle")
            _close(dom_hip[..., :18].permute(0, 3, 1, 2), goff, 8e-5, f"mode {mm} d(offset) vs oracle")
            if mm == ops.DCN_MASK_LOGIT:
                _close(dom_hip[..., 18:27].permute(0, 3, 1, 2), gm * mask * (1 - mask), 8e-5, f"mode {mm} d(mask logit)")
            else:
                assert torch.equal(dom_hip[..., 18:], torch.zeros_like(dom_hip[..., 18:]))
            if not frozen_w:
                _close(dw_hip / ot.PARAM_GRAD_MULT, gw, 2e-5, f"mode {mm} dW vs oracle")
    finally:
        ot.F32_COMPUTE = prev


@pytest.mark.parametrize("route", ["window", "atomics"])
def test_dcn_v1_f16_dom(dev, route):
    """the f16 form of d(om) (dom_channels: directly the dY of an f16 offset conv's backward) under DCNv1: d(offset) equal to
    the f32 form's to f16 rounding, channels 18..31 exactly zero, dx unchanged"""
    import detectron2_centernet_amd._lib as _lib
    import detectron2_centernet_amd.ops as ops
    import detectron2_centernet_amd.ops_train as ot

    g = torch.Generator().manual_seed(5)
    B, H, W, C = 2, 16, 32, 64
    x = torch.randn(B, H, W, C, generator=g).half().to(dev)
    dcol = (torch.randn(B, H, W, 9 * C, generator=g) * 0.1).half().to(dev)
    om = torch.full((B, H, W, 20), float("nan"))
    om[..., :18] = torch.randn(B, H, W, 18, generator=g) * 3.0
    om = om.to(dev)
    with _lib.tuning(_lib.TUNE_NO_COL2IM_WINDOW if route == "atomics" else 0):
        dx16, dom16 = ot.dcn_col2im_coord(dcol, x, om, ops.DCN_MASK_NONE, dom_channels=32)
        dx32, dom32 = ot.dcn_col2im_coord(dcol, x, om, ops.DCN_MASK_NONE)
        torch.cuda.synchronize()
    assert dom16.dtype == torch.float16 and dom16.shape[3] == 32 and dom32.shape[3] == 20
    assert torch.equal(dom16[..., 18:], torch.zeros_like(dom16[..., 18:]))
    assert torch.equal(dom32[..., 18:], torch.zeros_like(dom32[..., 18:]))
    ref = dom32[..., :18].double().cpu()
    err = (dom16[..., :18].double().cpu() - ref).abs().max().item()
    assert err <= 2.0 ** -10 * ref.abs().max().item(), err
    assert (dx16 - dx32).abs().max().item() <= 1e-6 * dx32.abs().max().item()
