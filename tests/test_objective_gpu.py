"""The kernels that define the training objective -- gaussian_targets, focal_loss, reg_l1_loss -- and the eval step's guard
finite_flag against float64 references, at the edge cases of objective_cases.py: per-class alpha on vectors that straddle
pixels, ragged and more than 256 focal blocks, want_grad=False, grad_scale, all four stats; non-square maps, corner / radius-0 /
oversized / out-of-map / out-of-class objects and stale caller-owned maps for the targets; strided channel slices for RegL1 and
finite_flag.

Bounds: the project's existing ones.  test_objective_host.py shows that the oracle itself, evaluated in f32, meets them, with the
gaps it measured.  Every test prints the error it observed before it asserts (run with -s); the largest over the table, measured on
an MI355X:
    hm                  <= 1e-6 abs                                    0 (equal to the oracle on all three cases)
    focal loss          rel 1e-5, abs 1e-6                             1.3e-6 relative (1x2x5x6 without positives)
    focal gradient      <= 1e-5 * max(1, max|ref|) * grad_scale        9.2e-7 of the same unit (2x80x101x130 without positives)
    focal pos / neg     as the loss                                    1.4e-7 / 1.3e-6 relative
    RegL1 loss          rel 1e-5                                       6.5e-8 relative
    RegL1 gradient      < 1e-6 * grad_scale                            1.7e-9 * grad_scale
The focal loss keeps a factor of 8: log(1 - p) loses digits in f32 where p is close to 1, in the kernel as in the f32 oracle.
Index, mask, wh, reg, num_pos, 1/num_pos, the finite flag and the gradients beyond the clamp are compared exactly.
"""
import numpy as np
import pytest
import torch

import objective_cases as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    import detectron2_centernet_amd.ops as ops

    return ops


def _rel(a, ref):
    return abs(a - ref) / abs(ref) if ref else abs(a)


# --------------------------------------------------------------------------------------------------------------- focal
@pytest.mark.parametrize("case", T.FOCAL_CASES, ids=T.focal_id)
def test_focal_loss(ops, dev, case):
    inp, ref = T.focal_inputs(case), T.focal_reference(case)
    logits, gt, alpha = inp["logits"].to(dev), inp["gt"].to(dev), inp["alpha"].to(dev)
    gref = ref["grad"]
    gmax = max(1.0, gref.abs().max().item())
    loss_ng, stats_ng, grad_ng = ops.focal_loss(logits, gt, alpha, want_grad=False)
    assert grad_ng is None
    for scale in (1.0, 1024.0):
        loss, stats, grad = ops.focal_loss(logits, gt, alpha, want_grad=True, grad_scale=scale)
        st = stats.cpu().double().tolist()
        gerr = (grad.cpu().double() - gref * scale).abs().max().item()
        print(f"focal {T.focal_id(case)} scale {scale:g}: loss rel err {_rel(loss.item(), ref['loss']):.2e}, grad err / (scale * "
              f"max(1, max|ref|)) {gerr / (scale * gmax):.2e}, pos rel err {_rel(st[0], ref['pos']):.2e}, neg rel err "
              f"{_rel(st[1], ref['neg']):.2e}")
        assert loss.item() == pytest.approx(ref["loss"], rel=1e-5, abs=1e-6)
        assert st[0] == pytest.approx(ref["pos"], rel=1e-5, abs=1e-6)
        assert st[1] == pytest.approx(ref["neg"], rel=1e-5, abs=1e-6)
        assert st[2] == float(ref["num_pos"])
        assert stats[3].item() == (float(np.float32(1.0 / ref["num_pos"])) if ref["num_pos"] else 1.0)
        assert gerr <= 1e-5 * gmax * scale
        if case.pinned:
            g = grad.cpu().reshape(-1)
            assert g[inp["marks"]["pin_pos"]] == 0 and g[inp["marks"]["pin_neg"]] == 0
        # the loss and the sums do not depend on the gradient path or its scale: same reduction order, bit for bit
        assert torch.equal(loss, loss_ng) and torch.equal(stats, stats_ng)


def test_focal_loss_refuses_a_map_that_is_no_multiple_of_4(ops, dev):
    B, C, H, W = T.FOCAL_RAISES
    logits, gt = torch.zeros(B, H, W, C, device=dev), torch.zeros(B, H, W, C, device=dev)
    alpha = torch.ones(C, device=dev)
    for want_grad in (True, False):
        with pytest.raises(RuntimeError):
            ops.focal_loss(logits, gt, alpha, want_grad=want_grad)
    torch.cuda.synchronize()
    assert not logits.any() and not gt.any() and bool((alpha == 1).all())


@pytest.mark.parametrize("case", [c for c in T.FOCAL_CASES if c.pinned or (c.C, c.H, c.with_pos) == (80, 16, False)], ids=T.focal_id)
def test_focal_loss_fn_backward(dev, case):
    """FocalLossFn under autograd with an upstream factor: .grad = GRAD_SCALE * factor * the float64 gradient"""
    from detectron2_centernet_amd import ops_train

    inp, ref = T.focal_inputs(case), T.focal_reference(case)
    factor = 0.375
    logits = inp["logits"].to(dev).requires_grad_(True)
    loss = ops_train.FocalLossFn.apply(logits, inp["gt"].to(dev), inp["alpha"].to(dev))
    (loss * factor).backward()
    assert loss.item() == pytest.approx(ref["loss"], rel=1e-5, abs=1e-6)
    scale = ops_train.GRAD_SCALE * factor
    gmax = max(1.0, ref["grad"].abs().max().item())
    assert (logits.grad.cpu().double() - ref["grad"] * scale).abs().max().item() <= 1e-5 * gmax * scale


# ------------------------------------------------------------------------------------------------------------- targets
@pytest.mark.parametrize("case", T.TARGET_CASES, ids=lambda c: c.name)
def test_gaussian_targets(ops, dev, case):
    ref = T.target_reference(case)
    B = case.boxes.shape[0]
    hm_buf = torch.full((B, case.H, case.W, case.C), float("nan"), device=dev) if case.prefill else None
    out = ops.gaussian_targets(case.boxes.to(dev), case.classes.to(dev), case.counts.to(dev), case.H, case.W, case.C, hm=hm_buf)
    if case.prefill:
        assert out["hm"].data_ptr() == hm_buf.data_ptr()
    hm = out["hm"].cpu().permute(0, 3, 1, 2).numpy()
    assert not np.isnan(hm).any(), "stale values survive in the map"
    for key in ("ind", "reg_mask", "wh", "reg"):          # all 128 slots, those past counts included
        got = out[key].cpu().numpy()
        assert got.dtype == ref[key].dtype and np.array_equal(got, ref[key]), key
    err = np.abs(hm.astype(np.float64) - ref["hm"]).max()
    print(f"targets {case.name}: hm max abs err {err:.2e}")
    assert np.array_equal(hm == 1.0, ref["hm"] == 1.0)
    assert np.array_equal(hm > 0, ref["hm"] > 0)
    assert err <= 1e-6


# -------------------------------------------------------------------------------------------------------------- reg L1
@pytest.mark.parametrize("case", T.REG_CASES, ids=T.reg_id)
def test_reg_l1_loss(ops, dev, case):
    inp, ref = T.reg_inputs(case), T.reg_reference(case)
    buf = inp["buf"].to(dev)
    pred = buf[..., case.lo:case.lo + 2]
    mask, ind, tgt = inp["mask"].to(dev), inp["ind"].to(dev), inp["target"].to(dev)
    outside = [ch for ch in range(case.S) if not case.lo <= ch < case.lo + 2]
    loss_ng, grad_ng = ops.reg_l1_loss(pred, mask, ind, tgt, want_grad=False)
    assert grad_ng is None
    for scale in T.REG_GRAD_SCALES:
        gbuf = torch.zeros_like(buf)
        loss, grad = ops.reg_l1_loss(pred, mask, ind, tgt, grad_scale=scale, grad=gbuf[..., case.lo:case.lo + 2])
        g = gbuf.cpu()
        gerr = (g.double() - ref["grad"] * scale).abs().max().item()
        print(f"reg_l1 {T.reg_id(case)} scale {scale:g}: loss rel err {_rel(loss.item(), ref['loss']):.2e}, grad err / scale "
              f"{gerr / scale:.2e}")
        assert loss.item() == pytest.approx(ref["loss"], rel=1e-5)
        assert torch.equal(loss, loss_ng)
        assert gerr < 1e-6 * scale
        assert not g[..., outside].any(), "the gradient leaked into the channels outside the slice"
    # an all-zero mask: loss 0 / 1e-4, no gradient
    gbuf = torch.zeros_like(buf)
    loss0, _ = ops.reg_l1_loss(pred, torch.zeros_like(mask), ind, tgt, grad=gbuf[..., case.lo:case.lo + 2])
    assert loss0.item() == 0.0 == T.reg_reference(case, zero_mask=True)["loss"] and not gbuf.any()


@pytest.mark.parametrize("S", [4, 8])
def test_reg_l1_two_losses_share_one_gradient_buffer(ops, dev, S):
    """the wh and the offset loss write into channel slices of one buffer: neither touches the other's channels"""
    a, b = T.RegCase(3, 128, S, 0), T.RegCase(3, 128, S, 2)
    gbuf = torch.zeros(3, T.REG_H, T.REG_W, S, device=dev)
    snap = {}
    for c in (a, b):
        inp = T.reg_inputs(c)
        ops.reg_l1_loss(inp["buf"].to(dev)[..., c.lo:c.lo + 2], inp["mask"].to(dev), inp["ind"].to(dev), inp["target"].to(dev),
                        grad_scale=1024.0, grad=gbuf[..., c.lo:c.lo + 2])
        snap[c] = gbuf.cpu().clone()
    assert not snap[a][..., 2:].any() and snap[a][..., 0:2].any()
    assert torch.equal(snap[b][..., 0:2], snap[a][..., 0:2]) and not snap[b][..., 4:].any()
    for c in (a, b):
        ref = T.reg_reference(c)["grad"][..., c.lo:c.lo + 2] * 1024.0
        assert (snap[b][..., c.lo:c.lo + 2].double() - ref).abs().max().item() < 1e-6 * 1024.0


@pytest.mark.parametrize("case", [T.RegCase(3, 128, 4, 0), T.RegCase(2, 37, 8, 0)], ids=T.reg_id)
def test_reg_l1_fn_backward_on_padded_channels(dev, case):
    """RegL1Fn on a head output that carries padded channels (only the first two are the prediction): .grad = GRAD_SCALE * factor *
    the float64 gradient, exactly 0 in the padding"""
    from detectron2_centernet_amd import ops_train

    assert case in T.REG_CASES
    inp, ref = T.reg_inputs(case), T.reg_reference(case)
    factor = 0.1
    pred = inp["buf"].to(dev).requires_grad_(True)              # [B, H, W, S], S > 2
    loss = ops_train.RegL1Fn.apply(pred, inp["mask"].to(dev), inp["ind"].to(dev), inp["target"].to(dev))
    (loss * factor).backward()
    assert loss.item() == pytest.approx(ref["loss"], rel=1e-5)
    scale = ops_train.GRAD_SCALE * factor
    g = pred.grad.cpu()
    assert (g.double() - ref["grad"] * scale).abs().max().item() < 1e-6 * scale
    assert not g[..., 2:].any()


# -------------------------------------------------------------------------------------------------------------- finite
@pytest.mark.parametrize("way", T.FINITE_WAYS)
@pytest.mark.parametrize("case", T.FINITE_CASES, ids=T.finite_id)
def test_finite_flag(ops, dev, case, way):
    bufs = T.finite_buffers(case, way)
    want = T.finite_reference(case, bufs)
    flag = ops.finite_flag(*[b.to(dev)[..., case.lo:case.hi] for b in bufs])
    assert flag.dtype == torch.int32 and flag.shape == (1,)
    assert flag.item() == want
