"""The f16x3 training kernels at the layer shapes of the batch-16 3 x 512 x 512 DLA-34 step, each against a float64
reference over the whole output.  The small-map tests of test_train_x3_gpu.py give every workgroup one tile and every
BatchNorm reduction one block; the launchers size their grids from the CU count, so only maps this large reach the
multi-tile loops (a window weight-gradient workgroup prefetching its next tile while it works on the current one), the
many-rounds-per-CU scatter and the BatchNorm blocks that loop over row groups.  Each case first asserts that it reaches the
regime it exists for -- the weight gradients from the label the launcher gives the real call in a dry run, the scatter and
BatchNorm from a mirror of their launchers' formulas: a launcher change then fails here instead of silently testing something
smaller.

References are computed on the GPU in f64 without MIOpen: shifted-view matmuls for the convolutions, the plain formulas for
BatchNorm, autograd through the oracle's sampler (on the CPU, sampled images) for the DCNv2 scatter."""
import pytest
import torch

import conv_grad_cases as G
from conv_grad_cases import dgrad_ref, wgrad_ref
from detectron2_centernet_amd import _lib
from oracle import ctdet_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import detectron2_centernet_amd.ops as ops
    import detectron2_centernet_amd.ops_train as ot

    return ops, ot


@pytest.fixture(autouse=True)
def _free():
    yield
    torch.cuda.empty_cache()


def rel_err(got, ref):
    """max |got - ref| over the whole tensor relative to max |ref| (f64 on the GPU)"""
    err = (got.double() - ref).abs().max().item()
    return err / max(1e-30, ref.abs().max().item())


def check(got, ref, tol, what):
    r = rel_err(got, ref)
    print(f"{what}: rel err {r:.2e} (bound {tol:.0e})")
    assert r <= tol, f"{what}: max err {r:.3e} of the largest element > {tol:.0e}"


def randn(shape, gen, dev, scale=1.0):
    return torch.randn(*shape, generator=gen, device=dev) * scale


# ------------------------------------------------------------------------------------------ launcher mirror
def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def wgrad_regime(T, x, dy, Cout, k, s, p):
    """which weight-gradient kernel the launcher picks for ot.conv_wgrad(x, dy, ...) in f16x3 and how it splits the work, from
    the label of the real call's dry run: kernel, workgroups per pixel range (split), tiles (window, narrow) or 64-pixel K steps
    (generic) of the longest range -- the arithmetic of conv_grad_cases.pixel_ranges"""
    ops, ot = T
    L = _lib.lib()
    L.ctdet_set_label_mode(2)
    try:
        ot.conv_wgrad(x, dy, Cout, k, k, s, p, scale=1.0, comp=ops.F16X3)
        label = L.ctdet_last_kernel_label().decode()
    finally:
        L.ctdet_set_label_mode(0)
    B, H, W, Cin = x.shape
    row = G.Case("f16x3", "wgrad", B, H, W, Cin, Cout, k, s, p, 1, Cin, dy.shape[3], label, ())
    kind = {"win": "window"}.get(G.kernel_kind(row), G.kernel_kind(row))
    ranges, total = G.pixel_ranges(row)
    per = max(hi - lo for lo, hi in ranges)
    r = dict(kernel=kind, label=label, split=G.label_split(label)[1], per=per // 64 if kind == "generic" else per)
    r["M" if kind == "generic" else "tiles"] = total
    return r


def col2im_regime(B, H, W):
    """the dcn_col2im_window_kernel<NT> variant launch_col2im_window picks and its tiles per CU"""
    tiles = B * (H // 8) * (W // 16)
    ncu = cu_count()
    nt = 3 if tiles * 3 <= ncu else 5 if tiles * 2 <= ncu else 9
    return dict(variant=nt, tiles=tiles, per_cu=tiles * {3: 3, 5: 2, 9: 1}[nt] / ncu)


def bn_regime(M, C):
    """chan_reduce_kernel<float>'s grid (chan_blocks): row lanes per channel vector, blocks, row groups per block"""
    rows = 256 // (C // 4)
    nb = min(1024, max(1, -(-M // (rows * 8))))
    return dict(rows=rows, blocks=nb, groups=-(-M // (rows * nb)))


# ------------------------------------------------------------------------------------------ f64 references
# wgrad_ref / dgrad_ref: conv_grad_cases.py (checked there against torch double autograd by test_conv_grad_host.py)


# ------------------------------------------------------------------------------------------ convolution layers of the step
# (B, H, W, Cin, Cout, k, stride, pad, kernel, regime check).  The small tests reach at most 1 tile per workgroup (window,
# narrow) and 5 workgroups of <= 4 K steps (generic)
LAYERS = {
    "win_64x64@128": (16, 128, 128, 64, 64, 3, 1, 1, "window", lambda r: r["per"] >= 16),
    "win_128x128@64": (16, 64, 64, 128, 128, 3, 1, 1, "window", lambda r: r["per"] >= 16 and r["split"] % 8 == 0),
    "win_256x256@32": (16, 32, 32, 256, 256, 3, 1, 1, "window", lambda r: r["per"] >= 16 and r["split"] % 8 != 0),
    "win_head_64x256@128": (16, 128, 128, 64, 256, 3, 1, 1, "window", lambda r: r["per"] >= 64),
    "win_offset_64x27@128": (16, 128, 128, 64, 27, 3, 1, 1, "window", lambda r: r["per"] >= 8),
    "narrow_7x7_8x16@512": (16, 512, 512, 8, 16, 7, 1, 3, "narrow", lambda r: r["per"] >= 64),
    "narrow_3x3_16x16@512": (16, 512, 512, 16, 16, 3, 1, 1, "narrow", lambda r: r["per"] >= 64),
    "generic_s2_16x32@512": (16, 512, 512, 16, 32, 3, 2, 1, "generic", lambda r: r["per"] >= 32),
    "generic_s2_32x64@256": (16, 256, 256, 32, 64, 3, 2, 1, "generic", lambda r: r["per"] >= 8 and r["split"] >= 256),
    "generic_1x1_64x128@64": (16, 64, 64, 64, 128, 1, 1, 0, "generic", lambda r: r["split"] >= 256),
}
# the input gradient of the offset conv (27 couts) is not a plain conv_dgrad in the step
DGRAD_LAYERS = [n for n in LAYERS if "offset" not in n]


def _layer_data(name, dev, T):
    B, H, W, Cin, Cout, k, s, p, kern, ok = LAYERS[name]
    Cd = (Cout + 7) // 8 * 8          # dY pixel stride: the offset conv's 27 couts arrive padded to 32 channels
    g = torch.Generator(device=dev).manual_seed(sum(LAYERS[name][:8]))
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    x = randn((B, H, W, Cin), g, dev).relu_() * 1.5 + randn((B, H, W, Cin), g, dev, 0.1)   # f32, not f16-representable
    dy = randn((B, Ho, Wo, Cd), g, dev)
    r = wgrad_regime(T, x, dy, Cout, k, s, p)
    assert r["kernel"] == kern and ok(r), f"{name} no longer reaches its regime: {r}"
    print(name, r)
    return x, dy, (B, H, W, Cin, Cout, k, s, p), g


@pytest.mark.parametrize("name", list(LAYERS))
def test_fullsize_wgrad_x3_vs_f64(T, dev, name):
    """ot.conv_wgrad in f16x3 over the whole [Cout, k*k*Cin] gradient.  Bound: 2e-5 of the largest element (as the small
    test; f32 accumulation over these lengths contributes ~1e-6)"""
    ops, ot = T
    x, dy, (B, H, W, Cin, Cout, k, s, p), _ = _layer_data(name, dev, T)
    dw = ot.conv_wgrad(x, dy, Cout, k, k, s, p, scale=1.0, comp=ops.F16X3)
    check(dw.view(Cout, k, k, Cin), wgrad_ref(x, dy[..., :Cout], k, s, p), 2e-5, f"dW {name}")


def test_fullsize_wgrad_x3_dcn_columns_vs_f64(T, dev):
    """the DCNv2 weight gradient of a 64 -> 64 @ 128^2 layer: a 1x1 weight gradient (generic kernel) over the f32 sampled
    columns [262144][576] from ot.dcn_cols"""
    ops, ot = T
    B, H, W, C = 16, 128, 128, 64
    g = torch.Generator(device=dev).manual_seed(29)
    x = randn((B, H, W, C), g, dev)
    om = randn((B, H, W, 28), g, dev)
    om[..., :18] *= 2.0
    cols = ot.dcn_cols(x, om)
    del x, om
    assert cols.dtype == torch.float32 and cols.shape == (B, H, W, 9 * C)
    dy = randn((B, H, W, C), g, dev)
    r = wgrad_regime(T, cols, dy, C, 1, 1, 0)
    assert r["kernel"] == "generic" and r["per"] >= 16, r
    dw = ot.conv_wgrad(cols, dy, C, 1, 1, 1, 0, scale=1.0, comp=ops.F16X3)
    ref = dy.double().reshape(-1, C).t() @ cols.double().reshape(-1, 9 * C)
    check(dw, ref, 2e-5, "dW of the DCN layer (1x1 over the columns)")


@pytest.mark.parametrize("name", DGRAD_LAYERS)
def test_fullsize_dgrad_x3_vs_f64(T, dev, name):
    """ot.conv_dgrad in f16x3 (stride 2: the four-phase 2x2 conv + depth_to_space2_kernel<float>) on the whole batch; the
    f64 reference per 4-image slice.  Bound: 2e-5 of the largest element"""
    ops, ot = T
    x, dy, (B, H, W, Cin, Cout, k, s, p), g = _layer_data(name, dev, T)
    del x
    w = randn((Cout, Cin, k, k), g, dev, 1.0 / (Cin * k * k) ** 0.5)
    dx = ot.conv_dgrad(dy, w, s, p, (H, W), comp=ops.F16X3)
    assert dx.dtype == torch.float32 and dx.shape == (B, H, W, Cin)
    worst, err, scale = 0.0, 0.0, 0.0
    for b0 in range(0, B, 4):
        ref = dgrad_ref(dy[b0:b0 + 4], w, s, p, H, W)
        err = max(err, (dx[b0:b0 + 4].double() - ref).abs().max().item())
        scale = max(scale, ref.abs().max().item())
        del ref
    worst = err / scale
    print(f"dX {name}: rel err {worst:.2e} (bound 2e-05)")
    assert worst <= 2e-5, f"dX {name}: max err {worst:.3e} of the largest element"


# ------------------------------------------------------------------------------------------ DCNv2 scatter
def f32_sampling_offsets(om):
    """offsets [1, 18, H, W] (f64 holding f32 values) moved to where the kernels sample: they form h = f32(base + offset)
    (dcn_col2im_window_kernel), the oracle the exact sum.  A rounding of the sum can cross an integer coordinate, a kink of
    the bilinear interpolation where d/d(offset) jumps by a second difference of x (~1 relative at 128^2, where ulp(127) =
    7.6e-6); the derivative is compared at the kernel's own sampling point.  Also returns how many of the 18 * H * W
    coordinates cross a kink or the sampling border (-1 / H) under the rounding."""
    _, _, H, W = om.shape
    off = om.clone()
    crossed = 0
    for k in range(9):
        for a, base in ((0, torch.arange(H, dtype=torch.float64).view(H, 1) + k // 3 - 1),
                        (1, torch.arange(W, dtype=torch.float64).view(1, W) + k % 3 - 1)):
            exact = base + om[0, 2 * k + a]                       # exact in f64: a 24-bit offset plus a small integer
            rounded = exact.float().double()
            crossed += int((torch.floor(exact) != torch.floor(rounded)).sum())
            crossed += int(((exact > -1) != (rounded > -1)).sum() + ((exact < (H, W)[a]) != (rounded < (H, W)[a])).sum())
            off[0, 2 * k + a] = rounded - base
    return off, crossed


# (B, H, W, Cin, variant, tiles per CU at least)
COL2IM = [(16, 128, 128, 64, 9, 8), (16, 64, 64, 128, 9, 2), (16, 32, 32, 256, 5, 1)]


@pytest.mark.parametrize("shape", COL2IM, ids=lambda c: f"{c[1]}x{c[2]}x{c[3]}")
def test_fullsize_dcn_col2im_x3(T, dev, shape):
    """the LDS-window scatter (dcn_col2im_window_kernel<NT, float>) on a whole f32 layer: (a) two launches give a
    bit-identical d(offset, mask) -- it is written per pixel from fixed-order sums; (b) dx and d(offset, mask) against the
    f32-atomics kernel at the small test's bounds; (c) images 0, 7 and 15 against f64 autograd through the oracle's sampler
    with sum(d(columns) * columns) as the scalar, at the kernel's f32 sampling positions (f32_sampling_offsets)"""
    ops, ot = T
    B, H, W, Cin, nt, per_cu = shape
    r = col2im_regime(B, H, W)
    assert r["variant"] == nt and r["per_cu"] >= per_cu, r
    print(shape, r)
    g = torch.Generator(device=dev).manual_seed(sum(shape))
    x = randn((B, H, W, Cin), g, dev)
    dcol = randn((B, H, W, 9 * Cin), g, dev)
    om = randn((B, H, W, 28), g, dev)
    om[..., :18] *= 2.0               # offsets of a few pixels: samples cross the tile windows and the map borders
    dx_w, dom_w = ot.dcn_col2im_coord(dcol, x, om, comp=ops.F16X3)
    _, dom_w2 = ot.dcn_col2im_coord(dcol, x, om, comp=ops.F16X3)
    assert torch.equal(dom_w, dom_w2), "d(offset, mask) differs between two launches"
    del dom_w2
    dx_a, dom_a = ot.dcn_col2im_coord(dcol, x, om, comp=ops.F32)
    ex = (dx_w - dx_a).abs().max().item() / dx_a.abs().max().item()
    eo = (dom_w - dom_a).abs().max().item() / dom_a.abs().max().item()
    print(f"vs f32 atomics: dx {ex:.2e} (bound {2.0 ** -16:.1e}), dom {eo:.2e} (bound 1e-5)")
    assert ex <= 2.0 ** -16 and eo <= 1e-5, (ex, eo)
    del dx_a, dom_a
    for b in (0, 7, 15):
        xb = x[b].double().cpu().permute(2, 0, 1).unsqueeze(0).requires_grad_(True)
        omb = om[b, ..., :27].double().cpu().permute(2, 0, 1).unsqueeze(0)
        off, crossed = f32_sampling_offsets(omb[:, :18])
        print(f"image {b}: {crossed} sampling coordinates cross a kink under the f32 rounding")
        omb = torch.cat([off, omb[:, 18:]], 1).requires_grad_(True)
        cols, _, _ = O.dcnv2_columns(xb, omb[:, :18], torch.sigmoid(omb[:, 18:27]))        # [1, Cin, 9, H*W]
        dcb = dcol[b].double().cpu().view(H, W, 9, Cin).permute(3, 2, 0, 1).reshape(1, Cin, 9, H * W)
        (cols * dcb).sum().backward()
        check(dx_w[b].cpu(), xb.grad[0].permute(1, 2, 0), 1e-4, f"dx image {b}")
        check(dom_w[b, ..., :27].cpu(), omb.grad[0].permute(1, 2, 0), 1e-4, f"d(offset, mask) image {b}")


# ------------------------------------------------------------------------------------------ BatchNorm (f32 tensors)
# (B, H, W, C, residual, relu, shifted means)
BN = {"128x128x64_res_relu": (16, 128, 128, 64, True, True, False),
      "512x512x16": (16, 512, 512, 16, False, True, False),
      "16x16x512": (16, 16, 16, 512, False, False, False),
      "512x512x16_shifted_mean": (16, 512, 512, 16, False, False, True)}


@pytest.mark.parametrize("name", list(BN))
def test_fullsize_bn_train_f32_vs_f64(T, dev, name):
    """ot.bn_train_fwd / bn_train_bwd on f32 tensors against the f64 formulas (biased batch variance for the output,
    unbiased for running_var; dgamma, dbeta, dy through the kernel's own ReLU mask).  The shifted-mean case has channel
    means 0 ... 10 and standard deviations 1 ... 0.1 -- mean / std up to 100, where a one-pass E[y^2] - mean^2 in f32 loses
    the variance.  Bounds of the small test: 2e-6 forward, 2e-5 backward, 1e-5 running statistics"""
    ops, ot = T
    B, H, W, C, res, relu, shifted = BN[name]
    M = B * H * W
    r = bn_regime(M, C)
    print(name, r)
    assert r["rows"] == 256 // (C // 4)
    if C == 512:
        assert r["rows"] == 2, r                            # two row lanes per channel vector
    else:
        assert r["blocks"] == 1024 and r["groups"] >= 16, r  # every block loops over many row groups
    g = torch.Generator(device=dev).manual_seed(M + C)
    if shifted:
        mu = torch.linspace(0.0, 10.0, C, device=dev)
        sd = torch.linspace(1.0, 0.1, C, device=dev)
    else:
        mu = torch.full((C,), 0.5, device=dev)
        sd = torch.full((C,), 2.0, device=dev)
    y = randn((B, H, W, C), g, dev) * sd + mu
    rs = randn((B, H, W, C), g, dev) if res else None
    gamma = torch.rand(C, generator=g, device=dev) + 0.5
    beta = randn((C,), g, dev)
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    z, mean, invstd, scale = ot.bn_train_fwd(y, gamma, beta, rm, rv, 1e-5, 0.1, res=rs, relu=relu)

    y64 = y.double().view(M, C)
    mean64 = y64.mean(0)
    var64 = (y64 - mean64).square().mean(0)
    invstd64 = 1.0 / torch.sqrt(var64 + 1e-5)
    xhat = (y64 - mean64) * invstd64
    zr = xhat * gamma.double() + beta.double()
    if res:
        zr += rs.double().view(M, C)
    if relu:
        zr.clamp_(min=0.0)
    errs = {"invstd": (rel_err(invstd, invstd64), 2e-6), "fwd": (rel_err(z.view(M, C), zr), 2e-6),
            "running_mean": (rel_err(rm, 0.1 * mean64), 1e-5),
            "running_var": (rel_err(rv, 0.9 + 0.1 * var64 * M / (M - 1)), 1e-5)}
    del zr

    dz = randn((B, H, W, C), g, dev)
    dy, dres, dgamma, dbeta = ot.bn_train_bwd(dz, z, y, mean, invstd, scale, relu=relu, want_dres=res, grad_mult=1.0)
    gg = dz.double().view(M, C)
    if relu:
        gg = gg * (z.view(M, C) > 0)
    db = gg.sum(0)
    dg = (gg * xhat).sum(0)
    errs["dbeta"] = (rel_err(dbeta, db), 2e-5)
    errs["dgamma"] = (rel_err(dgamma, dg), 2e-5)
    dyr = (gamma.double() * invstd64) * (gg - db / M - xhat * (dg / M))
    errs["dy"] = (rel_err(dy.view(M, C), dyr), 2e-5)
    for k, (e, tol) in errs.items():
        print(f"{name} {k}: rel err {e:.2e} (bound {tol:.0e})")
    assert all(e <= tol for e, tol in errs.values()), {k: f"{e:.2e} > {tol:.0e}" for k, (e, tol) in errs.items() if e > tol}
    if res:
        assert torch.equal(dres.view(M, C), gg.float()), "dres is the masked dz"
