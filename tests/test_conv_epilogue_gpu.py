"""The shared conv epilogue (csrc/conv_common.h: epilogue_wave, and epilogue_tiles for the ragged cases) through every kernel
family that ends in it, at the smallest shape that selects the kernel (the shapes of conv_tile_cases.py where a row exists).

Per family the contraction is computed once in float64 (conv / matmul / oracle DCNv2 on doubles) and shared; every variant then
applies its own epilogue to it in double:
  * scale, bias and residual each on and off as far as the Python entry points allow (f16x3 always carries the row scale of
    its packed weights; the deformable entry points take no residual);
  * activation none / ReLU / sigmoid-clamp;
  * the residual read from a channel slice of a wider tensor (res_stride != out_stride), the output written into a channel
    slice of a wider sentinel-filled tensor with one more image behind it: the neighbouring channels and the trailing image
    must stay untouched;
  * a Cout that is 4 * odd: the last cout-tile pair of a wave is cut, the ragged path runs (CUT_LABEL: where the selector
    then changes the cout tile);
  * the residual being the output buffer itself (in place), which must give exactly what the separate residual gives.
Checks: every element against the float64 reference within the project's bounds (f32 / f16x3: 1e-5, f16: 3e-3, each times
max(1, |ref|max)); the same launch twice is torch.equal; and for f32 outputs the identity
    out(scale, bias, residual, ReLU) == relu(out(scale, bias) + residual)      (torch.equal, computed in f32 by torch)
which holds exactly because the residual add and the max involve no product: nothing can be contracted or reordered."""
import pytest
import torch
import torch.nn.functional as F

import conv_tile_cases as T
from detectron2_centernet_amd import _lib
from oracle import ctdet_oracle as O

pytestmark = pytest.mark.gpu

COMPUTE = {"f16": _lib.F16, "f32": _lib.F32, "f16x3": _lib.F16X3}
SENTINEL = -1234.0          # exact in f16
LEFT = 8                    # sentinel channels in front of the output slice (16-byte aligned for f16 and f32)
RIGHT = 8                   # and behind it
CLAMP = (0.25, 0.75)


def _uk(mode, bp, bc, form="conv"):
    return T._uk(mode, bp, bc, form)


# name -> Case (epilogue / out_dtype of the row are not used here: every variant sets its own)
FAMILIES = {
    # f16x3 tap-pair kernels: 8 x 32- and 16 x 16-pixel tiles, 32-cout tiles (one workgroup row) and 64-cout tiles (>= 256 workgroups)
    "pair2_tw32_bc32": T.conv("f16x3", "conv3x3_halo_pair2_kernel<256x32,f16x3>", 1, 8, 32, 32, 64, k=3),
    "pair2_tw16_bc32": T.conv("f16x3", "conv3x3_halo_pair2_kernel<16x16x32,f16x3>", 1, 16, 16, 32, 64, k=3),
    "pair2_tw32_bc64": T.conv("f16x3", "conv3x3_halo_pair2_kernel<256x64,f16x3>", 1, 64, 64, 32, 1024, k=3),
    "pair2_tw16_bc64": T.conv("f16x3", "conv3x3_halo_pair2_kernel<16x16x64,f16x3>", 1, 80, 80, 32, 704, k=3),
    # f16x3 uniform-K
    "uk_x3_256x128": T.conv("f16x3", _uk("f16x3", 256, 128), 1, 120, 137, 16, 1024),
    "uk_x3_256x64": T.conv("f16x3", _uk("f16x3", 256, 64), 1, 137, 139, 16, 448),
    "uk_x3_128x128": T.conv("f16x3", _uk("f16x3", 128, 128), 2, 9, 13, 16, 128),
    "uk_x3_128x128_cat": T.cat("f16x3", _uk("f16x3", 128, 128, "cat"), 2, 9, 13, (16, 32), 128),
    "mfma_x3_128x128": T.conv("f16x3", T._generic("f16x3", 128, 128), 2, 9, 13, 12, 128, k=3),
    # f16x3 DCNv2 window kernels
    "dcn_x3_2x64": T.dcn("f16x3", "dcn_f16x3_window_kernel<8x16,64>", 1, 16, 32, 16, 64),
    "dcn_x3_2x64_fused": T.dcn("f16x3", "dcn_f16x3_window_kernel<8x16,64,offset conv fused>", 1, 16, 32, 32, 64, entry="dcnv2_offset"),
    "dcn_x3_1x128": T.dcn("f16x3", "dcn_f16x3_window_kernel<8x16,128>", 1, 16, 32, 16, 128),
    # f16
    "halo_f16_256x64": T.conv("f16", "conv3x3_halo_kernel<256x64,f16>", 1, 24, 32, 32, 128, k=3),
    "tap2_f16_256x64": T.conv("f16", "conv3x3_halo_tap2_kernel<256x64,f16>", 1, 24, 32, 64, 64, k=3),
    "uk_f16_128x64": T.conv("f16", _uk("f16", 128, 64), 2, 9, 13, 32, 128),
    "uk_f16_256x128": T.conv("f16", _uk("f16", 256, 128), 1, 120, 137, 32, 1024),
    # f32
    "uk_f32_128x128": T.conv("f32", _uk("f32", 128, 128), 2, 9, 13, 16, 128),
    "uk_f32_256x128": T.conv("f32", _uk("f32", 256, 128), 1, 120, 137, 16, 1024),
}

# variant -> (scale, bias, residual: None | "slice" | "inplace", activation, cut the couts to 4 * odd)
VARIANTS = {
    "plain": (False, False, None, "none", False),
    "scale_bias": (True, True, None, "none", False),
    "bias_sigmoid": (False, True, None, "sigmoid", False),
    "scale_relu": (True, False, None, "relu", False),
    "residual": (False, False, "slice", "none", False),
    "full": (True, True, "slice", "relu", False),
    "full_sigmoid": (True, True, "slice", "sigmoid", False),
    "full_cout_4odd": (True, True, "slice", "relu", True),
    "cout_4odd_plain": (False, True, None, "none", True),
    "full_inplace": (True, True, "inplace", "relu", False),
}
# With 4 couts fewer the selectors give these families' shapes 32-cout tiles (a Cout over 128 takes 64- or 128-cout tiles only
# when they divide it): the cut variants of these families run, and name, the 32-cout instantiation of the same kernel
CUT_LABEL = {
    "pair2_tw32_bc64": "conv3x3_halo_pair2_kernel<256x32,f16x3>",
    "pair2_tw16_bc64": "conv3x3_halo_pair2_kernel<16x16x32,f16x3>",
    "uk_x3_256x128": _uk("f16x3", 256, 32),
    "uk_x3_256x64": _uk("f16x3", 256, 32),
    "uk_f16_256x128": _uk("f16", 256, 32),
    "uk_f32_256x128": _uk("f32", 256, 32),
}
CASES = [(f, v) for f in FAMILIES for v in VARIANTS
         if not (FAMILIES[f].entry.startswith("dcnv2") and VARIANTS[v][2] is not None)]


@pytest.fixture(scope="module")
def ops():
    import detectron2_centernet_amd.ops as ops

    return ops


def _gen(*key):
    import zlib

    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _round(t, mode):
    return t.half().float() if mode == "f16" else t


_FAMILY = {}


def family_data(name):
    """inputs of the family and its contraction in float64 [B, Ho, Wo, Cout] (no epilogue), computed once"""
    if name in _FAMILY:
        return _FAMILY[name]
    c = FAMILIES[name]
    Cin = sum(c.Cin) if isinstance(c.Cin, tuple) else c.Cin
    g = _gen("epilogue", name)
    t = {"Cin": Cin}
    t["x"] = _round(torch.randn(c.B, c.H, c.W, Cin, generator=g), c.mode)
    t["w"] = _round(torch.randn(c.Cout, Cin, c.k, c.k, generator=g) / (Cin * c.k * c.k) ** 0.5, c.mode)
    t["scale"] = torch.rand(c.Cout, generator=g) + 0.5
    t["bias"] = torch.randn(c.Cout, generator=g)
    x, w = t["x"].double(), t["w"].double()
    if c.entry in ("conv2d", "conv1x1_cat"):
        if (c.k, c.stride, c.pad) == (1, 1, 0):
            y = (x.reshape(-1, Cin) @ w.reshape(c.Cout, Cin).t()).reshape(c.B, c.H, c.W, c.Cout)
        else:
            y = F.conv2d(x.permute(0, 3, 1, 2), w, None, c.stride, c.pad, c.dil).permute(0, 2, 3, 1)
    else:
        xn = x.permute(0, 3, 1, 2)
        if c.entry == "dcnv2_offset":
            t["w_off"] = torch.randn(27, Cin, 3, 3, generator=g) * (1.5 / (Cin * 9) ** 0.5)
            t["b_off"] = torch.randn(27, generator=g) * 0.5
            om = F.conv2d(xn, t["w_off"].double(), t["b_off"].double(), 1, 1)
        else:
            om = torch.randn(c.B, c.H, c.W, 28, generator=g)
            om[..., :18] *= 2.0
            om[..., 27] = 0.0
            t["om"] = om
            om = om.double().permute(0, 3, 1, 2)
        y = O.dcnv2_forward(xn, om[:, :18], torch.sigmoid(om[:, 18:27]), w, None, 1, 1, 1).permute(0, 2, 3, 1)
    t["raw"] = y.contiguous()
    t["res"] = _round(torch.randn(*y.shape[:3], c.Cout, generator=g), c.mode)
    _FAMILY[name] = t
    return t


def _tol(c):
    return 3e-3 if c.mode == "f16" else 1e-5


def launch(ops, dev, c, t, cout, scale, bias, res, act, inplace=False):
    """one launch of family c on its first `cout` couts.  res: CPU tensor [B, Ho, Wo, cout] or None.
    -> (dry-run label, the whole sentinel-framed buffer [B + 1, Ho, Wo, LEFT + cout + RIGHT])"""
    L = _lib.lib()
    adt = torch.float16 if c.mode == "f16" else torch.float32
    odt = adt
    deform = c.entry.startswith("dcnv2")
    kw = {"cout_align": 64} if (deform and c.mode == "f16") else {}
    pc = ops.PackedConv(t["w"][:cout].contiguous().to(dev), t["scale"][:cout].to(dev) if scale else None,
                        t["bias"][:cout].to(dev) if bias else None, stride=c.stride, pad=c.pad, dil=c.dil,
                        compute=COMPUTE[c.mode], **kw)
    assert pc.Cout_eff == cout
    Ho, Wo = t["raw"].shape[1:3]
    full = torch.full((c.B + 1, Ho, Wo, LEFT + cout + RIGHT), SENTINEL, dtype=odt, device=dev)
    out = full[:c.B, :, :, LEFT:LEFT + cout]
    rdev = None
    if res is not None and inplace:
        out.copy_(res.to(odt).to(dev))
        rdev = out
    elif res is not None:
        rfull = torch.full((c.B, Ho, Wo, cout + 24), float("nan"), dtype=odt, device=dev)    # res_stride != out_stride
        rdev = rfull[..., 8:8 + cout]
        rdev.copy_(res.to(odt).to(dev))
    a = {"none": ops.ACT_NONE, "relu": ops.ACT_RELU, "sigmoid": ops.ACT_SIGMOID_CLAMP}[act]
    if c.entry == "conv2d":
        x = t["x"].to(adt).to(dev)

        def call():
            return ops.conv2d(x, pc, out=out, act=a, residual=rdev, clamp=CLAMP)
    elif c.entry == "conv1x1_cat":
        xs = [s.contiguous().to(adt).to(dev) for s in torch.split(t["x"], list(c.Cin), dim=3)]

        def call():
            return ops.conv1x1_cat(xs, pc, out=out, act=a, residual=rdev)
    elif c.entry == "dcnv2":
        x, om = t["x"].to(adt).to(dev), t["om"].to(dev)

        def call():
            return ops.dcnv2(x, om, pc, out=out, act=a)
    else:
        x = t["x"].to(adt).to(dev)
        po = ops.PackedConv(t["w_off"].to(dev), None, t["b_off"].to(dev), stride=1, pad=1, compute=COMPUTE[c.mode])
        assert ops.dcnv2_offset_supported(x, po, pc)

        def call():
            return ops.dcnv2_offset(x, po, pc, out=out, act=a)
    L.ctdet_set_label_mode(2)
    try:
        call()
        label = L.ctdet_last_kernel_label().decode()
    finally:
        L.ctdet_set_label_mode(0)
    call()
    torch.cuda.synchronize()
    return label, full


def expected(c, t, cout, scale, bias, res, act):
    y = t["raw"][..., :cout]
    if scale:
        y = y * t["scale"][:cout].double()
    if bias:
        y = y + t["bias"][:cout].double()
    if res is not None:
        y = y + res.double()
    if act == "relu":
        y = y.relu()
    elif act == "sigmoid":
        lo, hi = CLAMP if c.entry == "conv2d" else (0.0, 1.0)
        y = torch.sigmoid(y).clamp(lo, hi)
    return y


@pytest.mark.parametrize("family,variant", CASES, ids=[f"{f}-{v}" for f, v in CASES])
def test_epilogue_variant(ops, dev, family, variant):
    c, t = FAMILIES[family], family_data(family)
    scale, bias, resmode, act, cut = VARIANTS[variant]
    cout = c.Cout - 4 if cut else c.Cout
    assert (cout // 4) % 2 == 1 or not cut
    res = t["res"][..., :cout].contiguous() if resmode else None
    label, full = launch(ops, dev, c, t, cout, scale, bias, res, act, inplace=resmode == "inplace")
    want_label = CUT_LABEL.get(family, c.label) if cut else c.label
    assert label == want_label, f"the selector sends this shape to {label}"
    got = full[:c.B, :, :, LEFT:LEFT + cout]
    ref = expected(c, t, cout, scale, bias, res, act)
    bound = _tol(c) * max(1.0, ref.abs().max().item())
    err = (got.double().cpu() - ref).abs().max().item()
    print(f"\n{family:20s} {variant:16s} {c.label:52s} cout {cout:4d} max err {err:.3e} / bound {bound:.3e}")
    assert err <= bound, f"max err {err:.3e} > {bound:.3e}"
    assert (full[c.B] == SENTINEL).all(), "the kernel wrote past the last image"
    assert (full[:c.B, :, :, :LEFT] == SENTINEL).all() and (full[:c.B, :, :, LEFT + cout:] == SENTINEL).all(), \
        "the kernel wrote outside its channel slice"
    # the same launch again: bit-identical
    _, again = launch(ops, dev, c, t, cout, scale, bias, res, act, inplace=resmode == "inplace")
    assert torch.equal(full, again)
    if resmode == "inplace":          # exactly what the separate residual tensor gives
        _, apart = launch(ops, dev, c, t, cout, scale, bias, res, act)
        assert torch.equal(full, apart)
    if resmode and act == "relu" and got.dtype == torch.float32:
        _, plain = launch(ops, dev, c, t, cout, scale, bias, None, "none")
        want = torch.relu(plain[:c.B, :, :, LEFT:LEFT + cout] + res.to(dev))
        assert torch.equal(got, want), "residual add / ReLU differ from f32 arithmetic on the plain output"
