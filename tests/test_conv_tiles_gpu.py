"""Every forward conv kernel instantiation of conv_tile_cases.py against a float64 CPU reference of the same operation, one
launch per row.  Per row:
  * the dry-run label of the real call (real tensors, the real ops.PackedConv) is the row's label: a row that no longer reaches
    its kernel fails instead of testing another one;
  * every output element against the reference -- F.conv2d in double (a matmul for 1x1) or oracle.dcnv2_forward on doubles, then
    scale, bias, residual and ReLU in double; f16-mode inputs, weights and residual are f16-representable -- within the project's
    bounds: f16 convs 3e-3 (test_conv2d), f16 DCN 6e-3 (test_dcnv2_random_shapes), f32 and f16x3 1e-5 (TOL of
    test_f32_mfma_gpu.py), each times max(1, |ref|max);
  * write guard: the output is a view into a sentinel-filled buffer with one more image and 8 more channels per pixel, and no
    sentinel changes (a ragged last pixel tile, a padded cout tile or a surplus workgroup of the rounded-up grid that stores);
  * read guard: the input (every source of a concat) is the first B images of a buffer whose image B is NaN, and no NaN reaches
    the output.
The rows that also write the sampled columns (ops.dcnv2(want_cols=True)) compare them with the oracle's columns in double and
with the columns the 64-cout row of the same mode wrote for the same input, both within the f32 bound above (the columns are f32
blends of four f32 samples: a few ulp).  One line per row is printed: label, shape, measured maximum error / bound."""
import zlib

import pytest
import torch
import torch.nn.functional as F

from conv_tile_cases import ROWS, case_id
from detectron2_centernet_amd import _lib
from oracle import ctdet_oracle as O

pytestmark = pytest.mark.gpu

COMPUTE = {"f16": _lib.F16, "f32": _lib.F32, "f16x3": _lib.F16X3}
TDT = {"f16": torch.float16, "f32": torch.float32}
SENTINEL = -1234.0          # exact in f16
GUARD_CHANNELS = 8


@pytest.fixture(scope="module")
def ops():
    import detectron2_centernet_amd.ops as ops

    return ops


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _round(t, mode):
    return t.half().float() if mode == "f16" else t


def _tol(c):
    if c.mode != "f16":
        return 1e-5
    return 6e-3 if c.entry.startswith("dcnv2") else 3e-3


def make_inputs(c):
    """CPU tensors of row c (NHWC activations, OIHW weights).  The activations depend on the mode and the input geometry only, so
    the three dcnv2_cols rows of a mode read one input"""
    Cin = sum(c.Cin) if isinstance(c.Cin, tuple) else c.Cin
    Ho = (c.H + 2 * c.pad - (c.dil * (c.k - 1) + 1)) // c.stride + 1
    Wo = (c.W + 2 * c.pad - (c.dil * (c.k - 1) + 1)) // c.stride + 1
    gx = _gen("x", c.mode, c.B, c.H, c.W, Cin, c.k)
    t = {"Cin": Cin, "Ho": Ho, "Wo": Wo, "Cout_eff": (c.Cout + 3) // 4 * 4}
    t["x"] = _round(torch.randn(c.B, c.H, c.W, Cin, generator=gx), c.mode)
    if c.entry in ("dcnv2", "dcnv2_cols"):
        om = torch.randn(c.B, c.H, c.W, 28, generator=gx)
        om[..., :18] *= 2.0                     # samples inside and outside the +-4 px LDS window and the image
        om[..., 27] = 0.0
        om[:, 0, 0, 0], om[:, 0, 0, 1], om[:, -1, -1, 2] = -0.0, -1.0, 1.0     # exactly on integer / border coordinates
        t["om"] = om
    g = _gen("w", *[sorted(v) if isinstance(v, frozenset) else v for v in c[:-1]])
    t["w"] = _round(torch.randn(c.Cout, Cin, c.k, c.k, generator=g) / (Cin * c.k * c.k) ** 0.5, c.mode)
    t["scale"] = torch.rand(c.Cout, generator=g) + 0.5
    t["bias"] = torch.randn(c.Cout, generator=g)
    if "residual" in c.epilogue:
        t["res"] = _round(torch.randn(c.B, Ho, Wo, t["Cout_eff"], generator=g), c.mode)
    if c.entry == "dcnv2_offset":
        t["w_off"] = _round(torch.randn(27, Cin, 3, 3, generator=g) * (1.5 / (Cin * 9) ** 0.5), c.mode)
        t["b_off"] = torch.randn(27, generator=g) * 0.5
    return t


def reference(c, t):
    """float64 NHWC output [B, Ho, Wo, Cout_eff] (padded couts: zero weights, scale 1, bias 0) and, for the DCN rows, the columns"""
    x = t["x"].double()
    w = t["w"].double()
    cols = None
    if c.entry in ("conv2d", "conv1x1_cat"):
        if (c.k, c.stride, c.pad) == (1, 1, 0):
            y = x.reshape(-1, t["Cin"]) @ w.reshape(c.Cout, t["Cin"]).t()
            y = y.reshape(c.B, c.H, c.W, c.Cout)
        else:
            y = F.conv2d(x.permute(0, 3, 1, 2), w, None, c.stride, c.pad, c.dil).permute(0, 2, 3, 1)
    else:
        xn = x.permute(0, 3, 1, 2)
        if c.entry == "dcnv2_offset":
            om = F.conv2d(xn, t["w_off"].double(), t["b_off"].double(), 1, 1)
        else:
            om = t["om"].double().permute(0, 3, 1, 2)
        off, mask = om[:, :18], torch.sigmoid(om[:, 18:27])
        y = O.dcnv2_forward(xn, off, mask, w, None, 1, 1, 1).permute(0, 2, 3, 1)
        if c.entry == "dcnv2_cols":
            cols = O.dcnv2_columns(xn, off, mask, 3, 3, 1, 1, 1)[0]                    # [B, C, 9, P]
            cols = cols.permute(0, 3, 2, 1).reshape(c.B, c.H, c.W, 9 * t["Cin"])       # the kernel's [tap][channel] order
    y = y * t["scale"].double() + t["bias"].double()
    y = F.pad(y, (0, t["Cout_eff"] - c.Cout))
    if "res" in t:
        y = y + t["res"].double()
    if "relu" in c.epilogue:
        y = y.relu()
    return y.contiguous(), cols


def _guarded_input(x, dtype, dev):
    """x as the first B images of a device buffer whose image B is NaN"""
    buf = torch.full((x.shape[0] + 1,) + tuple(x.shape[1:]), float("nan"), dtype=dtype)
    buf[:-1] = x.to(dtype)
    return buf.to(dev)[:-1]


def run(ops, dev, c, t):
    """(label of the dry run, guarded output buffer [B + 1, Ho, Wo, Cout_eff + 8], columns or None)"""
    L = _lib.lib()
    compute, adt, odt = COMPUTE[c.mode], TDT["f16" if c.mode == "f16" else "f32"], TDT[c.out_dtype]
    deform = c.entry.startswith("dcnv2")
    kw = {"cout_align": 64} if (deform and c.mode == "f16") else {}
    pc = ops.PackedConv(t["w"].to(dev), t["scale"].to(dev), t["bias"].to(dev), stride=c.stride, pad=c.pad, dil=c.dil, compute=compute, **kw)
    assert pc.Cout_eff == t["Cout_eff"]
    if isinstance(c.Cin, tuple):
        xs = [_guarded_input(s, adt, dev) for s in torch.split(t["x"], list(c.Cin), dim=3)]
    else:
        x = _guarded_input(t["x"], adt, dev)
    res = t["res"].to(odt).to(dev) if "res" in t else None
    act = ops.ACT_RELU if "relu" in c.epilogue else ops.ACT_NONE
    full = torch.full((c.B + 1, t["Ho"], t["Wo"], pc.Cout_eff + GUARD_CHANNELS), SENTINEL, dtype=odt, device=dev)
    out = full[:c.B, :, :, :pc.Cout_eff]
    if c.entry == "conv2d":
        def call():
            return ops.conv2d(x, pc, out=out, act=act, residual=res)
    elif c.entry == "conv1x1_cat":
        def call():
            return ops.conv1x1_cat(xs, pc, out=out, act=act, residual=res)
    elif c.entry in ("dcnv2", "dcnv2_cols"):
        om = t["om"].to(dev)

        def call():
            return ops.dcnv2(x, om, pc, out=out, act=act, want_cols=c.entry == "dcnv2_cols")
    else:
        po = ops.PackedConv(t["w_off"].to(dev), None, t["b_off"].to(dev), stride=1, pad=1, compute=compute)
        assert ops.dcnv2_offset_supported(x, po, pc)

        def call():
            return ops.dcnv2_offset(x, po, pc, out=out, act=act)
    L.ctdet_set_label_mode(2)
    try:
        call()                                  # checks and selection only: nothing is launched
        label = L.ctdet_last_kernel_label().decode()
    finally:
        L.ctdet_set_label_mode(0)
    got = call()
    torch.cuda.synchronize()
    cols = None
    if c.entry == "dcnv2_cols":
        got, cols = got
        assert cols is not None, "the layer is not served by the kernel that writes the columns"
    assert got.data_ptr() == full.data_ptr()
    return label, full, cols


_COLS64 = {}        # (mode, input geometry) -> the columns the 64-cout dcnv2_cols row wrote


def _cols_of_the_64_cout_row(ops, dev, c):
    key = (c.mode, c.B, c.H, c.W, c.Cin)
    if key not in _COLS64:
        c64 = [r for r in ROWS if r.entry == "dcnv2_cols" and r.Cout == 64 and (r.mode, r.B, r.H, r.W, r.Cin) == key]
        assert len(c64) == 1, key
        _COLS64[key] = run(ops, dev, c64[0], make_inputs(c64[0]))[2].cpu()
    return _COLS64[key]


@pytest.mark.parametrize("c", ROWS, ids=[case_id(c) for c in ROWS])
def test_row_against_float64(ops, dev, c):
    t = make_inputs(c)
    ref, ref_cols = reference(c, t)
    label, full, cols = run(ops, dev, c, t)
    assert label == c.label, f"the selector sends this shape to {label}"
    full = full.cpu()
    Ce = t["Cout_eff"]
    got = full[:c.B, :, :, :Ce].double()
    bound = _tol(c) * max(1.0, ref.abs().max().item())
    diff = (got - ref).abs()
    err = diff.max().item()
    where = ""
    if not err <= bound:
        b, ho, wo, n = [int(v) for v in torch.unravel_index(torch.nan_to_num(diff, nan=float("inf")).argmax(), diff.shape)]
        m = (b * t["Ho"] + ho) * t["Wo"] + wo
        where = f" worst at image {b} pixel ({ho}, {wo}) = m {m} (256-pixel tile {m // 256}, row {m % 256}) cout {n}; " \
                f"{int((diff > bound).sum())} elements over the bound"
    cin = "+".join(map(str, c.Cin)) if isinstance(c.Cin, tuple) else c.Cin
    print(f"\n{c.label:52s} {c.mode:5s} {c.entry:12s} {c.B}x{c.H}x{c.W} {cin}->{c.Cout} k{c.k}/s{c.stride}/p{c.pad} out {c.out_dtype} "
          f"{'+'.join(sorted(c.epilogue - {'scale_bias'})) or '-':13s} max err {err:.3e} / bound {bound:.3e} = {err / bound:.3f}")
    assert not torch.isnan(got).any(), "a NaN of the guard image after the input reached the output"
    assert err <= bound, f"max err {err:.3e} > {bound:.3e};{where}"
    assert (full[c.B] == SENTINEL).all(), "the kernel wrote past the last image"
    assert (full[:c.B, :, :, Ce:] == SENTINEL).all(), "the kernel wrote past the last cout of a pixel"
    if c.entry == "dcnv2_cols":
        cols = cols.cpu()
        cb = 1e-5 * max(1.0, ref_cols.abs().max().item())
        e_ref = (cols.double() - ref_cols).abs().max().item()
        e_64 = (cols - _cols_of_the_64_cout_row(ops, dev, c)).abs().max().item()
        print(f"    columns: vs float64 {e_ref:.3e}, vs the 64-cout row's {e_64:.3e} / bound {cb:.3e}")
        assert e_ref <= cb and e_64 <= cb, (e_ref, e_64, cb)
