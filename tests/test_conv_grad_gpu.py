"""Every row of conv_grad_cases.py on the GPU against the float64 references of that module (shifted-view matmuls in double on
the device, no MIOpen), one launch per row.  Per row:
  * label: the dry-run label of the real call (real tensors, ops_train.conv_wgrad / conv_dgrad; ConvTransposeFn: the labels its
    three launches record) is the row's label, split included: a row that no longer reaches its kernel fails instead of testing
    another one;
  * dense: every element of dW / dX against float64, relative to max(1, |ref|max).  Bounds of the project's own tests: f16 dW
    3e-3, dX 4e-3 (test_train_gpu.py); f16x3 2e-5, accumulating into an OIHW slot 3e-5 (test_train_x3_gpu.py); f32 2e-5 (what
    test_dcn_boundary_gpu.py allows the same weight-gradient kernel); the conv-transpose forward at the forward bounds of
    test_conv_tiles_gpu.py (f16 3e-3, f32 / f16x3 1e-5).  f16-mode operands are f16-representable;
  * impulse (weight-gradient rows): x on a 1/64 grid (f16-representable, so the lo halves of the f16x3 split are zero), dY zero
    except that cout channel n is 1.0 at the n-th pixel of the row's seam list (conv_grad_cases.seam_pixels: image corners,
    range and K-step boundaries from the label's split, tile corners).  Row n of dW is then exactly the zero-padded patch of x
    around that pixel, one term per element: torch.equal in all three modes.  A pixel dropped, read twice or taken from the
    neighbouring range or tile shows at full magnitude (in the dense check it is 1 / sqrt(M));
  * read guard: x and dY are the first B images of buffers whose image B is NaN; the channel slices of the wgrad_oihw rows have
    NaN channels on both sides;
  * write guard: dW (handed out by a stand-in for ops_train.ARENA, or the OIHW slot) and dX are views into sentinel-filled buffers
    and no sentinel changes; an OIHW slot has no room for the dropped padded channels, so a write of one lands on a neighbour or
    a sentinel and fails one of the checks.
ConvTransposeFn allocates its outputs itself: its rows have the read guard only.  Its weight gradient comes back multiplied by
ops_train.PARAM_GRAD_MULT (a power of two), which the comparison divides out.
One line per row is printed: label, shape, measured maximum error / bound."""
import zlib

import pytest
import torch

import conv_grad_cases as G
from conv_grad_cases import ROWS, case_id, out_hw
from detectron2_centernet_amd import _lib

pytestmark = pytest.mark.gpu

COMPUTE = {"f16": _lib.F16, "f32": _lib.F32, "f16x3": _lib.F16X3}
SENTINEL = -1234.0
PAD = 64                 # sentinel floats on either side of a dW buffer
SLICE_EXTRA = 16         # NaN channels around the channel slices of the wgrad_oihw rows (8 in front: 16-byte aligned in f16)
SLICE_OFF = 8
NAN = float("nan")
DW_TOL = {"f16": 3e-3, "f16x3": 2e-5, "f32": 2e-5}
DW_TOL_OIHW = {"f16": 3e-3, "f16x3": 3e-5, "f32": 2e-5}
DX_TOL = {"f16": 4e-3, "f16x3": 2e-5, "f32": 2e-5}
FWD_TOL = {"f16": 3e-3, "f16x3": 1e-5, "f32": 1e-5}

WGRAD = [c for c in ROWS if c.op in ("wgrad", "wgrad_oihw")]
DGRAD = [c for c in ROWS if c.op == "dgrad"]
CONVT = [c for c in ROWS if c.op == "convT"]


@pytest.fixture(scope="module")
def T():
    import detectron2_centernet_amd.ops as ops
    import detectron2_centernet_amd.ops_train as ot

    return ops, ot


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _adt(mode):
    return torch.float16 if mode == "f16" else torch.float32


def _rand(shape, mode, g, scale=1.0):
    t = torch.randn(*shape, generator=g) * scale
    return t.half().float() if mode == "f16" else t


def _grid(shape, g):
    return torch.randint(-256, 257, shape, generator=g).float() / 64.0


def _guarded(t, dtype, dev, sliced=False):
    """t [B, H, W, C] as the first B images of a device buffer whose image B is NaN; sliced: as channels 8 .. 8 + C of a buffer with
    16 more channels per pixel, NaN too"""
    B, H, W, Cc = t.shape
    extra, off = (SLICE_EXTRA, SLICE_OFF) if sliced else (0, 0)
    buf = torch.full((B + 1, H, W, Cc + extra), NAN, dtype=dtype)
    buf[:B, :, :, off:off + Cc] = t.to(dtype)
    return buf.to(dev)[:B, :, :, off:off + Cc]


def _dry_label(call):
    L = _lib.lib()
    L.ctdet_set_label_mode(2)
    try:
        call()                                   # checks and selection only: the labelled kernel is not launched
        return L.ctdet_last_kernel_label().decode()
    finally:
        L.ctdet_set_label_mode(0)


def _shape(c):
    geo = f"k{c.k}/s{c.stride}/p{c.pad}" + (f"/d{c.dil}" if c.dil > 1 else "")
    return f"{c.mode:5s} {c.op:10s} {c.B}x{c.H}x{c.W} {c.Cin}({c.cin_c})->{c.Cout}({c.cout_c}) {geo}"


def _check(what, got, ref, tol):
    """(max error, bound) after printing them; NaN counts as an infinite error"""
    bound = tol * max(1.0, ref.abs().max().item())
    err = torch.nan_to_num((got.double() - ref).abs(), nan=float("inf")).max().item()
    print(f"    {what}: max err {err:.3e} / bound {bound:.3e} = {err / bound:.3f}")
    return err, bound


class GuardArena:
    """stands in for ops_train.ARENA (the step's zeroed arena): hands conv_wgrad a zeroed slice between two runs of sentinels"""

    def __init__(self, dev):
        self.buf = torch.empty(1, dtype=torch.float32, device=dev)

    def take(self, numel):
        self.buf = torch.full((numel + 2 * PAD,), SENTINEL, dtype=torch.float32, device=self.buf.device)
        self.buf[PAD:PAD + numel] = 0.0
        return self.buf[PAD:PAD + numel]

    def sentinels_intact(self):
        return bool((self.buf[:PAD] == SENTINEL).all() and (self.buf[-PAD:] == SENTINEL).all())


def _wgrad_call(T, c, x, dy, slot, arena, monkeypatch):
    """the row's weight-gradient call on device tensors: a function that returns dW [Cout, k, k, C] (plain) or the slot"""
    ops, ot = T
    comp = COMPUTE[c.mode]
    monkeypatch.setattr(ot, "ARENA", arena)
    if c.op == "wgrad":
        def call():
            dw = ot.conv_wgrad(x, dy, c.Cout, c.k, c.k, c.stride, c.pad, dil=c.dil, scale=1.0, comp=comp)
            assert dw.data_ptr() == arena.buf.data_ptr() + 4 * PAD
            return dw.view(c.Cout, c.k, c.k, c.cin_c)
    else:
        def call():
            ot.conv_wgrad(x, dy, c.cout_c, c.k, c.k, c.stride, c.pad, dil=c.dil, scale=0.5, into=(slot, c.k * c.k, c.cin_c), comp=comp)
            return slot
    return call


def _slot(c, values, dev):
    """an OIHW gradient slot [Cout, Cin, k, k] holding `values`, between two runs of sentinels"""
    n = values.numel()
    buf = torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.float32, device=dev)
    buf[PAD:PAD + n] = values.reshape(-1).to(dev)
    return buf, buf[PAD:PAD + n].view(c.Cout, c.Cin, c.k, c.k)


@pytest.mark.parametrize("c", WGRAD, ids=[case_id(c) for c in WGRAD])
def test_weight_gradient_row(T, dev, c, monkeypatch):
    Ho, Wo = out_hw(c)
    sliced = c.op == "wgrad_oihw"
    adt = _adt(c.mode)
    g = _gen("wgrad", *c[:13])
    x = _rand((c.B, c.H, c.W, c.cin_c), c.mode, g)              # carried channels hold data: they must be dropped, not trusted
    dy = _rand((c.B, Ho, Wo, c.cout_c), c.mode, g)
    xd, dyd = _guarded(x, adt, dev, sliced), _guarded(dy, adt, dev, sliced)
    arena = GuardArena(dev)
    slot0 = sbuf = slot = None
    if sliced:
        slot0 = torch.randn(c.Cout, c.Cin, c.k, c.k, generator=g)
        sbuf, slot = _slot(c, slot0, dev)
    call = _wgrad_call(T, c, xd, dyd, slot, arena, monkeypatch)
    label = _dry_label(call)
    print(f"\n{label:52s} {_shape(c)} M={c.B * Ho * Wo}")
    assert label == c.label, f"the launcher sends this shape to {label}"
    if sliced:
        assert torch.equal(slot.cpu(), slot0), "the dry run launched"
    got = call()
    torch.cuda.synchronize()
    ref = G.wgrad_ref(x.to(dev), dy[..., :c.Cout].to(dev), c.k, c.stride, c.pad, c.dil)
    if sliced:
        ref = slot0.to(dev).double() + 0.5 * ref[..., :c.Cin].permute(0, 3, 1, 2)
    err, bound = _check("dense dW", got, ref, (DW_TOL_OIHW if sliced else DW_TOL)[c.mode])
    assert err <= bound, f"max err {err:.3e} > {bound:.3e}"
    assert sliced or arena.sentinels_intact(), "the kernel wrote outside dW"
    assert not sliced or bool((sbuf[:PAD] == SENTINEL).all() and (sbuf[-PAD:] == SENTINEL).all()), "the kernel wrote outside the slot"

    # ---- impulses at the seams, Cout pixels per launch
    seams = G.seam_pixels(c)
    xi = _grid((c.B, c.H, c.W, c.cin_c), g)
    xid = _guarded(xi, adt, dev, sliced)
    dyz = _guarded(torch.zeros(c.B, Ho, Wo, c.cout_c), adt, dev, sliced)
    s0 = _grid((c.Cout, c.Cin, c.k, c.k), g) * 8.0 if sliced else None          # a 1/8 grid: slot + 0.5 * x is exact
    launches = 0
    for i0 in range(0, len(seams), c.Cout):
        px = seams[i0:i0 + c.Cout]
        m = torch.tensor(px, device=dev)
        idx = (m // (Ho * Wo), m // Wo % Ho, m % Wo, torch.arange(len(px), device=dev))
        dyz.zero_()
        dyz[idx] = 1.0
        if sliced:
            sbuf, slot = _slot(c, s0, dev)
        got = _wgrad_call(T, c, xid, dyz, slot, arena, monkeypatch)()
        torch.cuda.synchronize()
        launches += 1
        patches = G.impulse_patches(xi, c, px)                                  # [n, k, k, cin_c]
        if sliced:
            want = s0.clone()
            want[:len(px)] += 0.5 * patches[..., :c.Cin].permute(0, 3, 1, 2)
            ok_guard = bool((sbuf[:PAD] == SENTINEL).all() and (sbuf[-PAD:] == SENTINEL).all())
        else:
            want = torch.zeros(c.Cout, c.k, c.k, c.cin_c)
            want[:len(px)] = patches
            ok_guard = arena.sentinels_intact()
        got = got.cpu()
        if not torch.equal(got, want):
            bad = (got != want) | torch.isnan(got)
            n = int(bad.reshape(c.Cout, -1).any(1).nonzero()[0])
            pytest.fail(f"impulse launch {launches}: dW row {n} (impulse at pixel {px[n] if n < len(px) else None}) is not the patch "
                        f"of x around it; {int(bad.sum())} elements differ, largest difference "
                        f"{torch.nan_to_num((got - want).abs(), nan=float('inf')).max().item():.3e}")
        assert ok_guard, "the kernel wrote outside dW"
    print(f"    impulse: {len(seams)} seam pixels in {launches} launches, exact")


@pytest.mark.parametrize("c", DGRAD, ids=[case_id(c) for c in DGRAD])
def test_input_gradient_row(T, dev, c):
    ops, ot = T
    Ho, Wo = out_hw(c)
    adt = _adt(c.mode)
    g = _gen("dgrad", *c[:13])
    dy = _rand((c.B, Ho, Wo, c.cout_c), c.mode, g)
    dy[..., c.Cout:] = 0.0                                       # carried channels of dY are zero by the layers' contract
    w = _rand((c.Cout, c.Cin, c.k, c.k), c.mode, g, 1.0 / (c.Cout * c.k * c.k) ** 0.5).to(dev)
    dyd = _guarded(dy, adt, dev)
    full = torch.full((c.B + 1, c.H, c.W, c.Cin + 8), SENTINEL, dtype=adt, device=dev)
    out = full[:c.B, :, :, :c.Cin]

    def call():
        return ot.conv_dgrad(dyd, w, c.stride, c.pad, (c.H, c.W), cin_pad=c.cout_c if c.cout_c != c.Cout else None,
                             comp=COMPUTE[c.mode], out=out)
    label = _dry_label(call)
    print(f"\n{label:52s} {_shape(c)}")
    got = call()
    torch.cuda.synchronize()
    assert got.data_ptr() == full.data_ptr() and tuple(got.shape) == (c.B, c.H, c.W, c.Cin)
    ref = G.dgrad_ref(dy[..., :c.Cout].to(dev), w, c.stride, c.pad, c.H, c.W)
    err, bound = _check("dense dX", got, ref, DX_TOL[c.mode])
    assert label == c.label, f"the launcher sends this shape to {label}"
    assert err <= bound, f"max err {err:.3e} > {bound:.3e}"
    assert bool((full[c.B] == SENTINEL).all()), "the kernel wrote past the last image"
    assert bool((full[:c.B, :, :, c.Cin:] == SENTINEL).all()), "the kernel wrote past the last channel of a pixel"


@pytest.mark.parametrize("c", CONVT, ids=[case_id(c) for c in CONVT])
def test_conv_transpose_row(T, dev, c, monkeypatch):
    ops, ot = T
    L = _lib.lib()
    adt = _adt(c.mode)
    g = _gen("convT", *c[:13])
    Ho, Wo = (c.H - 1) * c.stride - 2 * c.pad + c.k, (c.W - 1) * c.stride - 2 * c.pad + c.k
    x = _rand((c.B, c.H, c.W, c.Cin), c.mode, g)
    w = _rand((c.Cin, c.Cout, c.k, c.k), c.mode, g, 1.0 / (c.Cin * c.k * c.k / c.stride ** 2) ** 0.5)
    dy = _rand((c.B, Ho, Wo, c.Cout), c.mode, g)
    labels = []

    def logged(fn):
        def wrapper(*a, **kw):                   # the label state is per thread, and backward runs on autograd's thread
            L.ctdet_set_label_mode(1)            # record: the launcher names its kernel, then launches it
            try:
                r = fn(*a, **kw)
                labels.append(L.ctdet_last_kernel_label().decode())
            finally:
                L.ctdet_set_label_mode(0)
            return r
        return wrapper
    monkeypatch.setattr(ops, "conv2d", logged(ops.conv2d))
    monkeypatch.setattr(ot, "conv_wgrad", logged(ot.conv_wgrad))
    monkeypatch.setattr(ot, "F32_COMPUTE", COMPUTE[c.mode] if c.mode != "f16" else ot.F32_COMPUTE)
    xd = _guarded(x, adt, dev).requires_grad_()
    wd = w.to(dev).requires_grad_()
    y = ot.ConvTransposeFn.apply(xd, wd, c.stride, c.pad)
    dx, dw = torch.autograd.grad(y, (xd, wd), dy.to(adt).to(dev))
    torch.cuda.synchronize()
    print(f"\n{' | '.join(labels)}\n    {_shape(c)}")
    assert tuple(y.shape) == (c.B, Ho, Wo, c.Cout) and tuple(dx.shape) == x.shape and tuple(dw.shape) == w.shape
    ry, rdx, rdw = G.conv_transpose_refs(x.to(dev), w.to(dev), dy.to(dev), c.stride, c.pad)
    res = [_check("forward", y.detach(), ry, FWD_TOL[c.mode]), _check("dense dX", dx, rdx, DX_TOL[c.mode]),
           _check("dense dW", dw / ot.PARAM_GRAD_MULT, rdw, DW_TOL[c.mode])]
    assert tuple(labels) == tuple(c.label), f"the launchers send this shape to {labels}"
    for err, bound in res:
        assert err <= bound, f"max err {err:.3e} > {bound:.3e}"
