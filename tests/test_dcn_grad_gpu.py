"""Every row of dcn_grad_cases.py on the GPU against the float64 references of that module, one launch per check.  Per row:
  * label: the dry-run label of the real call (real tensors, ops_train.dcn_cols / dcn_col2im_coord / dcn_col2im_fused) is the
    row's label -- taps per workgroup, element type, fused or not, mask or no mask -- and the dry run wrote nothing;
  * dense: every element of cols / dx / dom against float64 on the operands as the kernel reads them, relative to
    max(1, |ref|max).  Bounds of the project's own tests: cols f16 4e-3 (test_dcn_cols_from_lds_window), f32 1e-5
    (test_dcn_forward_writes_the_columns); dx f16 8e-3 and f32 2e-5, dom four times that (test_dcn_boundary_gpu.py); f16x3 1e-4
    (test_dcn_training_fwd_bwd_x3).  Rows with two 32-channel chunks: dx per chunk against that chunk's own |ref|max (no floor
    of 1), so the chunk scaled by 2^-10 does not hide behind the one scaled by 2^10;
  * exact (cols and col2im rows): a second run on the permutation geometry (offsets from {-9, -5, -4, -1, -0.0, 0.5, 4, 5, 9},
    mask 1 through the PROB or NONE mode, x and dcol on the 1/64 grid with |v| <= 4).  Every bilinear weight is 0, 1/4, 1/2 or 1,
    every product a multiple of 2^-14 and every partial sum of the seeded data far below 2^10: all sums are exact in f32 in any
    order, in the window kernels' fixed point too (quantum <= 2^-16 of multiples of 2^-8), and the columns are exact in f16
    (multiples of 2^-8 below 4).  All outputs are exact: dx (always f32), cols and dom are torch.equal to the float64 reference
    cast to the output type (the f16 dom is the exact f32 value rounded once, like the cast of the reference).  A contribution
    dropped, doubled or taken from the neighbouring tile, image or tap shows at full magnitude;
  * zero outside: the dom entries of every sample outside the image (exactly on -1, exactly on H / W, far outside) are exactly
    0.0, and those samples add nothing to dx: the row runs once more with the dcol columns of exactly those (pixel, tap) pairs
    set to 1e4 (col2im rows; the fused rows have no dcol to replace).  On the permutation geometry, where no sum depends on its
    order, dx must stay bit for bit the same in every kernel.  On the row's own geometry dx is a sum of f32 atomics whose order
    changes from launch to launch in every kernel here (the generic kernels add every term with one, the window kernels the
    windows of neighbouring tiles and the out-of-window samples; measured on an MI355X: two launches on identical inputs differ
    in 50 to 75 % of the elements of the generic rows, by up to 1.9e-6, and in 35 to 68 of the 540672 elements of the 9-tap
    window rows, by up to 4.8e-7), so dx is not reproducible bit for bit even between identical calls: on the generic kernels
    and the 9-tap window kernel the change must stay within what another order of the same terms can do, 2 n 2^-24 S per element
    (n terms of absolute sum S, both counted by the float64 reference), on the tap-split window kernels within the dense bound;
  * read guard: x, dcol / dY and om are the first B images of buffers whose image B is NaN; x is a channel slice with NaN
    channels on both sides; om's padding channels (27.. / 18..) are NaN;
  * write guard: cols, dx and dom are views into sentinel-filled buffers and no sentinel changes; dom is NaN before the call,
    afterwards every entry below 27 (18) is finite and every padding channel exactly 0.
One line per row is printed: label, shape, measured maximum error / bound of every output."""
import pytest
import torch

import dcn_grad_cases as G
from dcn_grad_cases import MASK_MODE, ROWS, case_id
from detectron2_centernet_amd import _lib

pytestmark = pytest.mark.gpu

COMPUTE = {"f16": _lib.F16, "f32": _lib.F32, "f16x3": _lib.F16X3}
SENTINEL = -1234.0
PAD = 64                 # sentinel elements on either side of an output
SLICE_EXTRA, SLICE_OFF = 16, 8
OM_STRIDE = 32
NAN = float("nan")
COLS_TOL = {"f16": 4e-3, "f32": 1e-5}
DX_TOL = {"f16": 8e-3, "f32": 2e-5, "f16x3": 1e-4}
DOM_TOL = {"f16": 4 * 8e-3, "f32": 4 * 2e-5, "f16x3": 1e-4}


@pytest.fixture(scope="module")
def ot():
    import detectron2_centernet_amd.ops_train as ot

    return ot


def _adt(c):
    return torch.float16 if c.mode == "f16" else torch.float32


def _guarded(t, dtype, dev, sliced=False, width=None, stride=None):
    """t [B, H, W, C] as the first B images of a device buffer whose image B is NaN.  sliced: as channels 8 .. 8 + C of a buffer
    with 16 more NaN channels per pixel; stride / width: as the first C channels of `stride` per pixel (the rest NaN), the view
    `width` channels wide"""
    B, H, W, Cc = t.shape
    extra, off = (SLICE_EXTRA, SLICE_OFF) if sliced else ((stride - Cc, 0) if stride else (0, 0))
    buf = torch.full((B + 1, H, W, Cc + extra), NAN, dtype=dtype)
    buf[:B, :, :, off:off + Cc] = t.to(dtype)
    return buf.to(dev)[:B, :, :, off:off + (width or Cc)]


def _out(shape, dtype, dev, fill):
    """(buffer, view of `shape` filled with `fill` between two runs of PAD sentinels)"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * PAD,), SENTINEL, dtype=dtype, device=dev)
    buf[PAD:PAD + n] = fill
    return buf, buf[PAD:PAD + n].view(*shape)


def _intact(buf):
    return bool((buf[:PAD] == SENTINEL).all() and (buf[-PAD:] == SENTINEL).all())


def _dry_label(call):
    L = _lib.lib()
    L.ctdet_set_label_mode(2)
    try:
        call()
        return L.ctdet_last_kernel_label().decode()
    finally:
        L.ctdet_set_label_mode(0)


def _err(got, ref):
    return torch.nan_to_num((got.double() - ref).abs(), nan=float("inf")).max().item()


def _check(what, got, ref, tol, floor=1.0):
    bound = tol * max(floor, ref.abs().max().item())
    err = _err(got, ref)
    print(f"    {what}: max err {err:.3e} / bound {bound:.3e} = {err / bound:.3f}")
    return what, err, bound


def _batch(c):
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    B = G.batch_of(c, ncu)
    if B is None:
        pytest.skip(f"no batch selects {c.nt} taps per workgroup on {ncu} compute units")
    return B


class Run:
    """one call of a row on guarded tensors"""

    def __init__(self, ot, c, B, dev, d, om, mask_mode):
        self.c = c
        adt = _adt(c)
        omc = G.om_channels(c)
        dom_f32_of_om = c.op == "col2im" and c.mode == "f16" and c.dom_c != 32        # dom_channels=None: om's shape, f32
        self.x = _guarded(d["x"], adt, dev, sliced=True)
        self.om = _guarded(om, torch.float32, dev, stride=OM_STRIDE, width=c.dom_c if dom_f32_of_om else omc)
        shape = (B, c.H, c.W)
        if c.op == "cols":
            self.bufs = [_out(shape + (9 * c.Cin,), adt, dev, NAN)]
            self.call = lambda: ot.dcn_cols(self.x, self.om, mask_is_prob=mask_mode, out=self.bufs[0][1])
            return
        dom_dt = torch.float16 if c.mode == "f16" and c.dom_c == 32 else torch.float32
        self.bufs = [_out(shape + (c.Cin,), torch.float32, dev, 0.0), _out(shape + (c.dom_c,), dom_dt, dev, NAN)]
        out = (self.bufs[0][1], self.bufs[1][1])
        dom_channels = None if dom_f32_of_om else c.dom_c
        if c.op == "col2im":
            self.dcol = _guarded(d["dcol"], adt, dev)
            self.call = lambda: ot.dcn_col2im_coord(self.dcol, self.x, self.om, mask_mode, dom_channels, c.chunked,
                                                    comp=COMPUTE[c.mode], out=out)
        else:
            self.dy = _guarded(d["dy"], torch.float32, dev)
            w = d["weight"].to(dev)
            self.call = lambda: ot.dcn_col2im_fused(self.dy, w, self.x, self.om, mask_mode, dom_channels=c.dom_c, out=out)

    def __call__(self):
        r = self.call()
        torch.cuda.synchronize()
        assert r is not None, "the fused launcher refused the shape"
        assert all(_intact(b) for b, _ in self.bufs), "the kernel wrote outside its output"
        return r

    def check_dom_form(self, dom):
        omc = G.om_channels(self.c)
        assert bool(torch.isfinite(dom[..., :omc]).all()), "dom: an entry was not written (or is not finite)"
        assert bool((dom[..., omc:] == 0).all()), "dom: the padding channels are not all exactly 0"


def _shape(c, B):
    return f"{c.mode:5s} {c.op:12s} {B}x{c.H}x{c.W}x{c.Cin}" + (f"->{c.Cout}" if c.Cout else "") + f" {c.mask}" + \
        (f" dom{c.dom_c}" if c.dom_c else "") + (" chunked" if c.chunked else "")


def _outside_dom_is_zero(c, dom, outside):
    for t in range(9):
        o = outside[..., t]
        chans = [2 * t, 2 * t + 1] + ([18 + t] if c.mask != "none" else [])
        for ch in chans:
            v = dom[..., ch][o]
            assert bool((v == 0).all()), f"dom channel {ch}: a sample outside the image has a gradient of {v.abs().max().item():.3e}"


COLS = [c for c in ROWS if c.op == "cols"]
GRAD = [c for c in ROWS if c.op != "cols"]


@pytest.mark.parametrize("c", COLS, ids=[case_id(c) for c in COLS])
def test_columns_row(ot, dev, c):
    B = _batch(c)
    mm = MASK_MODE[c.mask]
    om, _ = G.geometry(c, B)
    d = G.operands(c, B)
    run = Run(ot, c, B, dev, d, om, mm)
    label = _dry_label(run.call)
    print(f"\n{label:60s} {_shape(c, B)}")
    assert label == c.label, f"the launcher sends this shape to {label}"
    assert bool(torch.isnan(run.bufs[0][1]).all()), "the dry run launched"
    col = run()
    ref = G.cols_ref(d["x"], om, mm).to(dev)
    _, err, bound = _check("dense cols", col, ref, COLS_TOL[c.mode])
    assert err <= bound, f"cols: max err {err:.3e} > {bound:.3e}"
    outside = G.classify(c, om)["outside"].to(dev)
    z = col.view(B, c.H, c.W, 9, c.Cin)[outside]
    assert bool((z == 0).all()), "a sample outside the image has a non-zero column"
    # ---- exact: permutation geometry, mask 1
    pm = 2 if c.mask == "none" else 1
    pom, pd = G.perm_geometry(c, B), G.operands(c, B, exact=True)
    run = Run(ot, c, B, dev, pd, pom, pm)
    assert _dry_label(run.call) == c.label
    col = run()
    want = G.cols_ref(pd["x"], pom, pm)
    assert torch.equal(want.to(col.dtype).double(), want), "the exact reference is not representable"
    bad = (col.cpu() != want.to(col.dtype)) | torch.isnan(col.cpu())
    assert not bool(bad.any()), f"exact: {int(bad.sum())} columns differ, largest difference {_err(col.cpu(), want):.3e}"
    print("    exact: equal")


@pytest.mark.parametrize("c", GRAD, ids=[case_id(c) for c in GRAD])
def test_gradient_row(ot, dev, c):
    B = _batch(c)
    mm = MASK_MODE[c.mask]
    omc = G.om_channels(c)
    om, _ = G.geometry(c, B)
    d = G.operands(c, B)
    run = Run(ot, c, B, dev, d, om, mm)
    label = _dry_label(run.call)
    print(f"\n{label:60s} {_shape(c, B)}")
    assert label == c.label, f"the launcher sends this shape to {label}"
    assert bool(torch.isnan(run.bufs[1][1]).all()) and bool((run.bufs[0][1] == 0).all()), "the dry run launched"
    dx, dom = run()
    xd, omd = d["x"].to(dev), om.to(dev)
    if c.op == "col2im":
        rdx, rdom = G.col2im_ref(d["dcol"].to(dev), xd, omd, mm, c.chunked)
    else:
        rdx, rdom = G.fused_ref(d["dy"].to(dev), d["weight"].to(dev), xd, omd, mm)
    res = []
    if c.kind == "window" and c.Cin == 64:          # per chunk, against the chunk's own magnitude
        for k in range(2):
            res.append(_check(f"dense dx chunk {k}", dx[..., 32 * k:32 * k + 32], rdx[..., 32 * k:32 * k + 32], DX_TOL[c.mode], floor=0.0))
    else:
        res.append(_check("dense dx", dx, rdx, DX_TOL[c.mode]))
    res.append(_check("dense dom", dom[..., :omc], rdom, DOM_TOL[c.mode]))
    for what, err, bound in res:
        assert err <= bound, f"{what}: max err {err:.3e} > {bound:.3e}"
    run.check_dom_form(dom)
    outside = G.classify(c, om)["outside"].to(dev)
    _outside_dom_is_zero(c, dom, outside)
    if c.op != "col2im":
        return

    # ---- the samples outside the image add nothing to dx, whatever their dcol
    d2 = dict(d)
    t = G.tap_major(d["dcol"], c.Cin, c.chunked).clone()
    t[outside.cpu()] = 1e4
    if c.chunked:
        t = t.view(B, c.H, c.W, 9, c.Cin // 32, 32).transpose(3, 4)
    d2["dcol"] = t.reshape(B, c.H, c.W, 9 * c.Cin).contiguous()
    run2 = Run(ot, c, B, dev, d2, om, mm)
    dx2, dom2 = run2()
    run2.check_dom_form(dom2)
    _outside_dom_is_zero(c, dom2, outside)
    diff = (dx2 - dx).abs().max().item()
    if c.kind == "generic" or c.nt == 9:
        # the same terms in another order: n terms of absolute sum S differ by at most 2 (n - 1) 2^-24 S between two orders
        oma = om.clone()
        oma[..., 18:] = oma[..., 18:].abs()                    # (a PROB mask may be negative)
        s_abs, _ = G.col2im_ref(d["dcol"].abs().to(dev), xd, oma.to(dev), mm, c.chunked)
        n, _ = G.col2im_ref(d["dcol"].to(dev), xd, omd, mm, c.chunked, counts=True)
        excess = ((dx2 - dx).abs().double() - 2.0 ** -23 * n * s_abs).max().item()
        print(f"    dcol = 1e4 outside the image: dx differs by {diff:.3e}, {excess:.3e} above the reordering bound (n max {int(n.max())})")
        assert excess <= 0, f"dx changes by {diff:.3e} with the dcol of samples outside the image"
    else:
        bound = DX_TOL[c.mode] * max(1.0, rdx.abs().max().item())
        print(f"    dcol = 1e4 outside the image: dx differs by {diff:.3e} / bound {bound:.3e} = {diff / bound:.3f}")
        assert diff <= bound, f"dx changes by {diff:.3e} > {bound:.3e} with the dcol of samples outside the image"

    # ---- exact: permutation geometry, mask 1
    pm = 2 if c.mask == "none" else 1
    pom, pd = G.perm_geometry(c, B), G.operands(c, B, exact=True)
    run = Run(ot, c, B, dev, pd, pom, pm)
    assert _dry_label(run.call) == c.label
    dx, dom = run()
    wdx, wdom = G.col2im_ref(pd["dcol"], pd["x"], pom, pm, c.chunked)
    assert torch.equal(wdx.float().double(), wdx) and torch.equal(wdom.float().double(), wdom), "the exact reference is not representable"
    run.check_dom_form(dom)
    dx, dom = dx.cpu(), dom.cpu()
    bad = (dx != wdx.float()) | torch.isnan(dx)
    assert not bool(bad.any()), f"exact: {int(bad.sum())} elements of dx differ, largest difference {_err(dx, wdx):.3e}"
    bad = (dom[..., :omc] != wdom.to(dom.dtype)) | torch.isnan(dom[..., :omc])
    assert not bool(bad.any()), f"exact: {int(bad.sum())} elements of dom differ, largest difference {_err(dom[..., :omc], wdom):.3e}"
    # and with dcol = 1e4 outside the image: here no sum depends on its order, so dx must not change in any kernel
    t = G.tap_major(pd["dcol"], c.Cin, c.chunked).clone()
    t[G.classify(c, pom)["outside"]] = 1e4
    if c.chunked:
        t = t.view(B, c.H, c.W, 9, c.Cin // 32, 32).transpose(3, 4)
    pd2 = dict(pd, dcol=t.reshape(B, c.H, c.W, 9 * c.Cin).contiguous())
    dx2, _ = Run(ot, c, B, dev, pd2, pom, pm)()
    assert torch.equal(dx2.cpu(), dx), f"exact: dx changes by {_err(dx2.cpu(), dx.double()):.3e} with the dcol of samples outside the image"
    print("    exact: dx and dom equal; dx bit for bit the same with dcol = 1e4 outside the image")
