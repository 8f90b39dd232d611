"""Case tables, input builders, float64 references and bounds for the map-wise kernels between the convolutions:
    csrc/pointwise.hip   maxpool2x2, maxpool3x3s2 (pad 1 and ceil), dwconvT_add (generic and rows<2|4|8>), global_avgpool, ese_scale,
                         preprocess (u8 | f32 -> f16 | f32, not mirrored)
    csrc/train_bwd.hip   maxpool2x2_bwd, maxpool3x3s2_bwd, dwconvT_dw, dwconvT_dx, ese_dot, ese_bwd, depth_to_space2
each in f16 and f32.  Every shape is the smallest that takes the branch named next to it.  test_pointwise_host.py checks the tables
against their own conditions on the CPU; test_pointwise_gpu.py runs the kernels over them.

Out of scope: the BatchNorm kernels (bn_cases.py holds their tables; test_bn_gpu.py runs them), the weight-pack kernels, the mirrored preprocess (test_tta_gpu.py), and NaN inputs to the pools: the
kernels compare with `>`, which drops a NaN, where torch propagates it.  The eval step is behind the finite guard, so no NaN reaches
a pool there; that difference is written down here and not tested.  The `gy > 65535` fall-back of launch_dwconvT_add to the generic
kernel needs B * ceil(H / 8) * f > 65535, which no map of test size reaches.

Inputs: f16-representable values where the tensor is f16, f32 values otherwise; weights and gates are f32.  The kernel and the
reference therefore start from the same numbers.  References: plain torch on the CPU in float64 -- F.max_pool2d, F.conv_transpose2d(...,
groups=C) and mean, under autograd for the backward kernels (the wrap case of dwconvT_bwd computes the same sums tap by tap;
the host test holds that form to autograd on the small cases).

Bounds, per element, nothing left out, no max-norm scaling:
  * selection and copy kernels (both pools forward, depth_to_space2): torch.equal.  (+0.0 and -0.0 compare equal: on a tie of the two
    the forward kernels return the later one, torch the first.)
  * pool backward: torch.equal with float64 autograd rounded once to the tensor type.  dz holds multiples of 2^-6 in [-4, 4], so sums
    of up to four are exact in f32 and representable in f16; x holds multiples of 0.5 in [-2, 2], so many windows have ties, and
    the channels 0..3 of window (0, 0) of image 0 hold a constant window, a +0.0 / -0.0 window, an all -inf window and one +inf.
  * sums of n products in f32:  |got - ref| <= (n + 2) * 2^-24 * A + u_T * |ref|,  A the float64 sum of the absolute values of the
    element's terms (skip / identity / bias term included), n the number of terms the element really has, u_T = 2^-11 for f16 outputs
    and 0 for f32 outputs.  n roundings of at most 2^-24 * A each cover any order of summation (the atomics of dwconvT_dw included),
    fused or not; the two spare ones cover hsigmoid's add and division.
    No f16 output may be subnormal (u_T is a relative error).  The builders see to that without retries: where an f16 tensor is a sum,
    all terms of an output element have one sign -- x, skip and dz carry a sign per channel, the weights another -- and every
    magnitude is at least 0.25.  Both signs occur in every tensor with more than one channel.  The f32-output sums (dw, mean, dot) mix
    signs freely.

Worst err / bound per kernel and dtype, measured on an MI355X on 2026-10-18 at the commit that adds this file (parent 6fb959f):
    dwconvT_add                 f16  0.997
    dwconvT_add                 f32  0.438
    dwconvT_add_rows<2>         f16  0.996
    dwconvT_add_rows<2>         f32  0.403
    dwconvT_add_rows<4>         f16  0.996
    dwconvT_add_rows<4>         f32  0.431
    dwconvT_add_rows<8>         f16  0.996
    dwconvT_add_rows<8>         f32  0.434
    dwconvT_dw                  f16  0.376
    dwconvT_dw                  f32  0.419
    dwconvT_dw (wrap)           f16  < 0.001
    dwconvT_dx                  f16  0.991
    dwconvT_dx                  f32  0.277
    dwconvT_dx (wrap)           f16  0.997
    ese_bwd                     f16  0.994
    ese_bwd                     f32  0.250
    ese_dot                     f16  0.106
    ese_dot                     f32  0.207
    ese_scale                   f16  0.999
    ese_scale                   f32  0.444
    global_avgpool              f16  0.113
    global_avgpool              f32  0.283
    preprocess f32->f16         f16  0.992
    preprocess f32->f32         f32  0.264
    preprocess u8->f16          f16  0.927
    preprocess u8->f32          f32  0.259
The f16 figures close to 1 are the rounding of the result to f16 (half an ulp against u_T = 2^-11), not the sums; both pools, their
backward kernels, depth_to_space2, the saturated eSE gates and every sentinel comparison were exact.
"""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

F16, F32 = torch.float16, torch.float32
DTYPES = [F16, F32]
VEC = {F16: 8, F32: 4}                    # N: elements of a 16-byte channel vector
U_T = {F16: 2.0 ** -11, F32: 0.0}
U32 = 2.0 ** -24
F16_MIN_NORMAL = 2.0 ** -14

# launch constants mirrored from the sources
BLOCK = 256                               # threads per workgroup, one channel vector each in the element-wise kernels
DW_ROWS = 8                               # pointwise.hip: output rows of one phase that a thread of dwconvT_add_rows_kernel walks
DW_GRID_CAP = 512                         # train_bwd.hip launch_dwconvT_bwd_t: workgroups per tap phase of dwconvT_dw_kernel
DW_POS_PER_SUB = 16                       # ... positions per sub-thread that the uncapped grid is sized for
DX_GRID_CAP = 4096                        # ... workgroups of dwconvT_dx_kernel
ESE_CH, ESE_PL = 64, 4                    # global_avgpool / ese_dot: 64 channels x 4 pixel lanes per workgroup
SENTINEL = {F16: 0x5A5A, F32: 0x5A5A5A5A}  # bit pattern of the memory a kernel must leave alone (203.25 / 1.5e16: finite)


def dt_name(dt):
    return "f16" if dt == F16 else "f32"


def dw_sub_threads(CV):
    """S of dwconvT_dw_kernel: pixel positions a workgroup takes at a time"""
    return BLOCK // CV


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2)


def bound(n, A, ref, dt):
    return (n + 2) * U32 * A + U_T[dt] * ref.abs()


def ratio(got, ref, n, A, dt):
    """worst |got - ref| / bound over all elements (float64 tensors); an element whose bound is 0 must be met exactly"""
    err = (got.double() - ref).abs()
    b = bound(n, A, ref, dt).expand_as(err)
    r = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return r.max().item()


def chan_signs(C):
    """(sigma, tau): two +-1 patterns over the channels, both signs in each (and in their product) once C >= 4"""
    c = torch.arange(C)
    return (1 - 2 * (c % 2)).float(), (1 - 2 * ((c // 2) % 2)).float()


def _mag(shape, g, lo=0.25, hi=4.0):
    return torch.rand(shape, generator=g) * (hi - lo) + lo


def _signed(shape, g):
    return _mag(shape, g) * (torch.randint(0, 2, shape, generator=g) * 2 - 1)


def _seed(*parts):
    return int(sum((i + 1) * 7919 * int(p) for i, p in enumerate(parts)) % (2 ** 31))


# ------------------------------------------------------------------------------------------------------------------------
# max pooling
# ------------------------------------------------------------------------------------------------------------------------
# mode: "2x2", "pad1" (F.max_pool2d(x, 3, 2, 1)) or "ceil" (nn.MaxPool2d(3, 2, ceil_mode=True)); C = CV * N
PoolCase = namedtuple("PoolCase", "mode B H W CV strided")

POOL_CASES = [
    PoolCase("2x2", 1, 2, 2, 1, False),        # one window
    PoolCase("2x2", 2, 6, 10, 3, False),       # CV = 3: divisions instead of masks
    PoolCase("2x2", 2, 10, 14, 5, False),      # 350 vectors: a full and a ragged workgroup
    PoolCase("2x2", 2, 6, 10, 3, True),        # x, dz and the output as channel slices of buffers 2C + N wide
] + [PoolCase(mode, B, H, W, 2, False) for mode in ("pad1", "ceil") for (B, H, W) in (
    (1, 3, 3),                                 # one ceil window (pad 1: four windows that share the centre)
    (2, 4, 7),                                 # ceil: the last window hangs over by one row
    (2, 5, 8),                                 # ... by one column
    (2, 8, 5),                                 # the same with H and W exchanged
    (2, 4, 6),                                 # ... by both
    (2, 17, 25),                               # interior elements lying in four windows
)] + [PoolCase("ceil", 2, 5, 8, 2, True), PoolCase("pad1", 2, 5, 8, 2, True)]
# launch_maxpool3x3s2's `if ((Ho - 1) * 2 >= H) --Ho` (pad 0) never fires for 3 <= H <= 64: Ho - 1 = (H - 2) // 2, and
# 2 * ((H - 2) // 2) <= H - 2 < H.  test_pointwise_host.py runs the loop.

POOL_SPECIALS = ("constant", "zeros", "ninf", "pinf")      # channel e of window (0, 0) of image 0 holds POOL_SPECIALS[e]


def pool_id(c):
    return f"{c.mode}-{c.B}x{c.H}x{c.W}-cv{c.CV}" + ("-strided" if c.strided else "")


def pool_out_hw(mode, H, W):
    if mode == "2x2":
        return H // 2, W // 2
    if mode == "pad1":
        return (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return -(-(H - 3) // 2) + 1, -(-(W - 3) // 2) + 1


def pool_window(mode, H, W, ho, wo):
    """(rows, columns) of the map that window (ho, wo) holds"""
    k, s, p = (2, 2, 0) if mode == "2x2" else (3, 2, 1 if mode == "pad1" else 0)
    return ([y for y in range(ho * s - p, ho * s - p + k) if 0 <= y < H], [x for x in range(wo * s - p, wo * s - p + k) if 0 <= x < W])


@functools.lru_cache(maxsize=None)
def pool_inputs(case, dt):
    """x [B,H,W,C] (multiples of 0.5 in [-2, 2] and the special windows), dz [B,Ho,Wo,C] (multiples of 2^-6 in [-4, 4]), type dt"""
    C = case.CV * VEC[dt]
    g = torch.Generator().manual_seed(_seed(case.B, case.H, case.W, case.CV, len(case.mode), VEC[dt]))
    x = torch.randint(-4, 5, (case.B, case.H, case.W, C), generator=g).float() / 2
    ys, xs = pool_window(case.mode, case.H, case.W, 0, 0)
    if case.mode != "2x2":          # the 3x3 block at the corner: window (0, 0) of either mode lies in it
        ys, xs = list(range(min(3, case.H))), list(range(min(3, case.W)))
    for y in ys:
        for xx in xs:
            x[0, y, xx, 0] = 1.0
            x[0, y, xx, 1] = -0.0 if (y + xx) % 2 == 0 else 0.0
            x[0, y, xx, 2] = float("-inf")
    x[0, 1, 0, 3] = float("inf")                # inside window (0, 0) of every mode
    Ho, Wo = pool_out_hw(case.mode, case.H, case.W)
    dz = torch.randint(-256, 257, (case.B, Ho, Wo, C), generator=g).float() / 64
    return {"x": x.to(dt), "dz": dz.to(dt)}


def _pool_f(mode, x):
    if mode == "2x2":
        return F.max_pool2d(x, 2, 2)
    if mode == "pad1":
        return F.max_pool2d(x, 3, 2, 1)
    return F.max_pool2d(x, 3, 2, 0, ceil_mode=True)


def pool_reference(case, dt, compute=torch.float64):
    """y and dx (NHWC, type dt): torch in `compute` precision under autograd, rounded once"""
    inp = pool_inputs(case, dt)
    x = nchw(inp["x"]).to(compute).requires_grad_(True)
    y = _pool_f(case.mode, x)
    y.backward(nchw(inp["dz"]).to(compute))
    return {"y": nhwc(y.detach()).to(dt), "dx": nhwc(x.grad).to(dt)}


def pool_reference_last_max(case, dt):
    """WRONG on purpose: the gradient goes to the last maximum in scan order (2x2 only: the flipped map's first)"""
    assert case.mode == "2x2"
    inp = pool_inputs(case, dt)
    x = nchw(inp["x"]).double().flip(2, 3).requires_grad_(True)
    F.max_pool2d(x, 2, 2).backward(nchw(inp["dz"]).double().flip(2, 3))
    return nhwc(x.grad.flip(2, 3)).to(dt)


def pool_reference_floor(case, dt):
    """WRONG on purpose: the ceil pool without its hanging windows"""
    assert case.mode == "ceil"
    return nhwc(F.max_pool2d(nchw(pool_inputs(case, dt)["x"]).double(), 3, 2, 0)).to(dt)


# ------------------------------------------------------------------------------------------------------------------------
# depthwise up-convolution: ConvTranspose2d(C, C, 2f, stride=f, padding=f/2, groups=C)(x) + skip, and its backward
# ------------------------------------------------------------------------------------------------------------------------
UpCase = namedtuple("UpCase", "B H W CV f strided")


def up_rows_kernel(c):
    """launch_dwconvT_add takes dwconvT_add_rows_kernel<f> (else the generic dwconvT_add_kernel)"""
    nchunk = -(-c.H // DW_ROWS)
    return c.f in (2, 4, 8) and c.CV & (c.CV - 1) == 0 and c.B * nchunk * c.f <= 65535


def up_grid(c):
    """workgroups: (x, y) of the rows kernel, (x, 1) of the generic one"""
    if up_rows_kernel(c):
        return -(-(c.W * c.f * c.CV) // BLOCK), c.B * -(-c.H // DW_ROWS) * c.f
    return -(-(c.B * c.H * c.f * c.W * c.f * c.CV) // BLOCK), 1


_UP_MAPS = [(1, 1, 1),           # every tap hits a border
            (1, 9, 3),           # two DW_ROWS chunks, the second with one input row
            (2, 9, 3)]           # blockIdx.y splits into (b, chunk, phase)
UP_FWD_CASES = (
    [UpCase(B, H, W, CV, f, False) for f in (2, 4, 8) for CV in (1, 8) for (B, H, W) in _UP_MAPS]          # the rows kernel
    + [UpCase(1, 2, 20, 8, 2, False), UpCase(1, 1, 5, 8, 8, False), UpCase(1, 1, 80, 1, 4, False)]         # W * f * CV = 320: two
    #                                                                                     x-workgroups, the second ragged
    + [UpCase(B, H, W, CV, f, False) for (CV, f) in ((3, 2), (3, 4), (8, 6), (3, 6)) for (B, H, W) in _UP_MAPS[::2]]   # generic
    + [UpCase(2, 9, 3, 8, 2, True), UpCase(2, 9, 3, 3, 2, True)]      # x, skip and out as channel slices: rows and generic kernel
)
UP_BWD_CASES = (
    [UpCase(B, H, W, CV, f, False) for f in (2, 4, 8) for CV in (1, 3, 8) for (B, H, W) in _UP_MAPS]
    + [UpCase(1, 2, 20, 8, 2, False), UpCase(1, 1, 5, 8, 8, False), UpCase(1, 1, 80, 1, 4, False)]
    + [UpCase(1, 2, 2, 256, 2, False),         # C = 2048 f16 / 1024 f32: S = 1, 32 KB (16 KB) of LDS
       UpCase(2, 17, 15, 8, 2, False),         # 576 positions > 16 S = 512: two workgroups of dwconvT_dw_kernel per phase
       UpCase(2, 9, 3, 8, 2, True)]            # x, dz and dx as channel slices
)
# both grid caps at once: B (H + 1) (W + 1) = 263 168 > 512 * 16 * S = 262 144 and B H W CV = 2 088 960 > 4096 * 256; with one row
# fewer (262 140 positions) dwconvT_dw_kernel's grid is no longer capped.  (B = 4, 256 x 256 meets both conditions too, but is not
# the smallest: it still meets them with a row less.)  f16 only.
UP_WRAP_CASE = UpCase(4, 255, 256, 8, 2, False)
UP_WRAP_DTYPE = F16
UP_WRAP_BOOST = 64.0         # x of the rows that only the wrapped pass of dwconvT_dw_kernel reaches is this much larger: they make
#                              0.4 % of the positions, which the bound of a 2.6e5-term sum (1.6 % of A) would not see otherwise


def up_id(c):
    return f"{c.B}x{c.H}x{c.W}-cv{c.CV}-f{c.f}" + ("-strided" if c.strided else "")


def up_wrap_tail(c):
    """(image, first input row) from which on every (iy1, ix1) position of dwconvT_dw_kernel lies beyond the first DW_POS_PER_SUB
    passes of a capped grid"""
    first = DW_GRID_CAP * DW_POS_PER_SUB * dw_sub_threads(c.CV)
    b, rem = divmod(first, (c.H + 1) * (c.W + 1))
    return b, -(-rem // (c.W + 1))


@functools.lru_cache(maxsize=4)
def up_inputs(case, dt):
    """x [B,H,W,C], skip and dz [B,Hf,Wf,C] of type dt, w f32 [C,1,2f,2f]"""
    B, H, W, CV, f = case[:5]
    C = CV * VEC[dt]
    g = torch.Generator().manual_seed(_seed(B, H, W, CV, f, VEC[dt]))
    sg, tau = chan_signs(C)
    x = (_mag((B, H, W, C), g) * sg).to(dt)
    skip = None
    if case == UP_WRAP_CASE:                    # backward only: no skip
        b0, y0 = up_wrap_tail(case)
        x[b0, y0:] *= UP_WRAP_BOOST
    else:
        skip = (_mag((B, H * f, W * f, C), g) * sg * tau).to(dt)
    dz = (_mag((B, H * f, W * f, C), g) * sg).to(dt)
    w = _mag((C, 1, 2 * f, 2 * f), g, 0.25, 1.25) * tau.view(C, 1, 1, 1)
    return {"x": x, "skip": skip, "dz": dz, "w": w}


def _convT(x, w, f):
    return F.conv_transpose2d(x, w, None, stride=f, padding=f // 2, groups=w.shape[0])


def up_fwd_reference(case, dt, with_skip, compute=torch.float64, drop_tap=False):
    """ref, A (NHWC) and n ([1,Hf,Wf,1]) of y = up(x) (+ skip).  drop_tap: WRONG on purpose -- the border output (0, f - f/2), which
    has the taps of input pixels (0, 0) and (0, 1) only, is left without the first: x[0, 0] * w[f/2][f]"""
    inp = up_inputs(case, dt)
    x, w = nchw(inp["x"]).to(compute), inp["w"].to(compute)
    p = case.f // 2
    y, A = _convT(x, w, case.f), _convT(x.abs(), w.abs(), case.f)
    if drop_tap:
        y[:, :, 0, case.f - p] -= x[:, :, 0, 0] * w[:, 0, p, case.f]
    n = _convT(torch.ones(1, 1, case.H, case.W, dtype=compute), torch.ones(1, 1, 2 * case.f, 2 * case.f, dtype=compute), case.f)
    if with_skip:
        s = nchw(inp["skip"]).to(compute)
        y, A, n = y + s, A + s.abs(), n + 1
    return {"y": nhwc(y), "A": nhwc(A), "n": nhwc(n)}


def _up_grads(x, dz, w, f):
    x, w = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    _convT(x, w, f).backward(dz)
    return x.grad, w.grad


def up_bwd_reference(case, dt, compute=torch.float64):
    """autograd of conv_transpose2d: dx, A_dx (NHWC), n_dx [1,H,W,1]; dw, A_dw [C,1,k,k], n_dw [1,1,k,k]"""
    inp = up_inputs(case, dt)
    x, dz, w = nchw(inp["x"]).to(compute), nchw(inp["dz"]).to(compute), inp["w"].to(compute)
    dx, dw = _up_grads(x, dz, w, case.f)
    Adx, Adw = _up_grads(x.abs(), dz.abs(), w.abs(), case.f)
    one = torch.ones(1, 1, case.H, case.W, dtype=compute)
    ndx, ndw = _up_grads(one, torch.ones(1, 1, case.H * case.f, case.W * case.f, dtype=compute),
                         torch.ones(1, 1, 2 * case.f, 2 * case.f, dtype=compute), case.f)
    return {"dx": nhwc(dx), "A_dx": nhwc(Adx), "n_dx": nhwc(ndx), "dw": dw, "A_dw": Adw, "n_dw": ndw * case.B}


def up_bwd_by_taps(x, dz, w, f, skip_from=None):
    """the same sums tap by tap, image by image, in float64, for maps on which autograd takes too long: x, dz NHWC of any type, w
    [C,1,k,k].  Returns dx [B,H,W,C], dw [C,1,k,k], n_dx [1,H,W,1], n_dw [1,1,k,k] in float64.  A is |ref| where the terms of every
    sum share a sign, which the caller establishes.  skip_from = (b, row): WRONG on purpose -- dw without the input rows from there on."""
    B, H, W, C = x.shape
    k, p = 2 * f, f // 2
    w64 = w.double()
    dx = torch.zeros(B, H, W, C, dtype=torch.float64)
    dw = torch.zeros(C, 1, k, k, dtype=torch.float64)
    ndx = torch.zeros(1, H, W, 1, dtype=torch.float64)
    ndw = torch.zeros(1, 1, k, k, dtype=torch.float64)
    iy, ix = torch.arange(H), torch.arange(W)
    for b in range(B):
        xb = x[b].double()
        if skip_from is not None and b >= skip_from[0]:
            xb = xb.clone()
            xb[(skip_from[1] if b == skip_from[0] else 0):] = 0
        dzp = F.pad(dz[b].double(), (0, 0, p, k, p, k))          # rows / columns -p .. Hf + k - 1 (zero outside the map)
        for ky in range(k):
            vy = ((iy * f - p + ky >= 0) & (iy * f - p + ky < H * f)).double()
            for kx in range(k):
                vx = ((ix * f - p + kx >= 0) & (ix * f - p + kx < W * f)).double()
                s = dzp[ky:ky + H * f:f, kx:kx + W * f:f]        # dz[b, iy f - p + ky, ix f - p + kx, :]
                dx[b].addcmul_(s, w64[:, 0, ky, kx])
                dw[:, 0, ky, kx] += (s * xb).sum((0, 1))
                if b == 0:
                    ndx[0, :, :, 0] += vy[:, None] * vx[None, :]
                    ndw[0, 0, ky, kx] = B * vy.sum() * vx.sum()
    return dx, dw, ndx, ndw


@functools.lru_cache(maxsize=1)
def up_wrap_reference():
    inp = up_inputs(UP_WRAP_CASE, UP_WRAP_DTYPE)
    dx, dw, ndx, ndw = up_bwd_by_taps(inp["x"], inp["dz"], inp["w"], UP_WRAP_CASE.f)
    return {"dx": dx, "A_dx": dx.abs(), "n_dx": ndx, "dw": dw, "A_dw": dw.abs(), "n_dw": ndw}


# ------------------------------------------------------------------------------------------------------------------------
# eSE: global_avgpool, ese_scale, ese_dot, ese_bwd
# ------------------------------------------------------------------------------------------------------------------------
EseCase = namedtuple("EseCase", "B H W C strided")         # C = None: N channels (one vector, idle channel lanes)
ESE_SHAPES = [(1, 1, 1, None),        # HW < 4: three pixel lanes with nothing to add; C = N < 64: idle channel lanes
              (2, 1, 3, None),        # HW = 3
              (3, 9, 13, 80),         # the second 64-channel workgroup is partial
              (2, 8, 8, 128)]
ESE_CASES = [EseCase(*s, False) for s in ESE_SHAPES] + [EseCase(3, 9, 13, 80, True)]      # the strided case of each kernel
# the knees of hsigmoid(s) = relu6(s + 3) / 6 and both sides of them; -3 + 2^-20 and 3 - 2^-20 are f32 numbers, s + 3 is exact
ESE_GATES = [-10.0, -3.0, -3.0 + 2.0 ** -20, 0.0, 3.0 - 2.0 ** -20, 3.0, 10.0]
ESE_GATE0, ESE_GATE1, ESE_TINY = (0, 1), (5, 6), 2         # indices: gate exactly 0, exactly 1, and 2^-20 / 6
ESE_TINY_BOOST = 4096.0              # x where the gate is 2^-20 / 6: x * gate alone (no identity) is then an f16 normal


def ese_id(c):
    return f"{c.B}x{c.H}x{c.W}x{c.C or 'N'}" + ("-strided" if c.strided else "")


def ese_channels(c, dt):
    return c.C or VEC[dt]


def ese_gate_index(B, C):
    """[B, C]: which of ESE_GATES a channel gets; shifted by 4 per image so that 2 x 4 channels see all seven"""
    return (torch.arange(C)[None, :] + 4 * torch.arange(B)[:, None]) % len(ESE_GATES)


def hsigmoid(s, clamp_hi=True):
    v = (s + 3.0).clamp_min(0.0)
    return (v.clamp_max(6.0) if clamp_hi else v) / 6.0


@functools.lru_cache(maxsize=None)
def ese_inputs(case, dt):
    """x, identity, dy [B,H,W,C] of type dt (per-channel signs: x * gate + identity and dy * gate + gp do not cancel); dy_dot
    [B,H,W,C] with free signs (the dot product's f32 sums may cancel); s, gate, gp f32 [B,C]"""
    B, H, W = case.B, case.H, case.W
    C = ese_channels(case, dt)
    g = torch.Generator().manual_seed(_seed(B, H, W, C, VEC[dt]))
    sg, _ = chan_signs(C)
    gi = ese_gate_index(B, C)
    s = torch.tensor(ESE_GATES, dtype=torch.float32)[gi]
    x = _mag((B, H, W, C), g) * sg
    x = torch.where((gi == ESE_TINY)[:, None, None, :], x * ESE_TINY_BOOST, x)
    gate = torch.clamp(s + 3.0, 0.0, 6.0) / 6.0              # f32, as EseFn.backward makes it
    return {"x": x.to(dt), "identity": (_mag((B, H, W, C), g) * sg).to(dt), "dy": (_mag((B, H, W, C), g) * sg).to(dt),
            "dy_dot": _signed((B, H, W, C), g).to(dt), "s": s, "gate": gate, "gp": _mag((B, C), g, 0.25, 1.0) * sg / 8}


def ese_reference(case, dt, compute=torch.float64, mean_div_extra=0, clamp_hi=True):
    """float64 (or `compute`) references of the four kernels with their A and n.  mean_div_extra, clamp_hi: WRONG on purpose"""
    inp = ese_inputs(case, dt)
    HW = case.H * case.W
    x, idn, dy, dyd = (inp[k].to(compute) for k in ("x", "identity", "dy", "dy_dot"))
    out = {"HW": HW}
    out["mean"] = x.sum((1, 2)) / (HW + mean_div_extra)
    out["A_mean"] = x.abs().sum((1, 2)) / HW
    gs = hsigmoid(inp["s"].to(compute), clamp_hi)[:, None, None, :]
    out["scale"], out["A_scale"] = x * gs, (x * gs).abs()
    out["scale_id"], out["A_scale_id"] = x * gs + idn, (x * gs).abs() + idn.abs()
    gl = torch.ones(case.B, x.shape[3], dtype=compute, requires_grad=True)      # d(sum dy * x * g) / dg under autograd
    (x * gl[:, None, None, :]).backward(dyd)
    out["dot"], out["A_dot"] = gl.grad, (dyd * x).abs().sum((1, 2))
    gt, gp = inp["gate"].to(compute)[:, None, None, :], inp["gp"].to(compute)[:, None, None, :]
    out["bwd"], out["A_bwd"] = dy * gt + gp, (dy * gt).abs() + gp.abs()
    return out


# ------------------------------------------------------------------------------------------------------------------------
# depth_to_space2: dst[b, y, x, c] = src[b, (y + 1) / 2, (x + 1) / 2, ((y & 1) * 2 + (x & 1)) * C + c]
# ------------------------------------------------------------------------------------------------------------------------
D2sCase = namedtuple("D2sCase", "B H W CV wide")          # wide: src_stride = 4C + N instead of 4C; dst is always a channel slice
D2S_CASES = [D2sCase(B, H, W, CV, wide) for (B, H, W, CV) in ((1, 1, 1, 1), (2, 5, 4, 3), (1, 6, 7, 2)) for wide in (False, True)]
D2S_RAISES = D2sCase(2, 5, 4, 3, False)                   # with Hs one short the launcher must refuse it


def d2s_id(c):
    return f"{c.B}x{c.H}x{c.W}-cv{c.CV}" + ("-wide" if c.wide else "")


def d2s_src_hw(H, W):
    """the smallest source map the launcher accepts"""
    return (H + 1) // 2 + (0 if H & 1 else 1), (W + 1) // 2 + (0 if W & 1 else 1)


def d2s_inputs(case, dt):
    """src buffer [B,Hs,Ws,src_stride] of distinct integers (all exact in f16)"""
    C = case.CV * VEC[dt]
    Hs, Ws = d2s_src_hw(case.H, case.W)
    stride = 4 * C + (VEC[dt] if case.wide else 0)
    n = case.B * Hs * Ws * stride
    return torch.arange(n, dtype=torch.float32).view(case.B, Hs, Ws, stride).to(dt)


def d2s_reference(case, dt, swap_parity=False):
    """swap_parity: WRONG on purpose -- row and column parity exchanged"""
    src = d2s_inputs(case, dt)
    C = case.CV * VEC[dt]
    out = torch.empty(case.B, case.H, case.W, C, dtype=dt)
    for y in range(case.H):
        for x in range(case.W):
            ph = (x & 1) * 2 + (y & 1) if swap_parity else (y & 1) * 2 + (x & 1)
            out[:, y, x] = src[:, (y + 1) // 2, (x + 1) // 2, ph * C:(ph + 1) * C]
    return out


# ------------------------------------------------------------------------------------------------------------------------
# preprocess: (x / 255 - mean) / std, zero padding to Hp x Wp, CHW -> NHWC, channels 3.. zero, optional border frame
# ------------------------------------------------------------------------------------------------------------------------
PreCase = namedtuple("PreCase", "in_dt out_dt H W Hp Wp border out_stride")
PRE_B = 2
PRE_MEAN, PRE_STD = [0.408, 0.447, 0.470], [0.289, 0.274, 0.278]
PRE_CASES = [PreCase(i, o, H, W, Hp, Wp, border, stride)
             for i in (torch.uint8, F32) for o in (F16, F32)
             for (H, W, Hp, Wp) in ((1, 1, 2, 3), (5, 7, 5, 7), (50, 70, 64, 96))          # 5x7: no padding
             for border in (0, 3) for stride in ((8,) if o == F16 else (4, 8))]


def pre_id(c):
    return (f"{'u8' if c.in_dt == torch.uint8 else 'f32'}-{dt_name(c.out_dt)}-{c.H}x{c.W}to{c.Hp}x{c.Wp}-border{c.border}"
            f"-stride{c.out_stride}")


def _pre_value(img, compute):
    m = torch.tensor(PRE_MEAN, dtype=torch.float32).to(compute).view(1, 3, 1, 1)       # the kernel gets mean and std as f32
    s = torch.tensor(PRE_STD, dtype=torch.float32).to(compute).view(1, 3, 1, 1)
    v = img.to(compute) / 255
    return (v - m) / s, (v.abs() + m.abs()) / s


@functools.lru_cache(maxsize=None)
def pre_inputs(in_dt, H, W):
    """images [B,3,H,W]: 0 and 255 in every channel; f32 images hold fractions, moved by 1 where the result would be an f16 subnormal"""
    g = torch.Generator().manual_seed(_seed(H, W, in_dt == F32))
    if in_dt == torch.uint8:
        img = torch.randint(0, 256, (PRE_B, 3, H, W), generator=g, dtype=torch.uint8)
    else:
        img = torch.rand(PRE_B, 3, H, W, generator=g) * 255
        small = _pre_value(img, torch.float64)[0].abs() < 2 * F16_MIN_NORMAL
        img = torch.where(small, img + 1.0, img)
    img[0, :, 0, 0] = 0
    img[PRE_B - 1, :, H - 1, W - 1] = 255
    return img


def pre_reference(case, compute=torch.float64):
    """ref and A [B,Hp,Wp,3] (NHWC, zero in the padding), n = 2 terms (x / 255 and the mean; three roundings)"""
    v, A = _pre_value(pre_inputs(case.in_dt, case.H, case.W), compute)
    pad = (0, case.Wp - case.W, 0, case.Hp - case.H)
    return {"y": nhwc(F.pad(v, pad)), "A": nhwc(F.pad(A, pad)), "n": 2}
