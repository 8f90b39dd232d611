"""Case table, launch geometry, float64 reference and error bound of the depthwise 3x3 kernels (csrc/dwconv.hip):
dwconv3x3_kernel<T, S> (forward; with rot180 the input gradient of a stride-1 layer), dwconv3x3_wgrad_kernel<T> and
dwconv3x3_wgrad_finalize_kernel.

A row gives the number of 16-byte channel vectors CV, so that one row serves both dtypes: C = 4 CV in f32, 8 CV in f16.
tests/test_dwconv_edges_host.py asserts for every row the property it is there for, against the constants read out of
dwconv.hip, so that a change of DW3_ROWS, WG3_ROWS or WG3_MAX_GROUPS moves the rows instead of silently emptying them.

Reference: nine shifted products in float64 on NHWC tensors (the host test holds it against F.conv2d, F.conv_transpose2d
and torch.nn.grad.conv2d_weight).  Bounds, u = 2^-24, an element that passes through at most D additions contributing at most
D u times the sum of the magnitudes of its terms, the tolerance twice that:
    forward / input gradient   one chain of 9 FMAs: 2 * 9 u sum |w| |x|; an f16 output adds 2^-11 |ref| + 2^-24
    weight gradient            a lane adds WG3_ROWS * ceil(ntiles / G) products serially (WG3_ROWS rows of a tile, tiles g, g + G,
                               ..), then the XL lanes of the workgroup are added serially: D = WG3_ROWS * ceil(ntiles / G) + XL
                               (the f64 finalize adds nothing at this scale); then one rounding of scale * sum to f32 and, with
                               accumulate, one of the add.  f16 products are exact in f32: the same bound."""
import torch
import torch.nn.functional as F

U = 2.0 ** -24
DW3_ROWS = 4                 # output rows a thread of the forward kernel walks
WG3_ROWS = 16                # rows of a weight-gradient tile
WG3_MAX_GROUPS = 1024        # cap of the weight-gradient grid
VEC = {torch.float32: 4, torch.float16: 8}
DTYPES = (torch.float32, torch.float16)


def wgrad_geom(B, H, W, C, N):
    """wgrad_geom of dwconv.hip: (XL, ncol, nstrip, ntiles, G)"""
    XL = 256 // (C // N)
    ncol = (W + XL - 1) // XL
    nstrip = (H + WG3_ROWS - 1) // WG3_ROWS
    ntiles = B * ncol * nstrip
    return XL, ncol, nstrip, ntiles, min(ntiles, WG3_MAX_GROUPS)


def wgrad_depth(B, H, W, C, N):
    XL, _, _, ntiles, G = wgrad_geom(B, H, W, C, N)
    return WG3_ROWS * -(-ntiles // max(G, 1)) + XL


# (name, B, CV, H, W, strides): forward and (stride 1, rot180) input gradient
FWD_ROWS = [
    ("1x1", 1, 4, 1, 1, (1, 2)),            # every neighbour is padding
    ("1x9", 2, 4, 1, 9, (1, 2)),            # ... in the vertical direction
    ("9x1", 2, 4, 9, 1, (1, 2)),            # ... in the horizontal direction
    ("2x2", 1, 4, 2, 2, (1, 2)),
    ("s2 4x6", 1, 4, 4, 6, (2,)),           # stride 2 on even / odd sizes
    ("s2 5x6", 1, 4, 5, 6, (2,)),
    ("s2 4x7", 1, 4, 4, 7, (2,)),
    ("s2 5x7", 1, 4, 5, 7, (2,)),
    ("H4", 1, 4, 4, 6, (1,)),               # Ho at, just above, at twice and just above twice DW3_ROWS: the last strip
    ("H5", 1, 4, 5, 6, (1,)),               # of H5 and H9 holds one row
    ("H8", 1, 4, 8, 6, (1,)),
    ("H9", 1, 4, 9, 6, (1,)),
    ("seam", 1, 20, 5, 13, (1,)),           # Wo * CV = 260 threads: the workgroup seam falls inside pixel 12
    ("seam s2", 1, 20, 5, 25, (2,)),
    ("Cmin", 1, 1, 3, 5, (1, 2)),           # 4 / 8 channels
    ("Cmax", 1, 256, 3, 5, (1, 2)),         # 1024 / 2048 channels
    ("B3", 3, 4, 9, 6, (1, 2)),             # batch times row strips in blockIdx.y
]
SLICE_ROWS = ("9x1", "seam")                # input and output as channel slices of wider buffers

# (name, B, CV, H, W): weight gradient, stride 1, both dtypes
WGRAD_ROWS = [(n, B, CV, H, W) for n, B, CV, H, W, s in FWD_ROWS if 1 in s] + [
    ("H16", 1, 4, 16, 6),                   # one full strip, one strip and a row, two strips and a row
    ("H17", 1, 4, 17, 6),
    ("H33", 2, 4, 33, 6),
    ("W=XL", 1, 64, 3, 4),                  # XL = 4 columns a tile
    ("W=XL+1", 1, 64, 3, 5),
    ("W=2XL", 1, 64, 3, 8),
]
# (name, dtype, B, C, H, W, ntiles, workgroups with a second tile, with a third): the rows where WG3_MAX_GROUPS binds
CAPPED_ROWS = [
    ("f32 1040 tiles", torch.float32, 1, 1024, 17, 520, 1040, 16, 0),
    ("f32 2080 tiles", torch.float32, 2, 1024, 17, 520, 2080, 1024, 32),
    ("f16 1032 tiles", torch.float16, 4, 160, 33, 1025, 1032, 8, 0),     # XL = 12: the last column tile is 5 of 12 wide
]
BEHAVIOUR_SMALL = ("H17", "seam")           # the small rows that get the workspace / into / scale / determinism checks too


def fwd_row(name):
    return next(r for r in FWD_ROWS if r[0] == name)


def wgrad_row(name):
    return next(r for r in WGRAD_ROWS if r[0] == name)


def make_inputs(seed, dtype, B, H, W, C, with_dy=False):
    """NHWC x (and dy), OIHW w [C,1,3,3] f32; f16 cases hold f16-representable values"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, C, generator=g)
    w = torch.randn(C, 1, 3, 3, generator=g) * 0.4
    dy = torch.randn(B, H, W, C, generator=g) if with_dy else None
    if dtype == torch.float16:
        x = x.half().float()
        dy = dy.half().float() if with_dy else None
    return x, w, dy


def out_size(n, stride):
    return (n - 1) // stride + 1


def fwd_ref(x, w, stride, rot180=False):
    """(y, magnitude) in float64, NHWC: y = dwconv(x, w), pad 1; rot180: the taps rotated by 180 degrees"""
    x, w = x.double(), w.double().reshape(-1, 3, 3)
    B, H, W, C = x.shape
    Ho, Wo = out_size(H, stride), out_size(W, stride)
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    y = torch.zeros(B, Ho, Wo, C, dtype=torch.float64)
    mag = torch.zeros_like(y)
    for ky in range(3):
        for kx in range(3):
            wt = w[:, 2 - ky, 2 - kx] if rot180 else w[:, ky, kx]
            xs = xp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride]
            y += xs * wt
            mag += xs.abs() * wt.abs()
    return y, mag


def fwd_tol(ref, mag, f16):
    tol = 2 * 9 * U * mag
    return tol + 2.0 ** -11 * ref.abs() + 2.0 ** -24 if f16 else tol


def wgrad_ref(x, dy):
    """(dw, magnitude) [C,1,3,3] in float64: dw[c,ky,kx] = sum over b, y, x of dy[b,y,x,c] * x[b,y-1+ky,x-1+kx,c]"""
    x, dy = x.double(), dy.double()
    B, H, W, C = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    xa, da = xp.abs(), dy.abs()
    dw = torch.zeros(C, 1, 3, 3, dtype=torch.float64)
    mag = torch.zeros_like(dw)
    for ky in range(3):
        for kx in range(3):
            dw[:, 0, ky, kx] = (dy * xp[:, ky:ky + H, kx:kx + W]).sum((0, 1, 2))
            mag[:, 0, ky, kx] = (da * xa[:, ky:ky + H, kx:kx + W]).sum((0, 1, 2))
    return dw, mag


def wgrad_tol(dw, mag, depth, scale=1.0, base=None):
    """2 (D u scale sum |dy| |x|  +  u |scale dw|  [+ u |base + scale dw|, accumulate])"""
    e = depth * U * abs(scale) * mag + U * (scale * dw).abs()
    if base is not None:
        e = e + U * (base + scale * dw).abs()
    return 2 * e


def worst_ratio(got, ref, tol):
    """max |got - ref| / tol, an element with tol == 0 (nothing but padding under the tap) having to be exact"""
    err = (got.double() - ref).abs()
    assert (err[tol == 0] == 0).all(), "a result that is all padding is not exactly zero"
    live = tol > 0
    return float((err[live] / tol[live]).max()) if live.any() else 0.0
