"""One row per instantiation of the DCN gradient kernels of csrc/train_bwd.hip (and the column sampler of csrc/conv_igemm.hip that
ops_train.dcn_cols reaches): the generic and LDS-window column kernels, the generic coordinate / col2im kernels in f16 and f32,
and the 18 instantiations of dcn_col2im_window_kernel<NT, T, FUSED, NM> the launchers can select (NT = 3, 5, 9 taps per
workgroup; T = f16 | float; FUSED only with float; NM = no mask).

test_dcn_grad_host.py replays every row through the library's dry run (no GPU) and asserts its label, checks that the table
covers every instantiation, that every row's geometry holds the edge classes the row lists, and the float64 references below
against the oracle and double autograd; test_dcn_grad_gpu.py runs every row once on the device against those references.

The labels assume 256 compute units (the MI355X; what ctdet_device_cu_count() answers outside a GPU process as well).

Row fields
  mode     "f16" | "f32" | "f16x3"
  op       "cols" (ops_train.dcn_cols) | "col2im" (ops_train.dcn_col2im_coord) | "col2im_fused" (ops_train.dcn_col2im_fused)
  kind     "generic" | "window"
  B        images, or None: taken from the CU count so that the launcher selects `nt` taps per workgroup (batch_of)
  H W Cin  the map and its channels; Cout: couts of the layer (col2im_fused only, dY is zero-padded to a multiple of 32)
  mask     "logit" | "prob" | "none" (DCN_MASK_LOGIT / _PROB / _NONE)
  dom_c    channels of dom (>= 27, or >= 18 without a mask); f16 mode: 32 -> an f16 dom, otherwise f32
  chunked  dcol in the chunked layout [Cin/32][tap][32] per pixel
  nt       taps per workgroup of the window scatter (0: not that kernel)
  label    the label of the launch
  edges    the edge classes the row's geometry must contain (classify)

Geometry.  Offsets are N(0, 1.5) rounded to the 2^-12 grid -- position = integer + offset is then exact in f32, so the float64
reference floors the very number the kernel floors (a position half an ulp from an integer would otherwise land in another
cell, and d(offset) is discontinuous there) -- with the designed samples of design() written over them; mask logits N(0, 1)."""
import math
from collections import namedtuple

import torch

from oracle import ctdet_oracle as O

Case = namedtuple("Case", "mode op kind B H W Cin Cout mask dom_c chunked nt label edges")
Sample = namedtuple("Sample", "cls b y x tap dh dw inwin")       # inwin: None, or the side of the window margin it is designed for
MASK_MODE = {"logit": 0, "prob": 1, "none": 2}
NCU = 256
TH, TW, MG = 8, 16, 4                     # the window kernels' tile and offset margin
EPS = 2.0 ** -10
BASE_EDGES = ("integer", "top_band", "left_band", "bottom_band", "right_band", "on_minus_one", "on_size", "far")
THIN_EDGES = ("integer", "top_band", "bottom_band", "on_minus_one", "on_size", "far")        # the 1 x 3 map
WIN_EDGES = BASE_EDGES + ("window_edge", "neg_index", "mixed_wave")


def om_channels(c):
    return 18 if c.mask == "none" else 27


def batch_of(c, ncu=NCU):
    """the row's batch on a device with ncu compute units, None when no batch selects the row's taps per workgroup there"""
    if c.B is not None:
        return c.B
    tiles = (c.H // TH) * (c.W // TW)
    for B in range(1, 4096):
        t = B * tiles
        nt = 3 if 3 * t <= ncu else 5 if 2 * t <= ncu else 9
        if nt == c.nt:
            return B
        if nt > c.nt:
            return None
    return None


def case_id(c):
    B = "Bncu" if c.B is None else f"{c.B}"
    extra = (f"-dom{c.dom_c}" if c.dom_c else "") + ("-chunked" if c.chunked else "") + (f"-to{c.Cout}" if c.Cout else "")
    return f"{c.mode}-{c.op}-{B}x{c.H}x{c.W}x{c.Cin}-{c.mask}{extra}-{c.label}"


def _m(mask):
    return "no mask" if mask == "none" else "mask"


def _row(mode, op, kind, B, H, W, Cin, mask, label, dom_c=0, chunked=False, nt=0, Cout=0, edges=None):
    if edges is None:
        edges = WIN_EDGES if kind == "window" else THIN_EDGES if H == 1 else BASE_EDGES
    return Case(mode, op, kind, B, H, W, Cin, Cout, mask, dom_c, chunked, nt, label, tuple(edges))


def _cols_rows():
    rows = []
    for mask in ("logit", "prob", "none"):
        rows += [
            _row("f16", "cols", "generic", 2, 5, 7, 8, mask, f"dcn_cols_kernel<f16,{_m(mask)}>"),
            _row("f16", "cols", "generic", 1, 1, 3, 72, mask, f"dcn_cols_kernel<f16,{_m(mask)}>"),       # 9 vectors: no power of two
            _row("f16", "cols", "window", 2, 16, 32, 32, mask, f"dcn_window_rows_kernel<columns only,f16,{_m(mask)}>"),
            _row("f16", "cols", "window", 2, 16, 32, 96, mask, f"dcn_window_rows_kernel<columns only,f16,{_m(mask)}>"),
            _row("f32", "cols", "generic", 2, 5, 7, 16, mask, f"dcn_cols_f32_kernel<{_m(mask)}>"),       # the minimum
            _row("f32", "cols", "generic", 2, 5, 7, 24, mask, f"dcn_cols_f32_kernel<{_m(mask)}>"),       # PP = 42: idle threads
            _row("f32", "cols", "generic", 1, 16, 32, 64, mask, f"dcn_cols_f32_kernel<{_m(mask)}>", edges=BASE_EDGES),
        ]
    return rows


def _generic_rows():
    f16 = lambda Cin, mask, dom_c: _row("f16", "col2im", "generic", 2, 5, 7, Cin, mask,          # noqa: E731
                                        f"dcn_col2im_coord_kernel<f16,{_m(mask)}>", dom_c)
    f32 = lambda mode, B, H, W, Cin, mask, dom_c: _row(mode, "col2im", "generic", B, H, W, Cin, mask,      # noqa: E731
                                                       f"dcn_col2im_coord_kernel<f32,{_m(mask)}>", dom_c, edges=BASE_EDGES)
    return [
        f16(8, "logit", 27), f16(8, "none", 18), f16(8, "prob", 28),
        f16(72, "logit", 32), f16(72, "none", 32), f16(72, "none", 20),
        f32("f32", 2, 5, 7, 16, "logit", 27), f32("f32", 2, 5, 7, 16, "none", 18),
        # the f32 mode takes the generic kernel on a tile-divisible map too
        f32("f32", 1, 16, 32, 64, "logit", 32), f32("f32", 1, 16, 32, 64, "none", 32),
        f32("f32", 1, 16, 32, 64, "none", 20), f32("f32", 1, 16, 32, 64, "logit", 28),
        # the f16x3 mode on a map without 8 x 16 tiles
        f32("f16x3", 2, 5, 7, 16, "logit", 32),
    ]


def _win_label(nt, mode, mask, fused=False):
    return f"dcn_col2im_window_kernel<{nt} taps,{'f16' if mode == 'f16' else 'f32'},{'fused dcol,' if fused else ''}{_m(mask)}>"


def _window_rows():
    rows = []
    for mode in ("f16", "f16x3"):
        for nt in (3, 5, 9):
            for mask in ("logit", "none"):
                dom_c = 32 if mask == "logit" else (18 if mode == "f16" else 20) if nt != 9 else 32
                rows.append(_row(mode, "col2im", "window", 1 if nt == 3 else None, 16, 32, 32, mask, _win_label(nt, mode, mask),
                                 dom_c, nt=nt))
        # two chunks of very different magnitude in the chunked layout; three chunks
        rows.append(_row(mode, "col2im", "window", 1, 16, 32, 64, "logit", _win_label(3, mode, "logit"), 32, chunked=True, nt=3))
        rows.append(_row(mode, "col2im", "window", 1, 16, 32, 96, "logit", _win_label(3, mode, "logit"), 32, nt=3))
    return rows


def _fused_rows():
    rows = []
    for mask in ("logit", "none"):
        dom_c = 32 if mask == "logit" else 20
        for nt in (3, 5, 9):
            rows.append(_row("f16x3", "col2im_fused", "window", 1 if nt == 3 else None, 16, 32, 32, mask,
                             _win_label(nt, "f16x3", mask, True), dom_c, chunked=True, nt=nt, Cout=32))
        rows.append(_row("f16x3", "col2im_fused", "window", 1, 16, 32, 64, mask, _win_label(3, "f16x3", mask, True), dom_c,
                         chunked=True, nt=3, Cout=40))           # dY zero-padded to K = 64
    return rows


ROWS = _cols_rows() + _generic_rows() + _window_rows() + _fused_rows()


# ------------------------------------------------------------------------------------------ geometry
def design(c, B):
    """the designed samples of a row: (class, image, pixel, tap, offset) -- every offset exactly representable in f32.  The first
    writer of a (pixel, tap) keeps it (the tiny maps have fewer slots than samples; `edges` lists what a row must still hold)"""
    H, W = c.H, c.W
    out, taken = [], set()

    def put(cls, b, y, x, tap, dh, dw, inwin=None):
        if not (0 <= y < H and 0 <= x < W) or (b, y, x, tap) in taken:
            return
        taken.add((b, y, x, tap))
        out.append(Sample(cls, b, y, x, tap, float(dh), float(dw), inwin))

    for n, b in enumerate(sorted({0, B - 1})):
        if c.kind == "window":
            # the last sample inside the +-4 margin and the first outside it, at the corner pixels of every tile: tap 0 reaches
            # up / left from the top / left pixels (-4 | -(4 + 2^-10)), tap 8 down / right from the bottom / right pixels
            # (4 - 2^-10 | 4).  Tiles alternate between the inner and the outer value, the last image the other way round
            for ti in range(H // TH):
                for tj in range(W // TW):
                    for ci in (0, 1):
                        for cj in (0, 1):
                            for tap in (0, 8):
                                neg = tap == 0
                                inner = (ti + tj + (0 if neg else 1) + n) % 2 == 0
                                v = (-MG if inner else -(MG + EPS)) if neg else (MG - EPS if inner else MG)
                                edge_h, edge_w = ci == (0 if neg else 1), cj == (0 if neg else 1)   # the pixel lies on that edge
                                both = edge_h == edge_w
                                dh = v if (edge_h or both) else 0.25
                                dw = v if (edge_w or both) else 0.25
                                y, x = ti * TH + ci * (TH - 1), tj * TW + cj * (TW - 1)
                                h, w = y - 1 + tap // 3 + dh, x - 1 + tap % 3 + dw
                                inside = -1 < h < H and -1 < w < W
                                put("window_edge", b, y, x, tap, dh, dw, inside and (inner or not (edge_h or edge_w)))
            # corner (h_low, w_low) of an out-of-window sample above / left of the image: the 30-bit two's-complement index
            put("neg_index", b, 8, 5, 1, -7.5, 0.25, False)
            put("neg_index", b, 5, 16, 3, 0.25, -15.5, False)
            put("neg_index", b, 8, 17, 0, -7.5, -16.5, False)
            for x in range(TW):           # one tile row of one tap: even lanes stay in the window, odd lanes leave it
                put("mixed_wave", b, 3, x, 4, 9.5 if x % 2 else 0.5, 0.25, not x % 2)
        r, q = min(H // 2 + 1, H - 1), min(W // 2 + 1, W - 1)
        put("integer", b, r, q, 4, 0.0, -0.0)
        put("integer", b, r, q, 5, 1.0, -1.0)
        put("top_band", b, 0, q, 1, 0.25, 0.5)
        put("left_band", b, r, 0, 3, 0.5, 0.25)
        put("bottom_band", b, H - 1, q, 7, -0.25, 0.5)
        put("right_band", b, r, W - 1, 5, 0.5, -0.25)
        put("on_minus_one", b, 0, q, 0, 0.0, 0.25)             # h_im = -1 exactly
        put("on_minus_one", b, r, 0, 6, -0.75, 0.0)            # w_im = -1 exactly
        put("on_size", b, H - 1, q, 8, 0.0, -1.25)             # h_im = H exactly
        put("on_size", b, r, W - 1, 2, 0.75, 0.0)              # w_im = W exactly
        y0, x0, y1, x1 = min(2, H - 1), min(3, W - 1), max(H - 3, 0), max(W - 4, 0)
        put("far", b, y0, x0, 2, 9.0, 9.0)                     # another tile
        put("far", b, y0, x0, 6, 40.0, 40.0)                   # outside the image
        put("far", b, y1, x1, 1, -9.0, -9.0)
        put("far", b, y1, x1, 7, -40.0, -40.0)
        put("far", b, 0, 0, 4, H - 1.5, W - 1.5)               # inside the image, in the opposite corner
    return out


def _gen(c, what):
    import zlib
    return torch.Generator().manual_seed(zlib.crc32(repr((what,) + tuple(c[:11])).encode()))


def geometry(c, B):
    """(om [B, H, W, 27 | 18] f32, the designed samples)"""
    g = _gen(c, "om")
    om = torch.randn(B, c.H, c.W, om_channels(c), generator=g)
    om[..., :18] = torch.round(om[..., :18] * 1.5 * 4096.0) / 4096.0
    samples = design(c, B)
    for s in samples:
        om[s.b, s.y, s.x, 2 * s.tap] = s.dh
        om[s.b, s.y, s.x, 2 * s.tap + 1] = s.dw
    return om, samples


PERM_OFFSETS = (-9.0, -5.0, -4.0, -1.0, -0.0, 0.5, 4.0, 5.0, 9.0)


def perm_geometry(c, B):
    """offsets from PERM_OFFSETS only: every bilinear weight is 0, 1/4, 1/2 or 1.  The mask channels (unused by the exact runs'
    NONE mode, all 1 in their PROB mode) are 1"""
    g = _gen(c, "perm")
    om = torch.ones(B, c.H, c.W, om_channels(c))
    pick = torch.randint(0, len(PERM_OFFSETS), (B, c.H, c.W, 18), generator=g)
    om[..., :18] = torch.tensor(PERM_OFFSETS)[pick]
    return om


def positions(om, H, W):
    """(h_im, w_im) [B, H, W, 9] in float64 of every (pixel, tap)"""
    om = om.double()
    taps = torch.arange(9, device=om.device)
    ys = torch.arange(H, device=om.device).view(1, H, 1, 1) - 1 + (taps // 3).view(1, 1, 1, 9)
    xs = torch.arange(W, device=om.device).view(1, 1, W, 1) - 1 + (taps % 3).view(1, 1, 1, 9)
    return ys + om[..., 0:18:2], xs + om[..., 1:18:2]


def classify(c, om):
    """{edge class: bool [B, H, W, 9]} of every (pixel, tap) of a row's geometry, plus "outside" (the sample contributes nothing),
    "inwin" (window rows: inside the image and its four corners inside the tile's LDS window) and "leaves" (inside the image,
    not inwin)"""
    H, W = c.H, c.W
    h, w = positions(om, H, W)
    inside = (h > -1) & (w > -1) & (h < H) & (w < W)
    hl, wl = torch.floor(h), torch.floor(w)
    k = {
        "outside": ~inside,
        "integer": inside & (h == hl) & (w == wl),
        "top_band": (h > -1) & (h < 0) & (w > -1) & (w < W), "left_band": (w > -1) & (w < 0) & (h > -1) & (h < H),
        "bottom_band": (h > H - 1) & (h < H) & (w > -1) & (w < W), "right_band": (w > W - 1) & (w < W) & (h > -1) & (h < H),
        "on_minus_one": (h == -1) | (w == -1), "on_size": (h == H) | (w == W),
        "far": (om[..., 0:18:2].abs() >= 9) | (om[..., 1:18:2].abs() >= 9),
    }
    if c.kind == "window":
        ty0 = (torch.arange(H) // TH * TH).view(1, H, 1, 1)
        tx0 = (torch.arange(W) // TW * TW).view(1, 1, W, 1)
        wr, wc = hl - (ty0 - 1 - MG), wl - (tx0 - 1 - MG)
        inwin = inside & (wr >= 0) & (wr + 1 < TH + 2 + 2 * MG) & (wc >= 0) & (wc + 1 < TW + 2 + 2 * MG)
        leaves = inside & ~inwin
        k["inwin"], k["leaves"] = inwin, leaves
        k["neg_index"] = leaves & ((hl == -1) | (wl == -1))
        k["neg_index_both"] = leaves & (hl == -1) & (wl == -1)
        # the 16 pixels of a tile row that one wave handles, per tap: lanes on both paths
        B = om.shape[0]
        a = inwin.view(B, H, W // TW, TW, 9).any(3, keepdim=True) & leaves.view(B, H, W // TW, TW, 9).any(3, keepdim=True)
        k["mixed_wave"] = a.expand(B, H, W // TW, TW, 9).reshape(B, H, W, 9)
        near = lambda v: ((v.abs() - MG).abs() <= EPS)      # noqa: E731
        k["window_edge"] = near(om[..., 0:18:2].double()) | near(om[..., 1:18:2].double())
    return k


# ------------------------------------------------------------------------------------------ operands
def _grid(shape, g):
    return torch.randint(-256, 257, shape, generator=g).float() / 64.0


def operands(c, B, exact=False):
    """the row's data on the CPU, as the kernel reads it (f16 mode: f16-representable f32): {"x"; "dcol" (col2im) | "dy", "weight"
    (col2im_fused)}.  exact: everything on the 1/64 grid, |v| <= 4.  Two-chunk window rows: chunk 0 of dcol times 2^-10, chunk 1
    times 2^10, and chunk 0 all zero in the last tile"""
    g = _gen(c, "exact" if exact else "data")
    rnd = (lambda *s: _grid(s, g)) if exact else (lambda *s: torch.randn(*s, generator=g))
    r16 = (lambda t: t.half().float()) if c.mode == "f16" else (lambda t: t)
    d = {"x": r16(rnd(B, c.H, c.W, c.Cin))}
    if c.op == "col2im":
        dcol = rnd(B, c.H, c.W, 9, c.Cin)
        if c.kind == "window" and c.Cin == 64 and not exact:
            dcol[..., :32] *= 2.0 ** -10
            dcol[..., 32:] *= 2.0 ** 10
            dcol[B - 1, c.H - TH:, c.W - TW:, :, :32] = 0.0
        dcol = r16(dcol)
        if c.chunked:
            dcol = dcol.view(B, c.H, c.W, 9, c.Cin // 32, 32).permute(0, 1, 2, 4, 3, 5)
        d["dcol"] = dcol.reshape(B, c.H, c.W, 9 * c.Cin).contiguous()
    elif c.op == "col2im_fused":
        K = (c.Cout + 31) // 32 * 32
        d["dy"] = torch.zeros(B, c.H, c.W, K)
        d["dy"][..., :c.Cout] = torch.randn(B, c.H, c.W, c.Cout, generator=g)
        d["weight"] = torch.randn(c.Cout, c.Cin, 3, 3, generator=g) / math.sqrt(c.Cout)
    return d


# ------------------------------------------------------------------------------------------ float64 references
def _mask(om, tap, mask_mode):
    if mask_mode == 2:
        return torch.ones_like(om[..., 0])
    return om[..., 18 + tap] if mask_mode == 1 else torch.sigmoid(om[..., 18 + tap])


def cols_ref(x, om, mask_mode):
    """the sampled columns [B, H, W, 9 * Cin] (tap-major) in f64: oracle.dcnv2_columns, rearranged"""
    B, H, W, Cin = x.shape
    om = om.double().cpu()
    mask = torch.stack([_mask(om, t, mask_mode) for t in range(9)], 1)
    cols, _, _ = O.dcnv2_columns(x.double().cpu().permute(0, 3, 1, 2), om[..., :18].permute(0, 3, 1, 2), mask)
    return cols.view(B, Cin, 9, H, W).permute(0, 3, 4, 2, 1).reshape(B, H, W, 9 * Cin).to(x.device)


def tap_major(dcol, Cin, chunked):
    """dcol [..., 9 * Cin] -> [..., 9, Cin]"""
    lead = dcol.shape[:-1]
    if chunked:
        return dcol.reshape(*lead, Cin // 32, 9, 32).transpose(-3, -2).reshape(*lead, 9, Cin)
    return dcol.reshape(*lead, 9, Cin)


def col2im_ref(dcol, x, om, mask_mode, chunked=False, counts=False):
    """(dx [B, H, W, Cin], dom [B, H, W, 27 | 18]) in f64 from dcol = d(columns) [B, H, W, 9 * Cin]: the scatter as index_add_
    over the four corners, the coordinate and mask gradients of oracle.dcnv2_backward, the logit's gradient through the sigmoid in
    the LOGIT mode.  counts: dx is replaced by the number of contributions that meet in each pixel"""
    B, H, W, Cin = x.shape
    dev = x.device
    x, om = x.double().reshape(-1, Cin), om.double()
    dc = tap_major(dcol.double(), Cin, chunked)
    h_all, w_all = positions(om, H, W)
    dx = torch.zeros(B * H * W, 1 if counts else Cin, dtype=torch.float64, device=dev)
    dom = torch.zeros(B, H, W, 18 if mask_mode == 2 else 27, dtype=torch.float64, device=dev)
    img = (torch.arange(B, device=dev) * H * W).view(B, 1, 1)
    for tap in range(9):
        h, w = h_all[..., tap], w_all[..., tap]
        inside = (h > -1) & (w > -1) & (h < H) & (w < W)
        hl, wl = torch.floor(h), torch.floor(w)
        lh, lw = h - hl, w - wl
        hh, hw = 1 - lh, 1 - lw
        m = _mask(om, tap, mask_mode)
        d = dc[..., tap, :]                                                   # [B, H, W, Cin]
        v = []
        for q, (hq, wq, wt) in enumerate(((hl, wl, hh * hw), (hl, wl + 1, hh * lw), (hl + 1, wl, lh * hw), (hl + 1, wl + 1, lh * lw))):
            ok = inside & (hq >= 0) & (hq <= H - 1) & (wq >= 0) & (wq <= W - 1)
            idx = (img + hq.clamp(0, H - 1).long() * W + wq.clamp(0, W - 1).long()).reshape(-1)
            okf = ok.double().unsqueeze(-1)
            v.append(x[idx].view(B, H, W, Cin) * okf)
            if counts:
                dx.index_add_(0, idx, ok.double().reshape(-1, 1))
            else:
                dx.index_add_(0, idx, ((wt * m).unsqueeze(-1) * okf * d).reshape(-1, Cin))
        dom[..., 2 * tap] = m * (d * (-hw.unsqueeze(-1) * v[0] - lw.unsqueeze(-1) * v[1] + hw.unsqueeze(-1) * v[2]
                                      + lw.unsqueeze(-1) * v[3])).sum(-1)
        dom[..., 2 * tap + 1] = m * (d * (-hh.unsqueeze(-1) * v[0] + hh.unsqueeze(-1) * v[1] - lh.unsqueeze(-1) * v[2]
                                          + lh.unsqueeze(-1) * v[3])).sum(-1)
        if mask_mode != 2:
            bil = (hh * hw).unsqueeze(-1) * v[0] + (hh * lw).unsqueeze(-1) * v[1] + (lh * hw).unsqueeze(-1) * v[2] \
                + (lh * lw).unsqueeze(-1) * v[3]
            gm = (d * bil).sum(-1)
            dom[..., 18 + tap] = gm if mask_mode == 1 else gm * m * (1 - m)
    return dx.view(B, H, W, -1), dom


def fused_dcol(dy, weight):
    """d(columns) = dY . W in f64, chunked column order (c / 32) * 288 + tap * 32 + c % 32"""
    Cout, Cin = weight.shape[:2]
    wm = weight.double().reshape(Cout, Cin // 32, 32, 9).permute(0, 1, 3, 2).reshape(Cout, 9 * Cin)
    return dy.double()[..., :Cout] @ wm.to(dy.device)


def fused_ref(dy, weight, x, om, mask_mode):
    return col2im_ref(fused_dcol(dy, weight), x, om, mask_mode, chunked=True)
