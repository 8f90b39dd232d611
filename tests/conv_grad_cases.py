"""One row per regime of the conv gradient kernels: the weight-gradient kernels of csrc/train_bwd.hip (window, narrow, generic,
the f32 kernel; plain [Cout][tap][Cin] output and the three wg_add layouts of ctdet_conv_wgrad_oihw) and the input-gradient /
conv-transpose paths of ops_train.py (conv_dgrad, ConvTransposeFn), which run forward kernels.

test_conv_grad_host.py replays every weight-gradient row through the library's dry run (no GPU) and asserts the label, split
included, then derives the row's regime facts from label and shape by plain arithmetic; test_conv_grad_gpu.py runs every row
once and compares it with the float64 references below.  A change to a selector threshold or a split formula must move the
affected rows (their shapes), never the regime a row exists for.

The labels assume 256 compute units (the MI355X; what ctdet_device_cu_count() answers outside a GPU process as well).

Row fields
  mode    "f16" | "f32" | "f16x3"
  op      "wgrad" (ops_train.conv_wgrad, plain output) | "wgrad_oihw" (conv_wgrad(into=...): accumulate into the parameter's OIHW
          slot) | "dgrad" (ops_train.conv_dgrad) | "convT" (ops_train.ConvTransposeFn: forward, dX and dW)
  B H W   the conv's input map; Cin -> Cout, k, stride, pad, dil: the conv whose gradient is taken (convT: the transposed conv's
          input map and its Cin -> Cout)
  cin_c / cout_c  channels the tensors carry per pixel (>= Cin / Cout): the 3 -> 8 channel image, the 27 -> 32 offset conv
  label   wgrad rows: the label of the weight-gradient launch; dgrad rows: the label of the forward kernel that computes dX;
          convT rows: the three labels (forward, dX, dW)
  facts   the regime facts the row exists for (checked by the host test)"""
from collections import namedtuple

import torch

Case = namedtuple("Case", "mode op B H W Cin Cout k stride pad dil cin_c cout_c label facts")
MODES = ("f16", "f32", "f16x3")


def out_hw(c):
    span = c.dil * (c.k - 1) + 1
    return (c.H + 2 * c.pad - span) // c.stride + 1, (c.W + 2 * c.pad - span) // c.stride + 1


def case_id(c):
    geo = f"k{c.k}s{c.stride}p{c.pad}" + (f"d{c.dil}" if c.dil > 1 else "")
    cin = f"{c.Cin}" + (f"of{c.cin_c}" if c.cin_c != c.Cin else "")
    cout = f"{c.Cout}" + (f"of{c.cout_c}" if c.cout_c != c.Cout else "")
    label = c.label if isinstance(c.label, str) else c.label[-1]
    return f"{c.mode}-{c.op}-{c.B}x{c.H}x{c.W}-{cin}to{cout}-{geo}-{label}"


def _row(mode, op, label, B, H, W, Cin, Cout, k, stride=1, pad=None, dil=1, cin_c=None, cout_c=None, facts=()):
    pad = k // 2 if pad is None else pad
    facts = (facts,) if isinstance(facts, str) else tuple(facts)
    return Case(mode, op, B, H, W, Cin, Cout, k, stride, pad, dil, cin_c or Cin, cout_c or Cout, label, facts)


def _wg(mode, kind, n):
    """label of a weight-gradient launch of the f16 / f16x3 launcher"""
    if kind == "win":
        return f"conv_wgrad_win_kernel<{mode}>,split={n}"
    if kind in ("7x7,Cin8", "3x3,Cin16"):
        return f"conv_wgrad_narrow_kernel<{kind},{mode}>,blocks={n}"
    return f"conv_wgrad_kernel<{mode}{',oihw' if kind == 'oihw' else ''}>,split={n}"


def _f32(n):
    return f"conv_wgrad_f32_kernel,split={n}"


def _wgrad_rows(mode):
    """the weight-gradient rows the f16 and f16x3 modes share (x and dY dense)"""
    w = lambda kind, n, *a, **kw: _row(mode, "wgrad", _wg(mode, kind, n), *a, **kw)      # noqa: E731
    return [
        # ---- window kernel: 8 x 32-pixel tiles, 32 cin x 32 cout per workgroup, split = min(256 / (gx * gy), tiles)
        w("win", 4, 1, 16, 64, 32, 27, 3, cout_c=32, facts=("tiles=4", "tiles_per_wg=1", "partial_cout_tile", "halo_all_sides")),
        w("win", 8, 2, 16, 64, 64, 64, 3, facts=("swizzle", "tiles_per_wg=1", "halo_all_sides")),
        w("win", 4, 2, 16, 64, 256, 256, 3, facts=("tiles_per_wg=2", "halo_all_sides")),
        w("win", 4, 1, 16, 96, 256, 256, 3, facts=("tiles=6", "tiles_per_wg=2", "empty_wg", "middle_tile_column")),
        w("win", 9, 3, 24, 32, 96, 40, 3, facts=("second_cout_tile_partial", "tiles_per_wg=1")),
        # ---- narrow kernels (Cout <= 16): blocks = min(256, tiles)
        w("7x7,Cin8", 8, 2, 16, 64, 8, 16, 7, facts="tiles_per_wg=1"),
        w("3x3,Cin16", 8, 2, 16, 64, 16, 16, 3, facts="tiles_per_wg=1"),
        w("3x3,Cin16", 3, 3, 8, 32, 16, 8, 3, facts="tiles_per_wg=1"),
        w("7x7,Cin8", 256, 1, 264, 256, 8, 16, 7, facts=("tiles=264", "tiles_per_wg=2", "empty_wg")),
        # ---- generic kernel: 128 k x 64 cout per workgroup, 64-pixel K steps, split = min(1024 / (gx * gy), ceil(M / 256))
        w("plain", 8, 1, 45, 45, 24, 72, 3, facts=("swizzle", "last_range=233", "ragged_last_range", "partial_k_tile",
                                                    "partial_cout_tile", "div_index")),
        w("plain", 2, 2, 32, 32, 16, 32, 3, stride=2, facts=("pow2_index", "split=2")),
        w("plain", 6, 3, 19, 23, 32, 64, 3, facts=("no_swizzle", "last_range=31", "ragged_last_range", "div_index")),
        w("plain", 1, 1, 8, 8, 576, 64, 1, facts="single_k_step"),
        w("plain", 2, 2, 12, 12, 32, 32, 3, pad=2, dil=2, facts=("dilation", "ragged_last_range")),
        # the conv-transpose weight gradient: "x" is the up-convolution's dY (2x14x10x24), "dY" its input (2x7x5x16)
        w("plain", 1, 2, 14, 10, 24, 16, 4, stride=2, pad=1, facts=("taps=16", "stride2", "div_index")),
    ]


def _oihw_rows(mode):
    """accumulate (scale 0.5) into an OIHW slot that already holds values; x and dY are channel slices of wider buffers"""
    f32 = mode == "f32"
    w = lambda kind, n, nf, *a, **kw: _row(mode, "wgrad_oihw", _f32(nf) if f32 else _wg(mode, kind, n), *a, **kw)   # noqa: E731
    return [
        w("oihw", 2, 8, 2, 12, 20, 256, 80, 1, facts="layout_1x1"),
        w("oihw", 2, 5, 2, 10, 14, 64, 48, 3, facts="layout_rxs"),
        w("7x7,Cin8", 8, 32, 2, 16, 64, 3, 16, 7, cin_c=8, facts=("layout_rxs", "cin_dropped")),
        w("win", 4, 16, 1, 16, 64, 32, 27, 3, cout_c=32, facts=("layout_rxs", "cout_dropped")),
    ]


def _f32_rows():
    w = lambda n, *a, **kw: _row("f32", "wgrad", _f32(n), *a, **kw)      # noqa: E731
    return [
        # split = min(4096 / (ceil(K / 16) * ceil(Cout / 16)), ceil(M / 64)); 16-pixel steps inside a range of ceil(M / split)
        w(32, 2, 16, 64, 4, 16, 7, facts="k_tail"),                         # K = 196
        w(2, 2, 15, 9, 16, 28, 3, stride=2, facts=("cout_tail", "range_tail")),  # Ho x Wo = 8 x 5, M = 80
        w(21, 3, 19, 23, 64, 32, 1, facts="range_tail"),                    # M = 1311: 20 ranges of 63 pixels and one of 51
        w(32, 2, 16, 64, 32, 64, 3),
        w(56, 4, 16, 64, 32, 64, 3, facts=("split_from_blocks", "range_tail")),   # 4096 / (18 * 4) = 56 < ceil(M / 64) = 64
        w(2, 2, 14, 10, 24, 16, 4, stride=2, pad=1, facts=("taps=16", "stride2", "range_tail")),
        w(5, 2, 12, 12, 32, 32, 3, pad=2, dil=2, facts=("dilation", "range_tail")),
    ]


def _fwd(mode, f16_label, f32_label, x3_label):
    return {"f16": f16_label, "f32": f32_label, "f16x3": x3_label}[mode]


def _dgrad_rows(mode):
    """input gradients: the label is the forward kernel's that computes dX.  In / out channel counts differ, so a transposition
    error shows"""
    d = lambda labels, *a, **kw: _row(mode, "dgrad", _fwd(mode, *labels), *a, **kw)      # noqa: E731
    rows = [
        # 3x3 / s1 / p1 on the transposed, flipped pack: dX = conv(dY [64 ch], 32 rows)
        d(("conv_igemm_uk_kernel<128x32,conv,f16>", "conv_f32_uk_kernel<128x32>", "conv_f16x3_uk_kernel<128x32>"),
          2, 9, 13, 32, 64, 3, facts="flipped_taps"),
        d(("conv3x3_halo_tap2_kernel<256x32,f16>", "conv_f32_uk_kernel<128x32>", "conv3x3_halo_pair2_kernel<256x32,f16x3>"),
          1, 16, 64, 32, 64, 3, facts="flipped_taps"),
        d(("conv_igemm_uk_kernel<128x64,conv,f16>", "conv_f32_uk_kernel<128x64>", "conv_f16x3_uk_kernel<128x64>"),
          3, 19, 23, 64, 32, 1, pad=0),
        # 3x3 / s2 / p1: the four-phase 2x2 conv + depth_to_space2 (f16, f16x3), zero-stuffed dY (f32); the odd map gives
        # Ho x Wo = 8 x 5 and phases that are cut at the bottom / right edge
        d(("conv_igemm_uk_kernel<128x64,conv,f16>", "conv_f32_mfma_kernel<256x16>", "conv_f16x3_uk_kernel<128x64>"),
          2, 20, 20, 16, 32, 3, stride=2, facts=("phases" if mode != "f32" else "in_dil")),
        d(("conv_igemm_uk_kernel<128x64,conv,f16>", "conv_f32_mfma_kernel<256x16>", "conv_f16x3_uk_kernel<128x64>"),
          2, 15, 9, 16, 32, 3, stride=2, facts=("phases" if mode != "f32" else "in_dil", "odd_map")),
        # 1x1 / s2 / p0, the ResNet shortcut: dY read as zero-stuffed by the generic kernels' gather
        d(("conv_igemm_dma_kernel<128x64,f16>", "conv_f32_mfma_kernel<128x64>", "conv_f16x3_mfma_kernel<128x64>"),
          1, 16, 16, 64, 128, 1, stride=2, pad=0, facts="in_dil"),
        d(("conv_igemm_dma_kernel<128x64,f16>", "conv_f32_mfma_kernel<128x64>", "conv_f16x3_mfma_kernel<128x64>"),
          2, 15, 9, 64, 128, 1, stride=2, pad=0, facts=("in_dil", "odd_map")),
    ]
    if mode == "f16x3":     # dY's channel count is no multiple of 16: the zero-stuffed form instead of the four phases
        rows.append(d((None, None, "conv_f16x3_mfma_kernel<256x16>"), 2, 15, 9, 16, 24, 3, stride=2, facts=("in_dil", "odd_map")))
    if mode != "f32":       # the offset conv: dY carries 32 channels for 27 couts, the operand gets zero columns (cin_pad)
        rows.append(d(("conv_igemm_uk_kernel<128x64,conv,f16>", None, "conv_f16x3_uk_kernel<128x64>"),
                      2, 9, 13, 64, 27, 3, cout_c=32, facts=("flipped_taps", "cin_pad")))
    return rows


def _convt_rows(mode):
    """ConvTransposeFn, 4x4 / s2 / p1 on 2x7x5 -> 2x14x10: (forward, dX, dW) labels; 29 couts are carried in 32 channels"""
    f32 = mode == "f32"
    t = lambda labels, dw, *a, **kw: _row(mode, "convT", _fwd(mode, *labels) + (dw,), *a, **kw)      # noqa: E731
    return [
        t((("conv_igemm_dma_kernel<128x32,f16>", "conv_igemm_uk_kernel<128x64,conv,f16>"),
           ("conv_f32_mfma_kernel<128x32>", "conv_f32_uk_kernel<128x64>"),
           ("conv_f16x3_mfma_kernel<128x32>", "conv_f16x3_uk_kernel<128x64>")),
          _f32(2) if f32 else _wg(mode, "plain", 1), 2, 7, 5, 64, 32, 4, stride=2, pad=1),
        t((("conv_igemm_dma_kernel<128x32,f16>", "conv_igemm_uk_kernel<128x64,conv,f16>"),
           ("conv_f32_mfma_kernel<128x32>", "conv_f32_uk_kernel<128x64>"),
           ("conv_f16x3_mfma_kernel<128x32>", "conv_f16x3_uk_kernel<128x64>")),
          _f32(2) if f32 else _wg(mode, "plain", 1), 2, 7, 5, 64, 29, 4, stride=2, pad=1, cout_c=32, facts="cout_carried"),
    ]


ROWS = (_wgrad_rows("f16") + _wgrad_rows("f16x3") + _f32_rows()
        + [r for m in MODES for r in _oihw_rows(m)]
        + [r for m in MODES for r in _dgrad_rows(m)]
        + [r for m in MODES for r in _convt_rows(m)])

# the label families of the weight-gradient launchers: each must have a row in f16 and in f16x3 (the f32 kernel: in f32)
WGRAD_FAMILIES = ("conv_wgrad_narrow_kernel<7x7,Cin8,{m}>", "conv_wgrad_narrow_kernel<3x3,Cin16,{m}>", "conv_wgrad_win_kernel<{m}>",
                  "conv_wgrad_kernel<{m}>", "conv_wgrad_kernel<{m},oihw>")
F32_FAMILY = "conv_wgrad_f32_kernel"


# ------------------------------------------------------------------------------------------ work split of a labelled launch
def label_split(label):
    """(kernel family, the split / blocks value the launcher computed)"""
    fam, n = label.rsplit(",", 1)
    key, val = n.split("=")
    assert key in ("split", "blocks"), label
    return fam, int(val)


def kernel_kind(c):
    """which weight-gradient kernel a wgrad row's label names: "win" | "narrow" | "generic" | "f32" """
    fam = label_split(c.label if isinstance(c.label, str) else c.label[-1])[0]
    for kind, s in (("win", "_win_"), ("narrow", "_narrow_"), ("f32", "_f32_")):
        if s in fam:
            return kind
    return "generic"


def wgrad_geometry(c):
    """(x map H, W and channels; dY map Ho, Wo and channels) of the weight-gradient launch of a wgrad / wgrad_oihw row"""
    Ho, Wo = out_hw(c)
    return (c.H, c.W, c.cin_c), (Ho, Wo, c.cout_c)


def pixel_ranges(c):
    """the [begin, end) ranges of dY pixels (generic, f32) or of 8 x 32-pixel tiles (win, narrow) the workgroups of the row's
    launch walk, as the kernels derive them from the split the label states -- empty ranges included"""
    kind = kernel_kind(c)
    n = label_split(c.label if isinstance(c.label, str) else c.label[-1])[1]
    Ho, Wo = out_hw(c)
    if kind in ("win", "narrow"):
        total = c.B * (c.H // 8) * (c.W // 32)
        per = -(-total // n)
    else:
        total = c.B * Ho * Wo
        per = -(-total // n)
        if kind == "generic":
            per = -(-per // 64) * 64
    return [(min(i * per, total), min(i * per + per, total)) for i in range(n)], total


def seam_pixels(c):
    """dY pixel indices (b * Ho + ho) * Wo + wo where a weight-gradient kernel could drop, repeat or misplace a pixel: the four
    corners of the first and last image, pixel M - 1, and per kernel kind
      generic: the first and last pixel of every workgroup's range and of every 64-pixel K step inside it
      f32:     the first and last pixel of every range and of the last (partial) 16-pixel step of every range
      win / narrow: the four corners of every tile (so also of the first and last tile of every workgroup's range)"""
    Ho, Wo = out_hw(c)
    M = c.B * Ho * Wo
    px = []
    for b in (0, c.B - 1):
        for ho in (0, Ho - 1):
            for wo in (0, Wo - 1):
                px.append((b * Ho + ho) * Wo + wo)
    px.append(M - 1)
    kind = kernel_kind(c)
    ranges, _ = pixel_ranges(c)
    if kind in ("win", "narrow"):
        ty, tx = c.H // 8, c.W // 32
        for tile in range(c.B * ty * tx):
            txi, tyi, b = tile % tx, tile // tx % ty, tile // (tx * ty)
            for ho in (8 * tyi, 8 * tyi + 7):
                for wo in (32 * txi, 32 * txi + 31):
                    px.append((b * Ho + ho) * Wo + wo)
    else:
        step = 64 if kind == "generic" else 16
        for lo, hi in ranges:
            if lo >= hi:
                continue
            px += [lo, hi - 1]
            if kind == "generic":
                for m in range(lo, hi, step):
                    px += [m, min(m + step, hi) - 1]
            else:
                px.append(lo + (hi - 1 - lo) // step * step)
    seen, out = set(), []
    for m in px:
        assert 0 <= m < M, (c, m)
        if m not in seen:
            seen.add(m)
            out.append(m)
    return out


# ------------------------------------------------------------------------------------------ float64 references
def wgrad_ref(x, dy, k, s, p, dil=1):
    """dW [Cout, k, k, Cin] of y = conv(x, W) in f64: one [Cout, M] @ [M, Cin] product per tap on shifted views of x"""
    B, H, W, Cin = x.shape
    _, Ho, Wo, Cout = dy.shape
    xp = torch.nn.functional.pad(x.double(), (0, 0, p, p, p, p))
    d = dy.double().reshape(-1, Cout).t()
    ref = torch.empty(Cout, k, k, Cin, dtype=torch.float64, device=x.device)
    for r in range(k):
        for c in range(k):
            ref[:, r, c] = d @ xp[:, r * dil:r * dil + s * Ho:s, c * dil:c * dil + s * Wo:s, :].reshape(-1, Cin)
    return ref


def dgrad_ref(dy, w, s, p, H, W):
    """dX [B, H, W, Cin] in f64: every tap's dY @ W_tap added into the padded input at its shifted (strided) positions"""
    B, Ho, Wo, Cout = dy.shape
    Cin, k = w.shape[1], w.shape[2]
    d = dy.double().reshape(-1, Cout)
    w = w.double()
    dxp = torch.zeros(B, H + 2 * p, W + 2 * p, Cin, dtype=torch.float64, device=dy.device)
    for r in range(k):
        for c in range(k):
            dxp[:, r:r + s * Ho:s, c:c + s * Wo:s, :] += (d @ w[:, :, r, c]).view(B, Ho, Wo, Cin)
    return dxp[:, p:p + H, p:p + W, :]


def conv_ref(x, w, s, p):
    """y [B, Ho, Wo, Cout] = conv(x, w [Cout, Cin, k, k]) in f64: one [M, Cin] @ [Cin, Cout] product per tap"""
    B, H, W, Cin = x.shape
    Cout, k = w.shape[0], w.shape[2]
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    xp = torch.nn.functional.pad(x.double(), (0, 0, p, p, p, p))
    w = w.double()
    y = torch.zeros(B * Ho * Wo, Cout, dtype=torch.float64, device=x.device)
    for r in range(k):
        for c in range(k):
            y += xp[:, r:r + s * Ho:s, c:c + s * Wo:s, :].reshape(-1, Cin) @ w[:, :, r, c].t()
    return y.view(B, Ho, Wo, Cout)


def conv_transpose_refs(x, w, dy, s, p):
    """(y, dX, dW) in f64 of y = conv_transpose2d(x [B, H, W, Cin], w [Cin, Cout, k, k]) (output_padding 0) for the output
    gradient dy: the transposed conv is the input gradient of the plain conv with the same weight read as [out = Cin][in = Cout]"""
    k = w.shape[2]
    Ho, Wo = (x.shape[1] - 1) * s - 2 * p + k, (x.shape[2] - 1) * s - 2 * p + k
    y = dgrad_ref(x, w, s, p, Ho, Wo)
    dx = conv_ref(dy, w, s, p)
    dw = wgrad_ref(dy, x, k, s, p).permute(0, 3, 1, 2)            # [Cin, k, k, Cout] -> [Cin, Cout, k, k]
    return y, dx, dw


def impulse_patches(x, c, pixels):
    """[len(pixels), k, k, C]: the zero-padded k x k patch of x (NHWC, the conv's input) that the taps of output pixel m read,
    for every m of `pixels` -- row n of dW when dY's channel n is 1.0 at that pixel and zero elsewhere"""
    Ho, Wo = out_hw(c)
    B, H, W, Cc = x.shape
    out = torch.zeros(len(pixels), c.k, c.k, Cc, dtype=x.dtype)
    for i, m in enumerate(pixels):
        wo, ho, b = m % Wo, m // Wo % Ho, m // (Wo * Ho)
        for r in range(c.k):
            hi = ho * c.stride - c.pad + r * c.dil
            if not 0 <= hi < H:
                continue
            for s in range(c.k):
                wi = wo * c.stride - c.pad + s * c.dil
                if 0 <= wi < W:
                    out[i, r, s] = x[b, hi, wi]
    return out
