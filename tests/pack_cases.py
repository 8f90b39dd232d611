"""Oracle and case table of the weight-packing kernels (csrc/pointwise.hip: pack_weights_kernel, pack_weights_batch_kernel,
pack3_kernel, pack3_batch_kernel; csrc/conv_f32.hip: split_weights_kernel).  Numpy only.

Index map (pack_value / pack_value_loop, pack_image): written from the layout comments of pointwise.hip and ctdet_hip.h, once
as one index computation per element and once by permuting, padding and reshaping whole arrays; tests/test_pack_host.py holds
the two against each other.
    transposed 0   rows = O, channels = I:               w[row][c][r][s]
    transposed 1   rows = I, channels = O, taps flipped: w[c][row][R-1-r][S-1-s]        (the input-gradient operand)
    transposed 2   rows = tap*I + c,                      k = o: w[o][c][tap]            (DCNv2 d(columns), tap-major rows)
    transposed 3   rows = (c/32)*288 + tap*32 + c%32,     k = o: w[o][c][tap]            (... chunk-major rows)
    korder 0       k = tap*chans_pad + c,  tap = r*S + s
    korder 1       k = ((c/32)*R*S + tap)*32 + c%32
    zero outside rows, taps and channels.

f16 image: the f32 image rounded to nearest even (numpy's float16 cast; `(f16)float` on the device).

f16x3 row rule (the specification of pack3_row):
    amax = max |row| over the real elements;  (m, ex) = frexp(amax);  sh = min(11 - ex, 126);  pw = 2^sh, scale = 2^-sh
    (amax == 0, a row of +-0 or of padding: pw = scale = 1);  v = f32(pw * w), exact whenever it is finite and normal;
    hi = f16(v), lo = f16(f32(v - f32(hi))).
The cap keeps pw and its inverse normal f32 numbers: a row with amax < 2^-116 is scaled by 2^126 only, its largest element lands
below 1024, and scale_out stays the exact inverse.  Rows with amax >= 2^-116 are scaled into [1024, 2048).

Reconstruction: |v| < 2048, so hi is v rounded to a multiple of at most 1 and |v - hi| <= 0.5, exactly an f32; rounding that
residual to f16 costs at most half an ulp of [0.25, 0.5], 2^-13, and at most 2^-25 where the residual is an f16 subnormal:
|hi + lo - v| <= 2^-13 in scaled units, 2^-23 of the row maximum for every row that the cap does not touch.

Cases: every row of X3_CASES / F16_CASES is named for the edge it is there for, and `expect` says which property of the case
makes it that edge (test_pack_host.py asserts each, so a change of the table cannot silently empty it).  The DCNv2 operands have
9*I packed rows by construction; every other case has at most 64."""
import zlib
from collections import namedtuple

import numpy as np

F32_MAX = np.float32(np.finfo(np.float32).max)
SHIFT_CAP = 126
RECON_BOUND = 2.0 ** -13           # |hi + lo - v|, scaled units
RECON_REL = 2.0 ** -23             # ... relative to the row maximum, rows that the cap leaves alone


def f32(x):
    return np.float32(x)


def pow2(e):
    return np.ldexp(np.float32(1.0), int(e)).astype(np.float32)


def below(x):
    """the f32 next to x towards zero"""
    return np.nextafter(np.float32(x), np.float32(0.0))


# ------------------------------------------------------------------------------------------------ index map
def packed_dims(O, I, R, S, transposed):
    """(rows, chans, taps) of the packed operand: real rows, real channels per tap, taps"""
    if transposed >= 2:
        return 9 * I, O, 1
    return (I, O, R * S) if transposed else (O, I, R * S)


def pack_value_loop(w, O, I, R, S, chans_pad, korder, transposed, row, k):
    """element (row, k) of the packed operand, one index computation (plain Python integers)"""
    w = np.asarray(w, dtype=np.float32)
    if transposed >= 2:                                   # the weight is [O, I, 3, 3]; R, S play no part
        if row >= 9 * I or k >= O:
            return np.float32(0.0)
        if transposed == 2:
            tap, c = divmod(row, I)
        else:
            chunk, rem = divmod(row, 288)
            tap, c32 = divmod(rem, 32)
            c = chunk * 32 + c32
        return w.reshape(O, I, 9)[k, c, tap]
    rows, chans, taps = packed_dims(O, I, R, S, transposed)
    if korder == 0:
        tap, c = divmod(k, chans_pad)
    else:
        chunk, rem = divmod(k, taps * 32)
        tap, c32 = divmod(rem, 32)
        c = chunk * 32 + c32
    if row >= rows or tap >= taps or c >= chans:
        return np.float32(0.0)
    r, s = divmod(tap, S)
    if not transposed:
        return w[row, c, r, s]
    return w[c, row, R - 1 - r, S - 1 - s]


def pack_image(w, O, I, R, S, chans_pad, rows_pad, Kpad, korder, transposed):
    """the whole f32 image [rows_pad, Kpad] by array operations: permute to [rows, taps, channels], pad, reorder, pad"""
    w = np.asarray(w, dtype=np.float32)
    if transposed >= 2:
        m = w.reshape(O, I, 9)
        if transposed == 2:
            m = m.transpose(2, 1, 0).reshape(9 * I, O)                           # [tap, c] rows
        else:
            m = m.reshape(O, I // 32, 32, 9).transpose(1, 3, 2, 0).reshape(9 * I, O)   # [chunk, tap, c % 32] rows
    else:
        if transposed:
            w = w[:, :, ::-1, ::-1].transpose(1, 0, 2, 3)
        rows, chans = w.shape[0], w.shape[1]
        t = w.reshape(rows, chans, R * S).transpose(0, 2, 1)                     # [rows, tap, c]
        t = np.concatenate([t, np.zeros((rows, R * S, chans_pad - chans), np.float32)], axis=2)
        if korder == 1:
            t = t.reshape(rows, R * S, chans_pad // 32, 32).transpose(0, 2, 1, 3)
        m = t.reshape(rows, R * S * chans_pad)
    img = np.zeros((rows_pad, Kpad), np.float32)
    img[:m.shape[0], :m.shape[1]] = m
    return img


def pack_value(w, O, I, R, S, chans_pad, korder, transposed, row, k):
    """element(s) (row, k) of the packed operand; row and k may be arrays (the vectorised form reads the array-built image)"""
    rows, chans, taps = packed_dims(O, I, R, S, transposed)
    row, k = np.asarray(row), np.asarray(k)
    rows_pad = max(int(row.max()) + 1, rows)
    Kpad = max(int(k.max()) + 1, (chans_pad if transposed >= 2 else taps * chans_pad))
    return pack_image(w, O, I, R, S, chans_pad, rows_pad, Kpad, korder, transposed)[row, k]


def pack_image_loop(w, O, I, R, S, chans_pad, rows_pad, Kpad, korder, transposed):
    out = np.empty((rows_pad, Kpad), np.float32)
    for row in range(rows_pad):
        for k in range(Kpad):
            out[row, k] = pack_value_loop(w, O, I, R, S, chans_pad, korder, transposed, row, k)
    return out


def f16_image(w, O, I, R, S, chans_pad, rows_pad, Kpad, korder, transposed):
    """uint16 bits [rows_pad, Kpad] of the f16 operand"""
    with np.errstate(over="ignore"):
        return pack_image(w, O, I, R, S, chans_pad, rows_pad, Kpad, korder, transposed).astype(np.float16).view(np.uint16)


# ------------------------------------------------------------------------------------------------ f16x3 rule
def row_shift(amax):
    """sh of the row rule for an array of row maxima (0 for amax == 0)"""
    amax = np.asarray(amax, dtype=np.float32)
    _, ex = np.frexp(amax)
    return np.where(amax > 0, np.minimum(11 - ex, SHIFT_CAP), 0).astype(np.int64)


def split(v):
    """(hi, lo) f16 of an f32 array: hi = f16(v), lo = f16(f32(v - f32(hi)))"""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = v.astype(np.float16)
        lo = (v - hi.astype(np.float32)).astype(np.float32).astype(np.float16)
    return hi, lo


def x3_rows(img):
    """img: tap-major f32 image [rows_pad, K] (korder 0, padding included) -> (v, hi, lo, pw, scale, sh, amax) per the row rule"""
    img = np.asarray(img, dtype=np.float32)
    amax = np.abs(img).max(axis=1) if img.shape[1] else np.zeros(img.shape[0], np.float32)
    sh = row_shift(amax)
    pw = np.ldexp(np.float32(1.0), sh).astype(np.float32)
    scale = np.ldexp(np.float32(1.0), -sh).astype(np.float32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        v = (pw[:, None] * img).astype(np.float32)
    hi, lo = split(v)
    return v, hi, lo, pw, scale, sh, amax


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float16).view(np.uint16)


def _grouped(hi, lo, Kpad, n):
    """tap-major image, every group of n k = {hi[n], lo[n]}"""
    rows, K = hi.shape
    h = np.zeros((rows, Kpad), np.float16)
    l = np.zeros((rows, Kpad), np.float16)
    h[:, :K], l[:, :K] = hi, lo
    g = np.stack([h.reshape(rows, Kpad // n, n), l.reshape(rows, Kpad // n, n)], axis=2)     # [row, group, hi/lo, n]
    return _bits(g.reshape(rows, 2 * Kpad))


def _step(x, ta, ca, tb, cb):
    """64 halves of one 128-byte step: X from hi, Y from lo; each = for q in 0..3 {a[4q..4q+3], b[4q..4q+3]} with a / b the
    16 channels from ca / cb of tap ta / tb.  x: (hi, lo) as [rows, 10 taps, chans]"""
    parts = []
    for p in x:
        a = p[:, ta, ca:ca + 16].reshape(-1, 4, 1, 4)
        b = p[:, tb, cb:cb + 16].reshape(-1, 4, 1, 4)
        parts.append(np.concatenate([a, b], axis=2).reshape(-1, 32))
    return np.concatenate(parts, axis=1)


def x3_image(w, O, I, R, S, chans_pad, rows_pad, Kpad, layout, transposed, scale_n):
    """(uint16 bits [rows_pad, 2*Kpad], f32 scale [scale_n]) of ctdet_pack_weights_x3"""
    K = chans_pad if transposed >= 2 else R * S * chans_pad
    _, hi, lo, _, scale, _, _ = x3_rows(pack_image(w, O, I, R, S, chans_pad, rows_pad, K, 0, transposed))
    if layout == 0:
        img = _grouped(hi, lo, Kpad, 4)
    elif layout == 5:
        img = _grouped(hi, lo, Kpad, 8)
    else:
        assert R * S == 9 and transposed < 2
        x = []
        for p in (hi, lo):                                   # [rows, 10 taps, chans]: the tenth tap is zero
            t = np.zeros((rows_pad, 10, chans_pad), np.float16)
            t[:, :9] = p.reshape(rows_pad, 9, chans_pad)
            x.append(t)
        steps = []
        if layout == 3:
            for cp in range(chans_pad // 32):
                A, B = 32 * cp, 32 * cp + 16
                steps += [_step(x, 2 * s, A, 2 * s + 1, A) for s in range(4)]
                steps.append(_step(x, 8, A, 8, B))
                steps += [_step(x, 2 * s, B, 2 * s + 1, B) for s in range(4)]
        else:
            assert layout == 2
            for ch in range(chans_pad // 16):
                steps += [_step(x, 2 * s, 16 * ch, 2 * s + 1, 16 * ch) for s in range(5)]
        img = _bits(np.concatenate(steps, axis=1))
    assert img.shape == (rows_pad, 2 * Kpad), (img.shape, rows_pad, Kpad)
    return img, scale[:scale_n].copy()


def x3_kpad(case, layout):
    """Kpad of a case in one layout: the pair layouts fix it"""
    if layout == 3:
        return case.chans_pad // 32 * 288
    if layout == 2:
        return case.chans_pad // 16 * 160
    return case.Kpad


# ------------------------------------------------------------------------------------------------ weights
# a plant: (packed row, tap-major position k of the maximum or None, value of the maximum, how the rest of the row is filled)
#   "ordinary"  f32(u * |max|), u uniform in [-0.9, 0.9]          "const"  every element = the value (k is None)
#   "tiny"      neighbours of magnitude 2^-31 .. 2^-29 and a few 1e-38: they underflow when the row is scaled down
Plant = namedtuple("Plant", "row k value fill")


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def ordinary_weight(name, shape):
    g = _rng(name)
    return (g.standard_normal(shape) * 0.3 * g.uniform(0.05, 1.0, (shape[0], 1, 1, 1))).astype(np.float32)


def plant_row(w, p, g):
    """write plant p into the forward operand's row p.row of w [O, I, R, S] (tap-major position k = tap*I + c)"""
    O, I, R, S = w.shape
    K = I * R * S
    if p.fill == "const":
        vec = np.full(K, p.value, np.float32)
    else:
        mag = np.abs(np.float32(p.value))
        if p.fill == "ordinary":
            with np.errstate(under="ignore"):
                vec = (g.uniform(-0.9, 0.9, K).astype(np.float32) * mag).astype(np.float32)
        else:
            vec = (g.choice([-1.0, 1.0], K) * np.ldexp(g.uniform(1.0, 2.0, K), g.integers(-31, -29, K))).astype(np.float32)
            vec[3::17] = np.float32(1e-38) * g.choice([-1.0, 1.0], len(vec[3::17])).astype(np.float32)
        vec[p.k] = p.value
    w[p.row] = vec.reshape(R * S, I).T.reshape(I, R, S)


X3Case = namedtuple("X3Case", "name O I R S chans_pad rows_pad Kpad layouts transposed scale_n plants expect")


def _x3(name, O, I, R, S, chans_pad, rows_pad, Kpad, layouts, transposed=0, scale_n=None, plants=(), **expect):
    return X3Case(name, O, I, R, S, chans_pad, rows_pad, Kpad, tuple(layouts), transposed,
                  rows_pad if scale_n is None else scale_n, tuple(plants), expect)


def _content(name, plants, **expect):
    """a row-content case: [8, 32, 3, 3] forward (K = 288: the amax loop takes two passes, four waves own red[0..3])"""
    return _x3(name, 8, 32, 3, 3, 32, 8, 288, (0, 5, 3, 2), plants=plants, **expect)


def _max_at(k):
    return _content(f"max_at_k{k}", [Plant(2, k, f32(3.0), "ordinary")], amax_pos={2: k}, K=288)


POW2_EXPONENTS = (-20, -1, 0, 1, 10, 11, 100)       # rows 0..6; row 7 stays ordinary

X3_CASES = [
    # ---- shapes
    _x3("k_below_256", 6, 8, 3, 3, 8, 8, 72, (0, 5), K=72, K_lt=256),
    _x3("k288_second_amax_pass", 8, 32, 3, 3, 32, 8, 288, (0, 5, 3, 2), K=288, K_gt=256),
    _x3("layout0_group_loop_wraps", 4, 128, 3, 3, 128, 4, 1152, (0,), groups4=288),
    _x3("layout3_288_pieces", 4, 128, 3, 3, 128, 32, 1152, (3,), scale_n=4, pieces3=288),
    _x3("layout3_one_chunk_pair", 5, 32, 3, 3, 32, 32, 288, (3,), scale_n=8, pieces3=72, chunk_pairs=1),
    _x3("layout2_seven_chunks", 4, 112, 3, 3, 112, 32, 1008, (2,), scale_n=4, pieces2=280, chunks=7),
    _x3("layout2_one_chunk", 12, 16, 3, 3, 16, 32, 144, (2, 0), scale_n=12, pieces2=40, chunks=1),
    _x3("layout5_288_groups", 8, 256, 3, 3, 256, 8, 2304, (5,), K=2304, groups8=288),
    _x3("dcn_cols_tap_major_i32", 48, 32, 1, 1, 64, 320, 64, (0, 5), transposed=2, rows=288, chans=48, rows_pad_gt_rows=True),
    _x3("dcn_cols_chunk_major_i32", 48, 32, 1, 1, 64, 288, 64, (0, 5), transposed=3, rows=288, chans=48, chans_pad_gt_chans=True),
    _x3("dcn_cols_tap_major_i64", 48, 64, 1, 1, 64, 576, 64, (0, 5), transposed=2, rows=576),
    _x3("dcn_cols_chunk_major_i64", 48, 64, 1, 1, 64, 576, 64, (0, 5), transposed=3, rows=576, scale_n=576),
    _x3("stem_7x7_three_channels", 16, 3, 7, 7, 8, 16, 400, (0, 5), K=392, chans=3, chans_pad_gt_chans=True, Kpad_gt_K=True),
    _x3("one_by_one", 10, 20, 1, 1, 20, 16, 24, (0, 5), scale_n=12, K=20, Kpad_gt_K=True),
    _x3("non_square_3x1", 7, 16, 3, 1, 16, 8, 48, (0, 5), K=48),
    _x3("non_square_2x3_input_gradient", 7, 12, 2, 3, 8, 12, 48, (0, 5), transposed=1, rows=12, chans=7, chans_pad_gt_chans=True),
    _x3("rows_not_a_multiple_of_4", 6, 8, 3, 3, 8, 16, 72, (0, 5), rows=6, rows_pad_gt_rows=True),
    _x3("chans_pad_above_chans", 8, 24, 3, 3, 32, 8, 288, (0, 5, 3, 2), chans=24, chans_pad_gt_chans=True),
    _x3("kpad_above_k", 8, 8, 3, 3, 8, 8, 96, (0, 5), K=72, Kpad_gt_K=True),
    _x3("scale_n_below_rows_pad", 8, 8, 3, 3, 8, 32, 72, (0, 5), scale_n=5, scale_n_lt_rows_pad=True),
    _x3("scale_n_zero", 8, 8, 3, 3, 8, 8, 72, (0,), scale_n=0, scale_n_lt_rows_pad=True),
    _x3("input_gradient_3x3_pair", 32, 8, 3, 3, 32, 32, 288, (0, 3, 2), transposed=1, scale_n=8, rows=8, chans=32),
    # ---- row contents
    _max_at(0), _max_at(63), _max_at(64), _max_at(255), _max_at(256), _max_at(287),
    _content("max_is_negative", [Plant(1, 130, f32(-2.5), "ordinary"), Plant(5, 256, f32(-1e-3), "ordinary")], amax_pos={1: 130, 5: 256},
             max_negative=(1, 5)),
    _content("amax_power_of_two", [Plant(r, 10 + 37 * r, pow2(e), "ordinary") for r, e in enumerate(POW2_EXPONENTS)],
             amax={r: pow2(e) for r, e in enumerate(POW2_EXPONENTS)}),
    _content("amax_below_power_of_two", [Plant(r, 20 + 31 * r, below(pow2(e)), "ordinary") for r, e in enumerate(POW2_EXPONENTS)],
             amax={r: below(pow2(e)) for r, e in enumerate(POW2_EXPONENTS)}),
    _content("amax_f32_max", [Plant(3, 200, F32_MAX, "ordinary"), Plant(4, 1, -F32_MAX, "ordinary")], amax={3: F32_MAX, 4: F32_MAX}, shift={3: -117}),
    _content("amax_2^-116_last_uncapped", [Plant(2, 77, pow2(-116), "ordinary"), Plant(5, 256, below(pow2(-116)), "ordinary")],
             amax={2: pow2(-116), 5: below(pow2(-116))}, shift={2: 126, 5: 126}, capped={2: False, 5: True}),
    _content("amax_below_2^-117", [Plant(2, 77, below(pow2(-117)), "ordinary"), Plant(6, 260, pow2(-117), "ordinary")],
             amax={2: below(pow2(-117)), 6: pow2(-117)}, shift={2: 126, 6: 126}, capped={2: True, 6: True}),
    _content("amax_2^-126_smallest_normal", [Plant(2, 5, pow2(-126), "ordinary")], amax={2: pow2(-126)}, shift={2: 126}, capped={2: True}),
    _content("amax_2^-149_smallest_subnormal", [Plant(2, 5, pow2(-149), "ordinary"), Plant(3, 280, -pow2(-140), "ordinary")],
             amax={2: pow2(-149), 3: pow2(-140)}, shift={2: 126, 3: 126}, capped={2: True, 3: True}),
    _content("row_of_plus_zero", [Plant(4, None, f32(0.0), "const")], amax={4: f32(0.0)}, shift={4: 0}, zero_sign={4: 0}),
    _content("row_of_minus_zero", [Plant(4, None, f32(-0.0), "const")], amax={4: f32(0.0)}, shift={4: 0}, zero_sign={4: 1}),
    _content("neighbours_underflow_when_scaled_down", [Plant(1, 0, pow2(120), "tiny"), Plant(6, 287, -pow2(127), "tiny")],
             amax={1: pow2(120), 6: pow2(127)}, shift={1: -110, 6: -117}, underflow=(1, 6)),
]


def x3_case(name):
    return next(c for c in X3_CASES if c.name == name)


def weight_shape(c):
    return (c.O, c.I, 3, 3) if c.transposed >= 2 else (c.O, c.I, c.R, c.S)


def make_weight(c):
    w = ordinary_weight(c.name, weight_shape(c))
    g = _rng(c.name + "/plants")
    for p in c.plants:
        plant_row(w, p, g)
    return w


def x3_properties(c):
    """what test_pack_host.py holds `expect` against"""
    rows, chans, taps = packed_dims(c.O, c.I, c.R, c.S, c.transposed)
    K = c.chans_pad if c.transposed >= 2 else taps * c.chans_pad
    img = pack_image(make_weight(c), c.O, c.I, c.R, c.S, c.chans_pad, c.rows_pad, K, 0, c.transposed)
    v, hi, lo, pw, scale, sh, amax = x3_rows(img)
    pos = np.abs(img).argmax(axis=1)
    p = dict(K=K, K_lt=K, K_gt=K, rows=rows, chans=chans, groups4=c.Kpad // 4, groups8=c.Kpad // 8,
             pieces3=c.chans_pad // 32 * 288 // 4, pieces2=c.chans_pad // 16 * 160 // 4, chunk_pairs=c.chans_pad // 32,
             chunks=c.chans_pad // 16, rows_pad_gt_rows=c.rows_pad > rows, chans_pad_gt_chans=c.chans_pad > chans,
             Kpad_gt_K=c.Kpad > K, scale_n_lt_rows_pad=c.scale_n < c.rows_pad)
    p["amax_pos"] = {int(r): int(pos[r]) for r in range(c.rows_pad)}
    p["amax"] = {int(r): amax[r] for r in range(c.rows_pad)}
    p["shift"] = {int(r): int(sh[r]) for r in range(c.rows_pad)}
    _, ex = np.frexp(amax)
    p["capped"] = {int(r): bool(amax[r] > 0 and 11 - ex[r] > SHIFT_CAP) for r in range(c.rows_pad)}
    p["max_negative"] = tuple(int(r) for r in range(c.rows_pad) if img[r, pos[r]] < 0)
    p["zero_sign"] = {int(r): int(np.signbit(img[r, :K]).all()) for r in range(c.rows_pad) if not img[r].any()}
    with np.errstate(under="ignore"):
        exact = pw[:, None].astype(np.float64) * img.astype(np.float64)
    p["underflow"] = tuple(int(r) for r in range(c.rows_pad) if (v[r].astype(np.float64) != exact[r]).any() or
                           ((v[r] == 0) & (img[r] != 0)).any())
    return p


F16Case = namedtuple("F16Case", "name O I R S chans_pad rows_pad Kpad korder transposed values expect")


def _f16(name, O, I, R, S, chans_pad, rows_pad, Kpad, korder=0, transposed=0, values=(), **expect):
    return F16Case(name, O, I, R, S, chans_pad, rows_pad, Kpad, korder, transposed, tuple(values), expect)


# values planted in the f16-only case, with the f16 bits they must become
F16_EDGE_VALUES = [
    (65504.0, 0x7BFF), (65519.996, 0x7BFF), (65520.0, 0x7C00), (-65520.0, 0xFC00), (1e5, 0x7C00), (float(F32_MAX), 0x7C00),  # overflow
    (2.0 ** -24, 0x0001), (2.0 ** -25, 0x0000), (float(np.nextafter(f32(2.0 ** -25), f32(1))), 0x0001), (3 * 2.0 ** -25, 0x0002),
    (-(2.0 ** -25), 0x8000), (2.0 ** -14, 0x0400), (float(below(2.0 ** -14)), 0x0400), (1023 * 2.0 ** -24, 0x03FF),      # subnormal range
    (5.5 * 2.0 ** -24, 0x0006), (6.5 * 2.0 ** -24, 0x0006), (2.0 ** -149, 0x0000), (-(2.0 ** -149), 0x8000),
    (-0.0, 0x8000), (0.0, 0x0000),
    (1 + 2.0 ** -11, 0x3C00), (1 + 3 * 2.0 ** -11, 0x3C02), (float(np.nextafter(f32(1 + 2.0 ** -11), f32(2))), 0x3C01),        # ties
    (-(1 + 2.0 ** -11), 0xBC00), (2047.5, 0x6800), (2046.5, 0x67FE),
]

F16_CASES = [
    _f16("forward_3x3_tap_major", 6, 8, 3, 3, 8, 16, 96, rows=6, rows_pad_gt_rows=True, Kpad_gt_K=True, total_mod_256=0),
    _f16("forward_3x3_chunk_major", 5, 64, 3, 3, 64, 16, 576, korder=1, K=576, total_mod_256=0),
    _f16("chunk_major_padded_channels", 6, 40, 3, 3, 64, 8, 576, korder=1, chans=40, chans_pad_gt_chans=True),
    _f16("input_gradient_chunk_major", 24, 8, 3, 3, 32, 16, 288, korder=1, transposed=1, rows=8, chans=24, chans_pad_gt_chans=True),
    _f16("input_gradient_tap_major", 12, 20, 3, 3, 16, 24, 160, transposed=1, rows=20, chans=12, Kpad_gt_K=True),
    _f16("non_square_3x1", 7, 16, 3, 1, 16, 9, 64, K=48, total_mod_256=64),
    _f16("non_square_2x3_input_gradient", 7, 12, 2, 3, 8, 16, 64, transposed=1, rows=12, chans=7),
    _f16("non_square_1x3_chunk_major", 5, 32, 1, 3, 32, 8, 96, korder=1, K=96),
    _f16("stem_7x7_three_channels", 16, 3, 7, 7, 8, 16, 416, K=392, chans=3, Kpad_gt_K=True),
    _f16("one_by_one", 10, 24, 1, 1, 24, 13, 32, K=24, rows_pad_gt_rows=True, total_mod_256=160),
    _f16("dcn_cols_tap_major", 48, 32, 3, 3, 64, 320, 64, transposed=2, rows=288, chans=48, rows_pad_gt_rows=True),
    _f16("dcn_cols_chunk_major", 48, 32, 3, 3, 64, 288, 96, transposed=3, rows=288, chans=48, Kpad_gt_K=True),
    _f16("dcn_cols_tap_major_small", 5, 8, 3, 3, 8, 80, 32, transposed=2, rows=72, chans=5, chans_pad_gt_chans=True),
    _f16("f16_edge_values", 4, 8, 3, 3, 8, 4, 72, values=F16_EDGE_VALUES, K=72),
]


def f16_case(name):
    return next(c for c in F16_CASES if c.name == name)


def make_weight_f16(c):
    """ordinary weights; the edge case's values go to consecutive elements of the flat parameter"""
    w = ordinary_weight("f16/" + c.name, (c.O, c.I, c.R, c.S))
    if c.values:
        flat = w.reshape(-1)
        flat[5:5 + len(c.values)] = np.array([v for v, _ in c.values], np.float64).astype(np.float32)
    return w


def f16_properties(c):
    rows, chans, taps = packed_dims(c.O, c.I, c.R, c.S, c.transposed)
    K = c.chans_pad if c.transposed >= 2 else taps * c.chans_pad
    return dict(K=K, rows=rows, chans=chans, rows_pad_gt_rows=c.rows_pad > rows, chans_pad_gt_chans=c.chans_pad > chans,
                Kpad_gt_K=c.Kpad > K, total_mod_256=c.rows_pad * c.Kpad % 256)


def check_expect(expect, props):
    """every `expect` entry against the properties: K_lt / K_gt are bounds, dict entries are compared key by key"""
    for key, want in expect.items():
        got = props[key]
        if key == "K_lt":
            ok = got < want
        elif key == "K_gt":
            ok = got > want
        elif key in ("max_negative", "underflow"):     # rows that must have the property (ordinary rows may have it too)
            ok = set(want) <= set(got)
        elif isinstance(want, dict):
            ok = all(got[r] == v for r, v in want.items())
        else:
            ok = got == want
        assert ok, (key, want, got)


# ------------------------------------------------------------------------------------------------ split_weights
def split_edge_image(n=1200):
    """f32 image for ctdet_split_weights: scaled-weight magnitudes with the edge values of the split planted (n / 4 = 300 groups:
    two workgroups, the second partly idle).  No NaN: its payload bits are not pinned."""
    g = _rng("split")
    a = (g.standard_normal(n) * 600.0).astype(np.float32)
    edge = [0.0, -0.0, 2047.5, -2047.5, 1024.0, 1023.99994, 2.0 ** -14, 2.0 ** -24, 2.0 ** -25, -(2.0 ** -25), 2.0 ** -126, 2.0 ** -149,
            -(2.0 ** -149), 65504.0, 65520.0, -1e5, float(F32_MAX), 1 + 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -23, 1 + 3 * 2.0 ** -11,
            0.1, 1e-3, 1e-5, 1e-7, 1e-9, 2047.0 + 2.0 ** -13, 1535.4999]
    a[7:7 + len(edge)] = np.array(edge, np.float64).astype(np.float32)
    a[n - len(edge):] = -np.array(edge, np.float64).astype(np.float32)
    return a


def split_image(a):
    """uint16 bits [n / 4, 8] of ctdet_split_weights: per group of 4 {hi[4], lo[4]}"""
    hi, lo = split(a)
    return _bits(np.stack([hi.reshape(-1, 4), lo.reshape(-1, 4)], axis=1).reshape(-1, 8))
