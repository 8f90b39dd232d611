"""The cases of the affine warp tests (test_warp_host.py, test_warp_gpu.py), each with the reason it is there; the scalar
per-pixel restatement of data/warp.py's arithmetic that the vectorised reference is held to; the source sizes the sampler
is checked on."""
import math

import numpy as np

COL_TILE, ROW_TILE = 64, 8      # output columns / rows of one block of csrc/warp.hip (WARP_TW, WARP_RB); test_warp_host.py pins them


def _rot(deg, tx, ty):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return [[c, -s, tx], [s, c, ty]]


# (name, (H, W), (out_h, out_w), inverse matrix M (destination -> source pixel index), flip, what it is there for)
CASES = [
    ("borders", (5, 7), (8, 8), [[1.3, 0, -1.5], [0, 0.95, -1.5]], False,
     "the map overhangs the source on all four sides: taps at -1, at W and H, pixels wholly outside"),
    ("seams", (11, 70), (ROW_TILE + 1, COL_TILE + 1), [[1.03, 0, 0.4], [0, 1.07, 0.2]], False,
     "out_h = the row tile + 1, out_w = the column tile + 1: a block with one live row, a block with one live column"),
    ("all_phases", (40, 40), (32, 32), [[33 / 32, 0, 0], [0, 33 / 32, 0]], False, "visits all 32 x 32 (fx, fy) phase pairs"),
    ("downscale", (60, 90), (16, 24), [[3.5, 0, 1.0], [0, 3.5, 0.5]], False, "a strong downscale: taps far apart, no prefilter"),
    ("rotation", (37, 53), (24, 40), _rot(5.0, 3.2, -1.7), False, "a rotation by 5 degrees: all four tables are non-trivial"),
    ("flip", (23, 31), (16, 40), [[0.8, 0, -2.5], [0, 0.8, 1.0]], True, "the source is read mirrored, overhanging both sides"),
    ("outside", (9, 9), (8, 8), [[1, 0, 500.0], [0, 1, -300.0]], False, "a map that lies entirely outside the source: zeros"),
    ("int32_limit", (4, 4), (2, 2), [[(2 ** 31 - 1) / 1024, 0, (2 ** 31 - 1 - 16) / 1024], [0, 1, 0]], False,
     "x0 = ax[1] = 2**31 - 1: their sum wraps to -2 in 32 bits, which would read column 0 at phase 31; in 64 bits it is outside"),
    ("identity", (12, 20), (12, 20), [[1, 0, 0], [0, 1, 0]], False, "the identity map returns the source"),
    ("one_pixel", (1, 1), (3, 3), [[0.5, 0, -0.25], [0, 0.5, -0.25]], False, "a one-pixel source"),
]
CASE_IDS = [c[0] for c in CASES]

# the batch of one launch: sources of different sizes, one of them flipped (indices into CASES share nothing: own maps)
BATCH_OUT = (10, 70)
BATCH = [((5, 7), [[0.1, 0, -0.3], [0, 0.5, -0.2]], False), ((33, 21), _rot(-12.0, 4.0, 9.0), True),
         ((64, 130), [[1.9, 0, -3.0], [0, 2.3, 0.0]], False)]

# the sampler's source sizes (h, w): a side below twice the border (100, 255: border() halves it), the workload's, a square
SAMPLER_SIZES = [(100, 255), (255, 100), (480, 640), (64, 64), (257, 256)]
BORDER_VALUES = {64: 16, 100: 32, 255: 64, 256: 64, 257: 128, 480: 128}      # border(128, size)


def make_image(H, W, seed=0, channels=3):
    return np.random.RandomState(seed).randint(0, 256, (H, W, channels), dtype=np.uint8)


def case_inputs():
    """(name, image HWC, M float64 [2, 3], flip, (out_h, out_w)) for every case"""
    for i, (name, (H, W), out, M, flip, _) in enumerate(CASES):
        yield name, make_image(H, W, seed=i), np.array(M, dtype=np.float64), flip, out


def _rint(v):
    """round half to even of a float (Python's round does that)"""
    return int(round(v))


def warp_scalar(img, M, out_h, out_w, flip=False):
    """data/warp.py's definition one pixel at a time, in Python integers: no table array, no vector operation"""
    H, W, C = img.shape
    out = np.zeros((out_h, out_w, C), dtype=np.uint8)
    M = [[float(v) for v in row] for row in np.asarray(M, dtype=np.float64)]
    for y in range(out_h):
        x0 = _rint((M[0][1] * y + M[0][2]) * 1024) + 16
        y0 = _rint((M[1][1] * y + M[1][2]) * 1024) + 16
        for x in range(out_w):
            X, Y = (x0 + _rint(M[0][0] * x * 1024)) >> 5, (y0 + _rint(M[1][0] * x * 1024)) >> 5
            sx, fx, sy, fy = X >> 5, X & 31, Y >> 5, Y & 31
            taps = (((sy, sx), 32 * (32 - fx) * (32 - fy)), ((sy, sx + 1), 32 * fx * (32 - fy)),
                    ((sy + 1, sx), 32 * (32 - fx) * fy), ((sy + 1, sx + 1), 32 * fx * fy))
            assert sum(w for _, w in taps) == 32768
            for c in range(C):
                acc = 16384
                for (ty, tx), w in taps:
                    if 0 <= ty < H and 0 <= tx < W:
                        acc += w * int(img[ty, W - 1 - tx if flip else tx, c])
                out[y, x, c] = acc >> 15
    return out
