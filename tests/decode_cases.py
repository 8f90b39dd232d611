"""Case tables for the kernels that finish every inference step -- dec_tile_kernel / dec_final_kernel (ops.decode) and
dec_postprocess_kernel (ops.postprocess), all in csrc/decode.hip -- at the geometry the COCO-shaped tests never reach: more than
one channel chunk, the 4-row tile, a partial last channel vector on the vector-load path, K up to the launcher's 1024, maps whose
every value falls into the first radix bin, the clamp floor and the flip merge on chunked maps; for postprocess every way a row can
be kept or dropped, on both sides of the 64-row wave seam.  Every shape is the smallest that still takes the branch named next to
it.  test_decode_host.py checks the tables against their own conditions on the CPU; test_decode_gpu.py runs the kernels over them.

References: oracle/ctdet_oracle.py alone -- ctdet_decode on the same maps in NCHW (the flip cases on maps merged by torch on the
CPU), inference_single_image followed by detector_postprocess with its keep mask for postprocess.
"""
import functools
from collections import namedtuple

import numpy as np
import torch

from oracle import ctdet_oracle as O
from test_hip_ops import _rand_heat, _trained_like, nhwc  # noqa: F401  (nhwc: for the GPU test)

# ------------------------------------------------------------------------------------------------------------------------
# decode.hip's tile geometry, restated
# ------------------------------------------------------------------------------------------------------------------------
DEC_LDS_TILE = 60 * 1024      # bytes of LDS for the tile image, later the peak list
DEC_TW = 16                   # tile columns (+ 2 halo columns)
DEC_CW_MAX = 112              # channels per workgroup at the most
DEC_TILE_BYTES = 4            # f32 tile value
DEC_LIST_BYTES = 6            # u32 score bits + u16 position per possible peak
DEC_TILE_SLACK = 128
DEC_K_MAX = 1024
DEC_INDEX_BITS = 24
DEC_BIN0_BELOW = 2.0 ** -15   # dec_d0: every value below this lands in bin 0 of the first radix level
HEAT_FLOOR = 1e-4

DecGeom = namedtuple("DecGeom", "CW TH cchunks tiles_x tiles_y")


def dec_geom(H, W, C):
    C4 = (C + 3) & ~3
    CW = min(C4, DEC_CW_MAX)
    TH = 8
    while TH > 1 and ((TH + 2) * (DEC_TW + 2) * CW * DEC_TILE_BYTES > DEC_LDS_TILE or TH * DEC_TW * CW * DEC_LIST_BYTES > DEC_LDS_TILE):
        TH >>= 1
    return DecGeom(CW, TH, -(-C4 // CW), -(-W // DEC_TW), -(-H // TH))


GEOMETRY = {80: (80, 8, 1), 81: (84, 4, 1), 112: (112, 4, 1), 113: (112, 4, 2), 116: (112, 4, 2), 224: (112, 4, 2), 225: (112, 4, 3),
            16: (16, 8, 1), 8: (8, 8, 1)}          # C -> (CW, TH, cchunks)

# ------------------------------------------------------------------------------------------------------------------------
# decode
# ------------------------------------------------------------------------------------------------------------------------
# kind: spread (_rand_heat), trained (_trained_like: background exactly on 1e-4; arg = (blobs per image, plant 0.3 at [0,0,0,1] and 0.2 in
# every image's last cell [C-1,H-1,W-1])),
# const2 (0.25 on the channels [arg[0], arg[1]), 0.1 elsewhere), tiny (rand * 2^-16 + 2^-60).  stride: channels per pixel of the
# buffer the map is a slice of (== C: dense).  flip: 2B images are decoded as B mirror-merged ones.
DecodeCase = namedtuple("DecodeCase", "group kind B C H W stride K floor flip seed arg")


def _dc(group, kind, shape, stride, K, floor=0.0, flip=False, seed=0, arg=None):
    B, C, H, W = shape
    return DecodeCase(group, kind, B, C, H, W, stride or C, K, floor, flip, seed, arg)


CHANNEL_ROWS = [(80, 80), (81, 81), (81, 84), (112, 112), (113, 113), (113, 116), (224, 224), (225, 228)]     # (C, pixel stride)
# seeds with which every image's selection has 100 distinct scores and reaches the last chunk (test_decode_host.py asserts both)
CHANNEL_SEEDS = {(80, 80): 1, (81, 81): 1, (81, 84): 1, (112, 112): 1, (113, 113): 3, (113, 116): 3, (224, 224): 1, (225, 228): 26}
K_SPREAD_SHAPE, K_SPREAD_KS = (1, 16, 32, 40), (1, 257, 513, 1024)
DENSE_BLOBS, SPARSE_BLOBS = 150, 5

DECODE_CASES = (
    # channel geometry: 9 x 21 gives partial tiles in both directions, two column tiles, two (TH 8) or three (TH 4) row tiles
    [_dc("channels", "spread", (2, C, 9, 21), s, 100, seed=CHANNEL_SEEDS[C, s]) for C, s in CHANNEL_ROWS] +
    # ties across the chunk seam
    [_dc("ties", "const2", (1, 225, 5, 19), 225, 300, arg=(110, 115)),
     _dc("ties", "const2", (1, 225, 5, 19), 228, 1024, arg=(200, 225))] +
    # K: the final sort widths 512 .. 2048, the fill region at 2K = 2048, the tile budget at large K
    [_dc("K", "spread", K_SPREAD_SHAPE, 0, K, seed=1) for K in K_SPREAD_KS] +
    [_dc("K", "spread", (1, 8, 12, 20), 0, 1024, seed=1),
     _dc("K", "const2", (1, 116, 3, 3), 0, 1024, arg=(0, 116)),
     _dc("K", "spread", (2, 112, 12, 16), 0, 513, seed=1)] +
    # every key in bin 0 of the first radix level
    [_dc("bin0", "tiny", (2, 8, 24, 40), 0, 100, seed=1)] +
    # the clamp floor on a chunked, strided map: more than K blobs, and five blobs plus one planted cell
    [_dc("floor", "trained", (2, 113, 24, 40), 116, 100, floor=f, seed=1, arg=(n, n == SPARSE_BLOBS))
     for n in (DENSE_BLOBS, SPARSE_BLOBS) for f in (HEAT_FLOOR, 0.0)] +
    # the flip merge
    [_dc("flip", kind, shape, s, 100, floor=f, flip=True, seed=1, arg=arg)
     for kind, shape, s, arg in (("spread", (2, 81, 9, 21), 84, None), ("spread", (2, 113, 9, 21), 113, None),
                                 ("trained", (2, 113, 24, 40), 116, (SPARSE_BLOBS, True)))
     for f in (0.0, HEAT_FLOOR)]
)


def decode_id(c):
    return (f"{c.group}-{c.kind}-{c.B}x{c.C}x{c.H}x{c.W}-s{c.stride}-K{c.K}-{'floor' if c.floor else 'nofloor'}"
            f"{'-flip' if c.flip else ''}{'' if c.arg is None else '-' + '_'.join(str(int(a)) for a in c.arg)}")


@functools.lru_cache(maxsize=None)
def _decode_inputs(kind, n, C, H, W, seed, arg):
    if kind == "spread":
        heat = _rand_heat(n, C, H, W, seed)
    elif kind == "trained":
        heat = _trained_like(n, C, H, W, arg[0], seed)
        if arg[1]:        # a cell next to flat index 0: the fill has to step over non-peak floor cells
            heat[0, 0, 0, 1] = 0.3
            heat[:, C - 1, H - 1, W - 1] = 0.2      # and the map's last cell: every image's selection reaches the last chunk
    elif kind == "const2":
        heat = torch.full((n, C, H, W), 0.1)
        heat[:, arg[0]:arg[1]] = 0.25
    elif kind == "tiny":
        heat = torch.rand(n, C, H, W, generator=torch.Generator().manual_seed(seed)) * 2.0 ** -16 + 2.0 ** -60
    else:
        raise ValueError(kind)
    g = torch.Generator().manual_seed(1)
    wh = torch.rand(n, 2, H, W, generator=g) * 20
    reg = torch.rand(n, 2, H, W, generator=g)
    return heat, wh, reg


def decode_inputs(case):
    """(heat [n,C,H,W], wh [n,2,H,W], reg [n,2,H,W]) f32 NCHW as the network would hand them over; n = 2B for a flip case.
    Shared between the tests: treat as read-only."""
    return _decode_inputs(case.kind, case.B * (2 if case.flip else 1), case.C, case.H, case.W, case.seed, case.arg)


def decode_maps(case):
    """the B maps that are decoded: the inputs, or for a flip case their mirror merge by torch on the CPU, in f32"""
    heat, wh, reg = decode_inputs(case)
    if not case.flip:
        return heat, wh, reg
    B = case.B
    return (heat[:B] + heat[B:].flip(3)) * 0.5, (wh[:B] + wh[B:].flip(3)) * 0.5, reg[:B]


@functools.lru_cache(maxsize=None)
def _decode_reference(key):
    return O.ctdet_decode(*decode_maps(key), down_ratio=4, K=key.K)


def decode_reference(case):
    """(boxes, scores, classes, inds) of the oracle; the floor is a promise about the map, not a parameter of the result"""
    return _decode_reference(case._replace(floor=0.0, stride=case.C, group=""))


def peaks(case):
    """the NMS-ed maps [B, C*H*W]: 0 where the cell is no 3x3 peak"""
    return O.nms_keep(decode_maps(case)[0]).reshape(case.B, -1)


# ------------------------------------------------------------------------------------------------------------------------
# postprocess
# ------------------------------------------------------------------------------------------------------------------------
POST_B = 3
POST_KS = (1, 63, 64, 65, 100, 1024)
POST_IMAGE = (96, 160)                                                    # (h, w) of the network's input
POST_OUT = {"g5": (192, 240), "unit": (96, 160), "inexact": (101, 167)}   # (h, w) asked for: x1.5 / x2, x1, and two scales
POST_THRESH = float(np.float32(0.3))                                      # that are no f32 numbers
PostCase = namedtuple("PostCase", "K max_det scale0")                     # scale0: the mixed image's output size
POST_CASES = [PostCase(K, md, sc) for K in POST_KS for md, sc in zip((K, K - 1, 1, K + 5), ("g5", "inexact", "inexact", "g5"))]

KEEP_RECIPES = ("inside", "clip_left_top", "clip_right_bottom", "inf_score", "inf_span")
DROP_RECIPES = ("low_score", "thresh_tie", "neg_inf_score", "nan_score", "left", "right", "above", "below", "reversed", "zero_w",
                "zero_h", "nan_x1", "nan_y1", "nan_x2", "inf_x1", "neg_inf_x2")
SPECIAL_BLOCK = KEEP_RECIPES + DROP_RECIPES        # every recipe once, at rows 2.. (K >= 63) and again at rows 72.. (K >= 100)
SPECIAL_ROWS = (2, 72)
ALT_ROWS = (48, 72)                                # kept and dropped rows alternate here, across the seam between rows 63 and 64


def post_id(c):
    return f"K{c.K}-max{c.max_det}-{c.scale0}"


def _row(recipe, rng):
    """one detection in the network input's pixels: (x1, y1, x2, y2, score)"""
    Hi, Wi = POST_IMAGE
    inf, nan = float("inf"), float("nan")
    x1, y1 = rng.uniform(2, 60), rng.uniform(2, 40)
    x2, y2 = x1 + rng.uniform(2, 60), y1 + rng.uniform(2, 40)
    score = rng.uniform(POST_THRESH + 0.05, 1.0)
    if recipe == "inside":
        pass
    elif recipe == "clip_left_top":
        x1, y1 = -rng.uniform(1, 15), -rng.uniform(1, 10)
    elif recipe == "clip_right_bottom":
        x1, y1, x2, y2 = rng.uniform(100, 150), rng.uniform(50, 90), Wi + rng.uniform(1, 15), Hi + rng.uniform(1, 10)
    elif recipe == "inf_score":
        score = inf
    elif recipe == "inf_span":
        x1, x2 = -inf, inf
    elif recipe == "low_score":
        score = rng.uniform(0.01, POST_THRESH - 0.05)
    elif recipe == "thresh_tie":
        score = POST_THRESH
    elif recipe == "neg_inf_score":
        score = -inf
    elif recipe == "nan_score":
        score = nan
    elif recipe == "left":
        x1, x2 = -rng.uniform(20, 30), -rng.uniform(1, 10)
    elif recipe == "right":
        x1, x2 = Wi + rng.uniform(1, 10), Wi + rng.uniform(20, 30)
    elif recipe == "above":
        y1, y2 = -rng.uniform(20, 30), -rng.uniform(1, 10)
    elif recipe == "below":
        y1, y2 = Hi + rng.uniform(1, 10), Hi + rng.uniform(20, 30)
    elif recipe == "reversed":
        x1, x2 = x2, x1
    elif recipe == "zero_w":
        x2 = x1
    elif recipe == "zero_h":
        y2 = y1
    elif recipe == "nan_x1":
        x1 = nan
    elif recipe == "nan_y1":
        y1 = nan
    elif recipe == "nan_x2":
        x2 = nan
    elif recipe == "inf_x1":
        x1 = inf
    elif recipe == "neg_inf_x2":
        x2 = -inf
    else:
        raise ValueError(recipe)
    return x1, y1, x2, y2, score


def post_recipes(case):
    """the recipe of every row: image 0 mixed, image 1 all kept, image 2 none kept"""
    K = case.K
    rng = np.random.RandomState(7 * K + 1)
    mixed = [None] * K
    for k in range(K):
        pool = KEEP_RECIPES if rng.randint(2) else DROP_RECIPES
        mixed[k] = pool[rng.randint(len(pool))]
    mixed[0] = "clip_left_top" if K > 1 else "thresh_tie"
    if K >= 63:
        for k in range(ALT_ROWS[0], min(K, ALT_ROWS[1])):
            mixed[k] = "inside" if k % 2 == 0 else ("low_score", "left", "zero_h", "nan_x1")[(k // 2) % 4]
        for start in SPECIAL_ROWS:
            if start + len(SPECIAL_BLOCK) <= K:
                mixed[start:start + len(SPECIAL_BLOCK)] = SPECIAL_BLOCK
    kept = [KEEP_RECIPES[rng.randint(len(KEEP_RECIPES))] for _ in range(K)]
    none = [DROP_RECIPES[rng.randint(len(DROP_RECIPES))] for _ in range(K)]
    return [mixed, kept, none]


@functools.lru_cache(maxsize=None)
def post_inputs(case):
    """dict: boxes f32 [3,K,4], scores f32 [3,K], classes i32 [3,K] (the row's own number: the order is checked with it),
    img_params f32 [3,4] = (scale_x, scale_y, out_w, out_h), out: the (h, w) asked for per image, fate: bool [3,K], the rows that
    the recipes mean to be kept (before max_det cuts)"""
    K = case.K
    rng = np.random.RandomState(11 * K + 5)
    recipes = post_recipes(case)
    rows = np.array([[_row(r, rng) for r in image] for image in recipes], dtype=np.float32)
    out = [POST_OUT[case.scale0], POST_OUT["unit"], POST_OUT["g5" if case.scale0 == "inexact" else "inexact"]]
    Hi, Wi = POST_IMAGE
    return {
        "boxes": torch.from_numpy(rows[..., :4].copy()), "scores": torch.from_numpy(rows[..., 4].copy()),
        "classes": torch.arange(K, dtype=torch.int32).repeat(POST_B, 1),
        "img_params": torch.tensor([[ow / Wi, oh / Hi, ow, oh] for oh, ow in out], dtype=torch.float32),
        "out": out, "recipes": recipes,
        "fate": torch.tensor([[r in KEEP_RECIPES for r in image] for image in recipes]),
    }


@functools.lru_cache(maxsize=None)
def post_reference(case):
    """per image (boxes [n,4], scores [n], classes [n]) of the reference path"""
    inp = post_inputs(case)
    res = []
    for b in range(POST_B):
        bb, ss, cc = O.inference_single_image(inp["boxes"][b], inp["scores"][b], inp["classes"][b], case.max_det, POST_THRESH)
        bb, keep = O.detector_postprocess(bb, POST_IMAGE, *inp["out"][b])
        res.append((bb[keep], ss[keep], cc[keep]))
    return res
