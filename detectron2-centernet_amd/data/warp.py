"""CenterNet's random scale-and-crop training input (INPUT.AFFINE): the sampler, the affine map, the 8-bit
warp arithmetic and the box rule, each written once.  This numpy restatement is the contract: csrc/warp.hip computes the
bytes of `warp_affine_u8_reference`, and data.transforms.AffineTransform is a thin shell around the functions here.

Neither half is in the reference tree (its mapper has ResizeShortestEdge alone).  The sampler is restated from the published
CenterNet `ctdet` training sampler (random centre inside a border, a scale from a list, a flip, one warp to a fixed input
size); the warp arithmetic is restated from OpenCV's 8-bit INTER_LINEAR warpAffine (10-bit fixed-point coordinates, 5-bit
phases, 15-bit weights).  cv2 is not a dependency and parity with either is unpinned, the standing the fvcore transforms
have in data/transforms.py.

The test side (INPUT.AFFINE.TEST_MODE) is here too, on the same standing: CenterNet's fix_res / keep_res test
input as a map (`test_params`), the way of its boxes back into the original image (`unwarp_params`) and the numpy oracle
csrc/unwarp.hip is held to bit for bit (`unwarp_boxes_reference`).

Coordinates are pixel indices: destination pixel (x, y) reads the source at M @ (x, y, 1), M the 2x3 inverse matrix.  With
`flip` the source is read mirrored -- column j of the image M speaks of is column W - 1 - j of the stored one."""
import numpy as np

COORD_BITS = 10                   # fixed-point bits of a source coordinate
PHASE_BITS = 5                    # of which the interpolation keeps this many: 32 phases per axis
WEIGHT_BITS = 15                  # the four weights of a pixel sum to 1 << 15
MAX_SOURCE_SIDE = 16384           # sources above this per side are refused (coordinate * 1024 stays far inside int32)
_PHASES = 1 << PHASE_BITS
_ROUND = 1 << (COORD_BITS - PHASE_BITS - 1)      # 16: rounds the 10-bit coordinate to its 5-bit phase


# ------------------------------------------------------------------------------------------------------------ the sampler
def border(limit, size):
    """the margin the centre keeps from an edge of a side of `size` pixels: `limit`, halved until two of them fit"""
    assert limit >= 0 and size >= 1, (limit, size)
    i = 1
    while size - limit // i <= limit // i:
        i *= 2
    return limit // i


def draw_params(h, w, scales, border_limit, flip_prob):
    """the draws for an h x w source, from numpy's global RNG in the order DESIGN.md 7.12 states: the scale index, the centre
    column, the centre row, the flip uniform.  Returns (s, cx, cy, flip): the source window's side in pixels, its centre
    (pixel indices of the unflipped image) and whether the image is mirrored."""
    s = max(h, w) * scales[np.random.randint(len(scales))]
    bw, bh = border(border_limit, w), border(border_limit, h)
    cx = np.random.randint(bw, w - bw)
    cy = np.random.randint(bh, h - bh)
    flip = bool(np.random.uniform(0, 1) < flip_prob)
    return float(s), int(cx), int(cy), flip


def inverse_matrix(s, cx, cy, flip, w, out_h, out_w):
    """float64 [2, 3]: destination pixel index -> source pixel index (of the mirrored image when `flip`).  The window of
    side s around the centre lands on the output's width; the scale is the same on both axes."""
    a = float(s) / out_w
    cxf = (w - 1 - cx) if flip else cx
    return np.array([[a, 0.0, cxf - a * out_w / 2], [0.0, a, cy - a * out_h / 2]], dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------- bytes
def warp_tables(M, out_h, out_w):
    """int32 (ax[out_w], bx[out_w], x0[out_h], y0[out_h]) of the inverse matrix M, from float64 with round-half-even:
    the 10-bit fixed-point source coordinate of destination (x, y) is (x0[y] + ax[x], y0[y] + bx[x]), 16 already added"""
    M = np.asarray(M, dtype=np.float64)
    assert M.shape == (2, 3) and np.isfinite(M).all(), M
    one = float(1 << COORD_BITS)
    x, y = np.arange(out_w, dtype=np.float64), np.arange(out_h, dtype=np.float64)
    tabs = (np.rint(M[0, 0] * x * one), np.rint(M[1, 0] * x * one),
            np.rint((M[0, 1] * y + M[0, 2]) * one) + _ROUND, np.rint((M[1, 1] * y + M[1, 2]) * one) + _ROUND)
    for t in tabs:
        if t.size and (t.min() < -2.0 ** 31 or t.max() > 2.0 ** 31 - 1):
            raise ValueError(f"warp_tables: the map {M.tolist()} leaves int32 at 10 fixed-point bits over a {out_h}x{out_w} output")
    return tuple(t.astype(np.int32) for t in tabs)


def warp_affine_u8_reference(img, M, out_h, out_w, flip=False):
    """uint8 [H, W, C] -> uint8 [out_h, out_w, C]: bilinear, taps outside the source contribute 0 (constant border 0).
    Integer throughout once the tables are built; the two table entries of a coordinate are added in 64 bits."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3, (img.dtype, img.shape)
    H, W = img.shape[:2]
    if not (1 <= H <= MAX_SOURCE_SIDE and 1 <= W <= MAX_SOURCE_SIDE):
        raise ValueError(f"warp_affine_u8: source {H}x{W} (1..{MAX_SOURCE_SIDE} per side)")
    if flip:
        img = img[:, ::-1]
    ax, bx, x0, y0 = (t.astype(np.int64) for t in warp_tables(M, out_h, out_w))
    X = (x0[:, None] + ax[None, :]) >> (COORD_BITS - PHASE_BITS)
    Y = (y0[:, None] + bx[None, :]) >> (COORD_BITS - PHASE_BITS)
    sx, fx = X >> PHASE_BITS, X & (_PHASES - 1)
    sy, fy = Y >> PHASE_BITS, Y & (_PHASES - 1)
    acc = np.full((out_h, out_w, img.shape[2]), 1 << (WEIGHT_BITS - 1), dtype=np.int64)
    for dy, dx, wgt in ((0, 0, (_PHASES - fx) * (_PHASES - fy)), (0, 1, fx * (_PHASES - fy)),
                        (1, 0, (_PHASES - fx) * fy), (1, 1, fx * fy)):
        ty, tx = sy + dy, sx + dx
        inside = (ty >= 0) & (ty < H) & (tx >= 0) & (tx < W)
        tap = img[np.clip(ty, 0, H - 1), np.clip(tx, 0, W - 1)].astype(np.int64)
        acc += tap * (np.where(inside, wgt, 0) << (WEIGHT_BITS - 2 * PHASE_BITS))[:, :, None]
    return (acc >> WEIGHT_BITS).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- boxes
def forward_coords(coords, M, flip, w):
    """[N, 2] source pixel indices (x, y) of the stored w-wide image -> destination pixel indices: mirrored first when
    `flip` (x -> w - 1 - x), then through the inverse of M"""
    coords = np.array(coords, dtype=np.float64).reshape(-1, 2)
    M = np.asarray(M, dtype=np.float64)
    if flip:
        coords[:, 0] = w - 1 - coords[:, 0]
    return (coords - M[:, 2]) @ np.linalg.inv(M[:, :2]).T


# ------------------------------------------------------------------------- the test input (INPUT.AFFINE.TEST_MODE, 7.13)
TEST_MODES = ("", "fix_res", "keep_res")


def check_test_mode(mode, out_hw, divisibility):
    """refuses, by name, a TEST_MODE that is none of TEST_MODES, a fix_res OUTPUT_SIZE that is no positive multiple of the
    size divisibility and a keep_res divisibility that is no power of two; returns the mode"""
    if mode not in TEST_MODES:
        raise ValueError(f"INPUT.AFFINE.TEST_MODE {mode!r}: one of {', '.join(repr(m) for m in TEST_MODES)}")
    D = int(divisibility)
    if mode == "fix_res":
        oh, ow = (int(v) for v in out_hw)
        if oh < 1 or ow < 1 or (D > 0 and (oh % D or ow % D)):
            raise ValueError(f"INPUT.AFFINE.OUTPUT_SIZE {tuple(out_hw)}: (out_h, out_w), each a positive multiple of "
                             f"MODEL.CENTERNET.SIZE_DIVISIBILITY ({D})")
    if mode == "keep_res" and (D < 1 or D & (D - 1)):
        raise ValueError(f"INPUT.AFFINE.TEST_MODE 'keep_res' pads to (side | (D - 1)) + 1: MODEL.CENTERNET.SIZE_DIVISIBILITY "
                         f"must be a power of two, got {D}")
    return mode


def test_params(h, w, mode, out_hw=None, divisibility=32):
    """(M, out_h, out_w) of CenterNet's test input for an h x w source: the inverse matrix (inverse_matrix, never flipped) and
    the size of the network input.
      "fix_res": letterbox to out_hw -- the window of side max(h, w) around the image's centre (w / 2, h / 2) lands on the
        output's width;
      "keep_res": out = (side | (D - 1)) + 1 per side, CenterNet's rule, which pads even a side that is a multiple of D; the
        window's side is out_w (scale 1) and the centre (w // 2, h // 2), so the map is an integer shift and the warp a copy
        of the source into a zero frame."""
    h, w = int(h), int(w)
    assert h >= 1 and w >= 1, (h, w)
    check_test_mode(mode, out_hw, divisibility)
    if mode == "fix_res":
        out_h, out_w = (int(v) for v in out_hw)
        s, cx, cy = float(max(h, w)), w / 2, h / 2
    elif mode == "keep_res":
        D = int(divisibility)
        out_h, out_w = (h | (D - 1)) + 1, (w | (D - 1)) + 1
        s, cx, cy = float(out_w), w // 2, h // 2
    else:
        raise ValueError("test_params: INPUT.AFFINE.TEST_MODE is off ('')")
    return inverse_matrix(s, cx, cy, False, w, out_h, out_w), out_h, out_w


test_params.__test__ = False      # a definition, not a test (its name is the one DESIGN.md 7.13 gives it)


def unwarp_params(M, orig_hw):
    """float32 [6] = (sx, sy, tx, ty, orig_w, orig_h): the map of a box coordinate of the network input back into the
    orig_h x orig_w source, x' = x * sx + tx, y' = y * sy + ty, and the frame it is clipped to.  M is the (axis-aligned)
    inverse matrix of the warp; computed in float64 and cast once."""
    M = np.asarray(M, dtype=np.float64)
    assert M.shape == (2, 3) and np.isfinite(M).all() and M[0, 1] == 0 and M[1, 0] == 0, f"an axis-aligned [2, 3] map, got {M.tolist()}"
    return np.array([M[0, 0], M[1, 1], M[0, 2], M[1, 2], float(orig_hw[1]), float(orig_hw[0])], dtype=np.float64).astype(np.float32)


def unwarp_boxes_reference(boxes, scores, classes, max_det, thresh, params):
    """the numpy float32 oracle of dec_postprocess_affine_kernel (csrc/unwarp.hip, ops.postprocess_affine) for ONE image:
    boxes f32 [K, 4] XYXY in network-input pixels, scores f32 [K], classes [K], params = unwarp_params(...) ->
    (boxes [n, 4], scores [n], classes [n]).

    The box map is the inverse of the training box rule forward_coords(., M, False, w): a source point that
    forward_coords sends to (x, y) comes back as (x * sx + tx, y * sy + ty).  Its arithmetic is x' = f32(f32(x * sx) + tx)
    -- two roundings, never a fused multiply-add -- and y' alike with sy, ty.  The rest is dec_postprocess_kernel's rule, word
    for word: clip to [0, orig_w] x [0, orig_h], a NaN coordinate handed on; keep row k only if score > thresh (strictly, in
    f32), x2 - x1 > 0, y2 - y1 > 0 and k < max_det; the kept rows stay in order."""
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    scores = np.asarray(scores, dtype=np.float32).reshape(-1)
    classes = np.asarray(classes).reshape(-1)
    p = np.asarray(params, dtype=np.float32).reshape(6)
    assert len(scores) == len(classes) == len(boxes)
    n = max(0, min(len(boxes), int(max_det)))
    boxes, scores, classes = boxes[:n], scores[:n], classes[:n]
    with np.errstate(invalid="ignore", over="ignore"):
        scale = np.array([p[0], p[1], p[0], p[1]], dtype=np.float32)
        shift = np.array([p[2], p[3], p[2], p[3]], dtype=np.float32)
        hi = np.array([p[4], p[5], p[4], p[5]], dtype=np.float32)
        prod = (boxes * scale).astype(np.float32)            # rounded once ...
        moved = (prod + shift).astype(np.float32)            # ... and once more
        clipped = np.where(np.isnan(moved), moved, np.minimum(np.maximum(moved, np.float32(0)), hi)).astype(np.float32)
        keep = (scores > np.float32(thresh)) & ((clipped[:, 2] - clipped[:, 0]) > 0) & ((clipped[:, 3] - clipped[:, 1]) > 0)
    return clipped[keep], scores[keep], classes[keep]


# --------------------------------------------------------------------------------------------------- the record's "warp"
def pack_warp(M, flip):
    """the "warp" entry of a raw training record: float64 [2, 4], columns 0..2 the inverse matrix, [0, 3] the flip flag"""
    out = np.zeros((2, 4), dtype=np.float64)
    out[:, :3] = M
    out[0, 3] = 1.0 if flip else 0.0
    return out


def unpack_warp(warp):
    """(M float64 [2, 3], flip) of a packed [2, 4] array / tensor, or of an (M, flip) pair"""
    if isinstance(warp, (tuple, list)) and len(warp) == 2 and np.ndim(warp[1]) == 0:
        return np.asarray(warp[0], dtype=np.float64).reshape(2, 3), bool(warp[1])
    arr = np.asarray(warp, dtype=np.float64)
    assert arr.shape == (2, 4), f"a warp is a float64 [2, 4] array (data.warp.pack_warp) or an (M, flip) pair, got shape {arr.shape}"
    return arr[:, :3].copy(), bool(arr[0, 3] != 0)
