"""Pillow's 8-bit bilinear resample as integer tables and a numpy restatement of its two passes.

`ResizeTransform.apply_image` is `Image.resize(..., BILINEAR)`.  For 8-bit images that is integer arithmetic (Pillow's
published `Resample.c`: precompute_coeffs, normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc / Vertical_8bpc):

  * per output index a window of source indices `[first, first + count)` around the centre `(i + 0.5) * in / out`, with
    triangle weights of support `max(in / out, 1)`, computed in float64 and normalised by their sum;
  * each weight rounded to 22-bit fixed point, `int(0.5 + w * 2**22)` (bilinear has no negative weights);
  * a pass accumulates `byte * weight` in int32 from `1 << 21`, shifts right by 22 and clips to a byte;
  * the horizontal pass runs first, its result is a uint8 image, the vertical pass runs on that;
  * a pass whose size does not change is not run.

The HIP kernel (csrc/resize.hip) reads the tables of `bilinear_tables`; `resize_u8_reference` is the same arithmetic in
numpy, what the tests compare with Pillow bit for bit.  Pillow is the arbiter: should a release change the algorithm, the
host tests of this module fail and the tables follow Pillow.
"""
import functools
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2      # Pillow's fixed-point position for 8-bit channels
ROUND = 1 << (PRECISION_BITS - 1)


def ksize_of(in_size, out_size):
    """taps per output index: 2 * ceil(support) + 1 with support = max(in / out, 1)"""
    return 2 * int(math.ceil(max(in_size / out_size, 1.0))) + 1


@functools.lru_cache(maxsize=64)
def bilinear_tables(in_size, out_size):
    """(bounds int32 [out, 2] = first source index and tap count, coeffs int32 [out, ksize], zero padded).  The arrays are
    cached and shared: read only."""
    in_size, out_size = int(in_size), int(out_size)
    assert in_size >= 1 and out_size >= 1, (in_size, out_size)
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = ksize_of(in_size, out_size)
    centre = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    first = np.maximum((centre - support + 0.5).astype(np.int64), 0)      # C's (int) truncates; negatives clamp to 0 either way
    last = np.minimum((centre + support + 0.5).astype(np.int64), in_size)
    count = last - first
    x = np.arange(ksize, dtype=np.float64)[None, :]
    w = 1.0 - np.abs((x + first[:, None] - centre[:, None] + 0.5) * (1.0 / filterscale))
    w = np.where((w > 0.0) & (x < count[:, None]), w, 0.0)
    total = np.cumsum(w, axis=1)[:, -1:]      # summed left to right like the C loop (numpy's sum adds pairwise)
    w = np.where(total != 0.0, w / np.where(total != 0.0, total, 1.0), w)
    coeffs = (0.5 + w * (1 << PRECISION_BITS)).astype(np.int64).astype(np.int32)
    coeffs[x.repeat(out_size, 0) >= count[:, None]] = 0
    bounds = np.stack([first, count], axis=1).astype(np.int32)
    bounds.setflags(write=False)
    coeffs.setflags(write=False)
    return bounds, coeffs


def _pass(img, out_size, axis):
    """one resample pass of a uint8 array along `axis`"""
    bounds, coeffs = bilinear_tables(img.shape[axis], out_size)
    src = np.moveaxis(img, axis, 0).astype(np.int32)
    out = np.empty((out_size,) + src.shape[1:], dtype=np.uint8)
    for i in range(out_size):
        first, count = int(bounds[i, 0]), int(bounds[i, 1])
        k = coeffs[i, :count].reshape((count,) + (1,) * (src.ndim - 1))
        acc = ROUND + (src[first:first + count] * k).sum(axis=0, dtype=np.int32)
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize_u8_reference(img_hwc, new_h, new_w):
    """uint8 [H, W, C] -> uint8 [new_h, new_w, C]: horizontal pass, then vertical pass on its uint8 result; a pass whose
    size does not change is skipped"""
    img = np.asarray(img_hwc)
    assert img.dtype == np.uint8 and img.ndim == 3, (img.dtype, img.shape)
    if img.shape[1] != new_w:
        img = _pass(img, new_w, 1)
    if img.shape[0] != new_h:
        img = _pass(img, new_h, 0)
    return np.ascontiguousarray(img)
