"""The arithmetic of the training mapper's colour jitters, restated per byte.

The mapper (dataset_mapper.py) applies, after the resize, RandomContrast, RandomBrightness, RandomSaturation and
RandomLighting in that order, each with probability 0.15, each a `BlendTransform(src, ws, wd)` on the uint8 result of the one
before (transforms.py).  For a uint8 image numpy evaluates that blend as

    out = trunc(clip(f64(ws) * src  +  f64(f32(wd) * f32(byte)), 0, 255))

-- `ws * src` one float64 product, `wd * byte` one float32 product widened to float64, one float64 add, nothing fused; then
the clip, then the truncation of `astype(uint8)`.  `src` is

    contrast     f64(S) / f64(3 h w), S the integer sum of the bytes of the image at that point      ws, wd = 1 - w, w
    brightness   0                                                                                   ws, wd = 1 - w, w
    saturation   (c0 * 0.299 + c1 * 0.587) + c2 * 0.114 per pixel, float64, channels as stored      ws, wd = 1 - w, w
    lighting     eigen_vecs.dot(weights * eigen_vals)[c], formed on the host in float64              ws, wd = 1, 1

The HIP kernel (csrc/jitter.hip) evaluates exactly this; `colour_jitter_reference` is the same in numpy, what the tests
compare with the chain of host transforms byte for byte.  The host code stays the arbiter.

A record's draws travel as a "jitter spec": float64 [4, 4], row t = transform t of JITTER_ORDER,
    (drawn, ws, wd, 0) for the three blends,  (drawn, offset c0, offset c1, offset c2) for lighting."""
import numpy as np

JITTER_ORDER = ("RandomContrast", "RandomBrightness", "RandomSaturation", "RandomLighting")


def empty_spec():
    return np.zeros((4, 4), dtype=np.float64)


def spec_array(spec):
    """a jitter spec (numpy array, torch tensor, or None = nothing drawn) as float64 [4, 4]"""
    if spec is None:
        return empty_spec()
    spec = np.asarray(spec.numpy() if hasattr(spec, "numpy") else spec, dtype=np.float64)
    assert spec.shape == (4, 4), f"a jitter spec is float64 [4, 4], got {spec.shape}"
    return spec


def _blend(ws, src, wd, img):
    f = np.float32(wd) * img.astype(np.float32)                     # float32 product
    v = np.float64(ws) * np.asarray(src, dtype=np.float64) + f.astype(np.float64)
    return np.clip(v, 0, 255).astype(np.uint8)


def colour_jitter_reference(img_hwc, spec):
    """uint8 [h, w, 3] -> the jittered uint8 [h, w, 3] of the draws in `spec`, by the arithmetic above"""
    img = np.asarray(img_hwc)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3, (img.dtype, img.shape)
    spec = spec_array(spec)
    if spec[0, 0]:
        mean = np.float64(int(img.sum(dtype=np.uint64))) / np.float64(img.size)
        img = _blend(spec[0, 1], mean, spec[0, 2], img)
    if spec[1, 0]:
        img = _blend(spec[1, 1], 0.0, spec[1, 2], img)
    if spec[2, 0]:
        c = img.astype(np.float64)
        grey = (c[..., 0] * 0.299 + c[..., 1] * 0.587) + c[..., 2] * 0.114
        img = _blend(spec[2, 1], grey[:, :, None], spec[2, 2], img)
    if spec[3, 0]:
        img = _blend(1.0, spec[3, 1:4], 1.0, img)
    return img
