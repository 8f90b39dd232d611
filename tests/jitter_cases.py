"""The cases of the colour-jitter tests (test_jitter_host.py, test_jitter_gpu.py): sizes, images and parameter sets, each
with the reason it is there, and the host chain they are compared with -- the very BlendTransforms the training mapper
builds (data/transforms.py), applied in the mapper's order."""
import numpy as np

from detectron2_centernet_amd.data import transforms as T
from detectron2_centernet_amd.data.jitter import empty_spec

TILE_W, TILE_H = 64, 4      # pixel tile of one block of csrc/jitter.hip (JITTER_TW x JITTER_TH); test_jitter_host.py pins both

# (name, (h, w), what it is there for)
SIZES = [
    ("one_pixel", (1, 1), "one pixel: one live thread in the grid"),
    ("one_row", (1, TILE_W + 1), "one row, tile width + 1: a second block with one live column"),
    ("tall", (TILE_H + 1, 3), "tile height + 1: a second block row with one live row"),
    ("odd", (37, 53), "odd sizes, several block rows, a partial tile in both axes"),
]
SUM_SIZE = (2400, 2400)     # all-255: 3 * 2400 * 2400 * 255 > 2**32, for the byte sum only

IMAGES = ("random", "checker", "white", "black")

AUGS = (T.RandomContrast(0.8, 1.2), T.RandomBrightness(0.8, 1.2), T.RandomSaturation(0.8, 1.2), T.RandomLighting(0.8))
LIGHT_POS = np.array([0.31, 0.07, 0.52])        # offsets of a few tenths of a grey level, as the transform draws them
LIGHT_NEG = np.array([-0.27, -0.61, -0.04])
LIGHT_MIX = np.array([0.45, -0.33, 0.0])


def _params():
    """name -> per-transform parameters (None = not drawn): what Augmentation.draw() returns"""
    out = {"none": (None, None, None, None)}
    for t, name in enumerate(("contrast", "brightness", "saturation")):
        for w in (0.8, 1.0, 1.2):      # 1.0: brightness must be the identity; 1.2 clips at 255, 0.8 exercises the truncation
            p = [None] * 4
            p[t] = w
            out[f"{name}_{w}"] = tuple(p)
    for name, off in (("light_pos", LIGHT_POS), ("light_neg", LIGHT_NEG), ("light_mix", LIGHT_MIX)):
        out[name] = (None, None, None, off)
    out["all_four"] = (1.1373, 0.8641, 1.1902, LIGHT_MIX)
    out["all_four_low"] = (0.8123, 1.1999, 0.8005, LIGHT_NEG)
    return out


PARAMS = _params()


def make_image(kind, h, w, seed=0):
    """uint8 [h, w, 3]: random bytes; a 0/255 checker; constant 255 (the upper clip under brightness and contrast above 1);
    constant 0 (a negative lighting offset must clip at 0, a positive one below 1 must truncate back to 0)"""
    if kind == "random":
        return np.random.RandomState(seed).randint(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "checker":
        yy, xx = np.mgrid[0:h, 0:w]
        return np.ascontiguousarray((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None].repeat(3, 2))
    return np.full((h, w, 3), {"white": 255, "black": 0}[kind], dtype=np.uint8)


def spec_of(params):
    """the jitter spec (float64 [4, 4]) of a parameter set, built the way the raw-record mapper builds it"""
    spec = empty_spec()
    for t, (aug, p) in enumerate(zip(AUGS, params)):
        if p is not None:
            spec[t, 0], spec[t, 1:] = 1.0, aug.spec_row(p)
    return spec


def host_chain(img_hwc, params):
    """the host pipeline's result: each drawn transform built from the image it arrives at and applied to it"""
    img = np.ascontiguousarray(img_hwc)
    for aug, p in zip(AUGS, params):
        if p is not None:
            img = aug.transform_of(p, img).apply_image(img)
    return img


def all_cases():
    """(id, image HWC, parameter set) for every size x image x parameter set"""
    for i, (sname, (h, w), _) in enumerate(SIZES):
        for kind in IMAGES:
            for pname, params in PARAMS.items():
                yield f"{sname}-{kind}-{pname}", make_image(kind, h, w, seed=i), params
