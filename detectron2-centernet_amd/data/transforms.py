"""Image / box transforms and the augmentations the CenterNet dataset mapper uses (host side, numpy + PIL).

Reference: detectron2/data/transforms/augmentation_impl.py (ResizeShortestEdge :123-173, RandomApply :26-68,
RandomContrast :406-431, RandomBrightness :434-457, RandomSaturation :460-486, RandomLighting :489-515, RandomFlip
:71-101), transform.py (ResizeTransform :83-136).  The Transform base classes (`Transform`, `TransformList`,
`BlendTransform`, `HFlipTransform`, `NoOpTransform`) come from the third-party package fvcore
(`fvcore.transforms.transform`, not in the reference tree and unpinned): restated here from their published behaviour --
`apply_box` maps the four corners and takes the axis-aligned hull; `BlendTransform` computes
`src_weight * src_image + dst_weight * img` in float32 and clips uint8 images to [0, 255]."""
import sys

import numpy as np
from PIL import Image

from . import warp as W


class Transform:
    def apply_image(self, img):
        raise NotImplementedError

    def apply_coords(self, coords):
        raise NotImplementedError

    def apply_box(self, box):
        """box: [N,4] XYXY -> axis-aligned hull of the transformed corners"""
        box = np.asarray(box, dtype=np.float64).reshape(-1, 4)
        idxs = np.array([(0, 1), (2, 1), (0, 3), (2, 3)]).flatten()
        coords = box[:, idxs].reshape(-1, 2)
        coords = self.apply_coords(coords).reshape((-1, 4, 2))
        minxy, maxxy = coords.min(axis=1), coords.max(axis=1)
        return np.concatenate((minxy, maxxy), axis=1)


class NoOpTransform(Transform):
    def apply_image(self, img):
        return img

    def apply_coords(self, coords):
        return coords


class ResizeTransform(Transform):
    def __init__(self, h, w, new_h, new_w, interp=None):
        self.h, self.w, self.new_h, self.new_w = h, w, new_h, new_w
        self.interp = Image.BILINEAR if interp is None else interp

    def apply_image(self, img, interp=None):
        assert img.shape[:2] == (self.h, self.w), (img.shape, self.h, self.w)
        if img.dtype != np.uint8:
            raise NotImplementedError("the mapper resizes uint8 images (transform.py:105-109); float images are not on the path")
        pil = Image.fromarray(img).resize((self.new_w, self.new_h), interp if interp is not None else self.interp)
        return np.asarray(pil)

    def apply_coords(self, coords):
        coords = np.asarray(coords, dtype=np.float64)
        coords[:, 0] = coords[:, 0] * (self.new_w * 1.0 / self.w)
        coords[:, 1] = coords[:, 1] * (self.new_h * 1.0 / self.h)
        return coords


class HFlipTransform(Transform):
    def __init__(self, width):
        self.width = width

    def apply_image(self, img):
        return np.flip(img, axis=1)

    def apply_coords(self, coords):
        coords = np.asarray(coords, dtype=np.float64)
        coords[:, 0] = self.width - coords[:, 0]
        return coords


class AffineTransform(Transform):
    """one affine warp of a uint8 image to out_h x out_w (data/warp.py holds every definition): Minv [2, 3] maps a destination
    pixel index to a source pixel index, of the mirrored image when `flip`"""

    def __init__(self, Minv, flip, out_h, out_w, src_w=None):
        self.Minv, self.flip = np.asarray(Minv, dtype=np.float64).reshape(2, 3), bool(flip)
        self.out_h, self.out_w = int(out_h), int(out_w)
        self.w = src_w      # the source width the mirror of a coordinate needs; None: learnt from the image apply_image gets

    def apply_image(self, img):
        assert self.w is None or self.w == img.shape[1], (self.w, img.shape)
        self.w = img.shape[1]
        return W.warp_affine_u8_reference(img, self.Minv, self.out_h, self.out_w, self.flip)

    def apply_coords(self, coords):
        assert self.w is not None or not self.flip, "a flipped AffineTransform maps coordinates once it knows the source width"
        return W.forward_coords(coords, self.Minv, self.flip, self.w)


class BlendTransform(Transform):
    def __init__(self, src_image, src_weight, dst_weight):
        self.src_image, self.src_weight, self.dst_weight = src_image, src_weight, dst_weight

    def apply_image(self, img, interp=None):
        if img.dtype == np.uint8:
            src = np.asarray(self.src_image)
            if src.size in (1, img.shape[-1]) and img.ndim == 3:
                # per-channel affine map of a byte: tabulate the 256 results with the very expression below (same dtypes,
                # same rounding) and look the pixels up -- 5 float passes over the image become one gather
                ramp = np.arange(256, dtype=np.uint8).reshape(256, 1).repeat(img.shape[-1], 1)
                lut = np.clip(self.src_weight * src.reshape(-1) + self.dst_weight * ramp.astype(np.float32), 0, 255).astype(np.uint8)
                if img.shape[-1] == 3:     # PIL applies a 3 x 256 table to an RGB image in C
                    pil = Image.fromarray(np.ascontiguousarray(img)).point(lut.T.reshape(-1).tolist())
                    return np.asarray(pil)
                return np.stack([np.take(lut[:, c], img[..., c]) for c in range(img.shape[-1])], axis=-1)
            out = self.src_weight * self.src_image + self.dst_weight * img.astype(np.float32)
            return np.clip(out, 0, 255).astype(np.uint8)
        return self.src_weight * self.src_image + self.dst_weight * img

    def apply_coords(self, coords):
        return coords


class TransformList(Transform):
    def __init__(self, transforms):
        self.transforms = []
        for t in transforms:     # flattened, no-ops dropped (fvcore does the same)
            if isinstance(t, TransformList):
                self.transforms.extend(t.transforms)
            elif not isinstance(t, NoOpTransform):
                self.transforms.append(t)

    def apply_image(self, img):
        for t in self.transforms:
            img = t.apply_image(img)
        return img

    def apply_coords(self, coords):
        for t in self.transforms:
            coords = t.apply_coords(coords)
        return coords

    def apply_box(self, box):
        for t in self.transforms:
            box = t.apply_box(box)
        return np.asarray(box, dtype=np.float64).reshape(-1, 4)

    def __len__(self):
        return len(self.transforms)


# ------------------------------------------------------------------------------------------ augmentations
class Augmentation:
    """get_transform(image) -> Transform; draws from numpy's global RNG like the reference"""

    def get_transform(self, image):
        raise NotImplementedError


class ResizeShortestEdge(Augmentation):
    def __init__(self, short_edge_length, max_size=sys.maxsize, sample_style="range", interp=Image.BILINEAR):
        assert sample_style in ("range", "choice"), sample_style
        self.is_range = sample_style == "range"
        if isinstance(short_edge_length, int):
            short_edge_length = (short_edge_length, short_edge_length)
        if self.is_range:
            assert len(short_edge_length) == 2, short_edge_length
        self.short_edge_length, self.max_size, self.interp = tuple(short_edge_length), max_size, interp

    @staticmethod
    def output_size(h, w, size, max_size):
        """the size rule of augmentation_impl.py:162-172"""
        scale = size * 1.0 / min(h, w)
        if h < w:
            newh, neww = size, scale * w
        else:
            newh, neww = scale * h, size
        if max(newh, neww) > max_size:
            scale = max_size * 1.0 / max(newh, neww)
            newh, neww = newh * scale, neww * scale
        return int(newh + 0.5), int(neww + 0.5)

    def draw_size(self, h, w):
        """the size draw: (new_h, new_w) of an h x w image, or None when the drawn size is 0 (no resize)"""
        if self.is_range:
            size = np.random.randint(self.short_edge_length[0], self.short_edge_length[1] + 1)
        else:
            size = np.random.choice(self.short_edge_length)
        if size == 0:
            return None
        return self.output_size(h, w, int(size), self.max_size)

    def get_transform(self, image):
        h, w = image.shape[:2]
        new = self.draw_size(h, w)
        if new is None:
            return NoOpTransform()
        return ResizeTransform(h, w, new[0], new[1], self.interp)


class RandomApply(Augmentation):
    def __init__(self, aug, prob=0.5):
        assert 0.0 <= prob <= 1.0
        self.aug, self.prob = aug, prob

    def draw(self):
        """the apply-or-not uniform, then the wrapped augmentation's own draws: its parameters, or None when it is not applied"""
        if np.random.uniform(0, 1) < self.prob:
            return self.aug.draw()
        return None

    def get_transform(self, image):
        params = self.draw()
        if params is None:
            return NoOpTransform()
        return self.aug.transform_of(params, image)


class RandomFlip(Augmentation):
    def __init__(self, prob=0.5):
        self.prob = prob

    def get_transform(self, image):
        if np.random.uniform(0, 1) < self.prob:
            return HFlipTransform(image.shape[1])
        return NoOpTransform()


class RandomAffineCrop(Augmentation):
    """CenterNet's training sampler (INPUT.AFFINE): a random centre inside a border, a scale from a list, a flip, one warp to a
    fixed size.  In two halves like the colour jitters: draw(h, w) makes the draws (none depends on a pixel),
    transform_of(params, image) builds the AffineTransform."""

    def __init__(self, cfg):
        a = cfg.INPUT.AFFINE
        self.out_h, self.out_w = (int(v) for v in a.OUTPUT_SIZE)
        div = int(cfg.MODEL.CENTERNET.SIZE_DIVISIBILITY)
        if self.out_h < 1 or self.out_w < 1 or (div > 0 and (self.out_h % div or self.out_w % div)):
            raise ValueError(f"INPUT.AFFINE.OUTPUT_SIZE {tuple(a.OUTPUT_SIZE)}: (out_h, out_w), each a positive multiple of "
                             f"MODEL.CENTERNET.SIZE_DIVISIBILITY ({div})")
        self.scales = tuple(float(v) for v in a.SCALES)
        if not self.scales or min(self.scales) <= 0:
            raise ValueError(f"INPUT.AFFINE.SCALES {tuple(a.SCALES)}: at least one positive scale")
        self.border, self.flip_prob = int(a.BORDER), float(a.FLIP_PROB)
        if self.border < 0 or not 0.0 <= self.flip_prob <= 1.0:
            raise ValueError(f"INPUT.AFFINE: BORDER {a.BORDER} must not be negative, FLIP_PROB {a.FLIP_PROB} lies in [0, 1]")

    def draw(self, h, w):
        """(s, cx, cy, flip) for an h x w source, data.warp.draw_params"""
        return W.draw_params(h, w, self.scales, self.border, self.flip_prob)

    def transform_of(self, params, image):
        s, cx, cy, flip = params
        w = image.shape[1]
        return AffineTransform(W.inverse_matrix(s, cx, cy, flip, w, self.out_h, self.out_w), flip, self.out_h, self.out_w, src_w=w)

    def get_transform(self, image):
        return self.transform_of(self.draw(*image.shape[:2]), image)


class _ColourJitter(Augmentation):
    """a colour jitter in two halves: draw() makes the random draws (none depends on the pixels) and returns the parameters,
    transform_of(params, image) builds the BlendTransform from them.  The host pipeline runs both (get_transform); the
    raw-record mapper (INPUT.DEVICE_AUGMENT) runs draw() alone and ships spec_row(params) to the device kernel."""

    def draw(self):
        raise NotImplementedError

    def transform_of(self, params, image):
        raise NotImplementedError

    def spec_row(self, params):
        """the three numbers of this transform's row of a jitter spec (data/jitter.py)"""
        raise NotImplementedError

    def get_transform(self, image):
        return self.transform_of(self.draw(), image)


class _RandomIntensity(_ColourJitter):
    def __init__(self, intensity_min, intensity_max):
        self.intensity_min, self.intensity_max = intensity_min, intensity_max

    def draw(self):
        return np.random.uniform(self.intensity_min, self.intensity_max)

    def spec_row(self, w):
        return (1 - w, w, 0.0)      # (src_weight, dst_weight) exactly as transform_of forms them


class RandomContrast(_RandomIntensity):
    def transform_of(self, w, image):
        return BlendTransform(src_image=image.mean(), src_weight=1 - w, dst_weight=w)


class RandomBrightness(_RandomIntensity):
    def transform_of(self, w, image):
        return BlendTransform(src_image=0, src_weight=1 - w, dst_weight=w)


class RandomSaturation(_RandomIntensity):
    def transform_of(self, w, image):
        assert image.shape[-1] == 3, "RandomSaturation only works on RGB images"
        # image.dot([0.299, 0.587, 0.114]) in the reference: the same float64 sum channel by channel (numpy's generic
        # uint8 x float64 dot is 6x slower)
        grayscale = (image[..., 0] * 0.299 + image[..., 1] * 0.587 + image[..., 2] * 0.114)[:, :, np.newaxis]
        return BlendTransform(src_image=grayscale, src_weight=1 - w, dst_weight=w)


class RandomLighting(_ColourJitter):
    """AlexNet's PCA lighting noise with the fixed ImageNet eigen-decomposition (augmentation_impl.py:505-508)"""

    def __init__(self, scale):
        self.scale = scale
        self.eigen_vecs = np.array([[-0.5675, 0.7192, 0.4009], [-0.5808, -0.0045, -0.8140], [-0.5836, -0.6948, 0.4203]])
        self.eigen_vals = np.array([0.2175, 0.0188, 0.0045])

    def draw(self):
        """the per-channel offsets"""
        weights = np.random.normal(scale=self.scale, size=3)
        return self.eigen_vecs.dot(weights * self.eigen_vals)

    def spec_row(self, offsets):
        return tuple(float(v) for v in offsets)

    def transform_of(self, offsets, image):
        assert image.shape[-1] == 3, "RandomLighting only works on RGB images"
        return BlendTransform(src_image=offsets, src_weight=1.0, dst_weight=1.0)


def apply_augmentations(augmentations, image):
    """run the augmentations in order on `image` (each sees the output of the previous one, like
    StandardAugInput.apply_augmentations); returns (image, TransformList)"""
    tfms = []
    for aug in augmentations:
        t = aug.get_transform(image) if isinstance(aug, Augmentation) else aug
        image = t.apply_image(image)
        tfms.append(t)
    return image, TransformList(tfms)
