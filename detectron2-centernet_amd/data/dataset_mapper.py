"""The CenterNet project's dataset mapper.  Contract (reference: projects/CenterNet/center_net/dataset_mapper.py:17-175):
input one Detectron2 dataset dict; output a copy with "image" (uint8 CHW tensor, channel order INPUT.FORMAT) and, when
training, "instances" (gt_boxes XYXY in the resized image, gt_classes int64; crowd and empty boxes removed); the
"annotations" list is consumed.  Pipeline: read -> ResizeShortestEdge -> four colour jitters, each applied with probability
0.15 (training only) -> boxes through the same transform list.

INPUT.DEVICE_RESIZE (test time only): the resize is left to the model.  The record then carries "image_raw" (the uint8 HWC
array as read, channel order INPUT.FORMAT) and "resize_hw" (the size ResizeShortestEdge would have resized it to) instead
of "image"; CenterNet resizes the whole batch in one launch (ops.resize_u8) to the very bytes the host resize produces.

INPUT.DEVICE_AUGMENT (training only): resize AND colour jitters are left to the model.  The mapper decodes the image and makes
exactly the random draws of the host pipeline, in its order, from numpy's global RNG -- the size draw, per jitter the
apply-or-not uniform and, when it applies, its weight (or lighting's normal(size=3)); none of them depends on a pixel.  The
record carries "image_raw" (uint8 HWC torch tensor: shared memory across the loader's worker boundary), "resize_hw", "jitter"
(float64 [4, 4] tensor, data/jitter.py) and "instances" (the boxes through the resize alone: a colour transform moves no
coordinate).  CenterNet.stage_raw_train turns a batch of them into the bytes the host pipeline gives from the same draws.

INPUT.AFFINE.ENABLED (training only, not in the reference): CenterNet's random scale-and-crop sampler (T.RandomAffineCrop,
data/warp.py) takes ResizeShortestEdge's place as the first augmentation; every image leaves it at INPUT.AFFINE.OUTPUT_SIZE.
Its draws come first, the jitters' follow as before.  A raw record then also carries "warp" (float64 [2, 4] tensor,
data.warp.pack_warp: the inverse matrix and the flip flag) and "resize_hw" is the output size.

INPUT.AFFINE.TEST_MODE (test time only, not in the reference): "fix_res" / "keep_res" put CenterNet's test warp
(data.warp.test_params) in ResizeShortestEdge's place.  The record carries "warp" (never flipped) and the original "height" /
"width"; "image" holds the bytes of data.warp.warp_affine_u8_reference, or, with INPUT.DEVICE_RESIZE, "image_raw" / "resize_hw"
leave the warp to the model (ops.warp_affine_u8).  The model maps the boxes back through the inverse map."""
import copy

import numpy as np
import torch

from . import detection_utils as du
from . import transforms as T
from .jitter import JITTER_ORDER, empty_spec
from . import warp as W
from .warp import pack_warp

# colour jitters of the training pipeline (:36-43 of the reference mapper): (augmentation, constructor arguments)
_COLOUR_JITTER = ((T.RandomContrast, (0.8, 1.2)), (T.RandomBrightness, (0.8, 1.2)), (T.RandomSaturation, (0.8, 1.2)),
                  (T.RandomLighting, (0.8,)))
_JITTER_PROB = 0.15


def bulb_traffic_light_augmentation(cfg, is_train):
    """resize rule from INPUT.{MIN,MAX}_SIZE_{TRAIN,TEST}; training adds the colour jitters"""
    inp = cfg.INPUT
    if is_train:
        sizes, longest, style = inp.MIN_SIZE_TRAIN, inp.MAX_SIZE_TRAIN, inp.MIN_SIZE_TRAIN_SAMPLING
        if style == "range" and len(sizes) != 2:
            raise AssertionError("more than 2 ({}) min_size(s) are provided for ranges".format(len(sizes)))
    else:
        sizes, longest, style = inp.MIN_SIZE_TEST, inp.MAX_SIZE_TEST, "choice"
    pipeline = [T.ResizeShortestEdge(sizes, longest, style)]
    affine = getattr(inp, "AFFINE", None)
    if is_train and affine is not None and affine.ENABLED:      # CenterNet's sampler takes the resize's place
        pipeline = [T.RandomAffineCrop(cfg)]
    if is_train:
        pipeline += [T.RandomApply(aug(*args), prob=_JITTER_PROB) for aug, args in _COLOUR_JITTER]
    return pipeline


class TrafficLightDatasetMapper:
    def __init__(self, cfg, is_train=True):
        unsupported = [k for k in ("MASK_ON", "KEYPOINT_ON", "LOAD_PROPOSALS") if getattr(cfg.MODEL, k, False)]
        if unsupported:
            raise NotImplementedError(f"MODEL.{unsupported[0]}: masks / keypoints / proposals are not part of the CenterNet path")
        crop = getattr(cfg.INPUT, "CROP", None)
        if is_train and crop is not None and getattr(crop, "ENABLED", False):
            raise NotImplementedError("INPUT.CROP is off in the CenterNet configs and not built")
        self.is_train = is_train
        self.device_resize = bool(getattr(cfg.INPUT, "DEVICE_RESIZE", False))
        if self.device_resize and is_train:
            raise NotImplementedError("INPUT.DEVICE_RESIZE is a test-time switch: the training pipeline's colour jitters follow the "
                                      "resize on the host (build the training mapper with INPUT.DEVICE_RESIZE False; "
                                      "INPUT.DEVICE_AUGMENT moves the training resize and the jitters to the device)")
        self.device_augment = bool(getattr(cfg.INPUT, "DEVICE_AUGMENT", False)) and is_train      # test time: ignored
        # CenterNet's test input (INPUT.AFFINE.TEST_MODE): read at test time alone, checked there by name
        affine = getattr(cfg.INPUT, "AFFINE", None)
        self.test_mode = "" if (is_train or affine is None) else getattr(affine, "TEST_MODE", "")
        if self.test_mode != "":
            self.test_out_hw, self.test_div = tuple(affine.OUTPUT_SIZE), int(cfg.MODEL.CENTERNET.SIZE_DIVISIBILITY)
            W.check_test_mode(self.test_mode, self.test_out_hw, self.test_div)
        self.img_format = cfg.INPUT.FORMAT
        self.augmentation = bulb_traffic_light_augmentation(cfg, is_train)
        if self.device_augment:
            order = tuple(type(a.aug).__name__ for a in self.augmentation[1:])
            if order != JITTER_ORDER:
                raise NotImplementedError(
                    f"INPUT.DEVICE_AUGMENT: the device kernel applies {', '.join(JITTER_ORDER)} in that order (contrast first: its "
                    f"mean is the resized image's); _COLOUR_JITTER is now {', '.join(order)} -- train with INPUT.DEVICE_AUGMENT False")

    def _image(self, record):
        pixels = du.read_image(record["file_name"], format=self.img_format)
        du.check_image_size(record, pixels)
        return T.apply_augmentations(self.augmentation, pixels)

    @staticmethod
    def _targets(annotations, transforms, hw):
        kept = [du.transform_instance_annotations(a, transforms, hw) for a in annotations if not a.get("iscrowd", 0)]
        return du.filter_empty_instances(du.annotations_to_instances(kept, hw))

    def _raw_train_record(self, record):
        """INPUT.DEVICE_AUGMENT: the draws of the host pipeline, in its order, and no pixel work beyond the decode"""
        pixels = du.read_image(record["file_name"], format=self.img_format)
        du.check_image_size(record, pixels)
        resize = self.augmentation[0].get_transform(pixels)      # the size draw (INPUT.AFFINE: the sampler's draws); reads the image's shape only
        if isinstance(resize, T.AffineTransform):
            hw = (resize.out_h, resize.out_w)
            record["warp"] = torch.from_numpy(pack_warp(resize.Minv, resize.flip))
        else:
            hw = (resize.new_h, resize.new_w) if isinstance(resize, T.ResizeTransform) else tuple(pixels.shape[:2])
        spec = empty_spec()
        for t, apply in enumerate(self.augmentation[1:]):
            params = apply.draw()
            if params is not None:
                spec[t, 0], spec[t, 1:] = 1.0, apply.aug.spec_row(params)
        record["image_raw"] = torch.from_numpy(np.require(pixels, requirements="CW"))      # a copy only where the decoder's array is a view or read-only
        record["resize_hw"] = hw
        record["jitter"] = torch.from_numpy(spec)
        annotations = record.pop("annotations", None)
        if annotations is not None:
            record["instances"] = self._targets(annotations, T.TransformList([resize]), hw)
        return record

    def _affine_test_record(self, record):
        """INPUT.AFFINE.TEST_MODE: the image through CenterNet's test warp (data.warp.test_params), on the host ("image") or
        left to the model ("image_raw" / "resize_hw", INPUT.DEVICE_RESIZE); either way the record carries "warp" and the
        original "height" / "width", from which the model maps the boxes back"""
        pixels = du.read_image(record["file_name"], format=self.img_format)
        du.check_image_size(record, pixels)
        h, w = pixels.shape[:2]
        M, out_h, out_w = W.test_params(h, w, self.test_mode, self.test_out_hw, self.test_div)
        record["warp"] = torch.from_numpy(pack_warp(M, False))
        record["height"], record["width"] = h, w
        if self.device_resize:
            record["image_raw"] = np.ascontiguousarray(pixels)
            record["resize_hw"] = (out_h, out_w)
        else:
            warped = W.warp_affine_u8_reference(np.ascontiguousarray(pixels), M, out_h, out_w)
            record["image"] = torch.as_tensor(np.ascontiguousarray(warped.transpose(2, 0, 1)))
        record.pop("annotations", None)
        return record

    def __call__(self, dataset_dict):
        record = copy.deepcopy(dataset_dict)       # the caller's dict (shared by every epoch) is never modified
        if self.device_augment:
            return self._raw_train_record(record)
        if self.test_mode:
            return self._affine_test_record(record)
        if self.device_resize:
            pixels = du.read_image(record["file_name"], format=self.img_format)
            du.check_image_size(record, pixels)
            resize = self.augmentation[0]
            record["image_raw"] = np.ascontiguousarray(pixels)
            size = int(resize.short_edge_length[0])      # test time: one size ("choice" of MIN_SIZE_TEST); 0 = no resize
            record["resize_hw"] = (resize.output_size(pixels.shape[0], pixels.shape[1], size, resize.max_size) if size
                                   else tuple(pixels.shape[:2]))
            record.pop("annotations", None)
            return record
        pixels, transforms = self._image(record)
        record["image"] = torch.as_tensor(np.ascontiguousarray(pixels.transpose(2, 0, 1)))
        annotations = record.pop("annotations", None)
        if self.is_train and annotations is not None:
            record["instances"] = self._targets(annotations, transforms, pixels.shape[:2])
        return record
