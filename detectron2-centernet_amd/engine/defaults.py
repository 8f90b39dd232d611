"""`DefaultPredictor`: one image in, its detections out (reference: detectron2/engine/defaults.py:154-218).

Contract of the reference: build the model from the config, load `cfg.MODEL.WEIGHTS` through DetectionCheckpointer, take a
BGR uint8 HWC array, reverse the channel order when `INPUT.FORMAT` is "RGB", resize with ResizeShortestEdge(MIN_SIZE_TEST,
MAX_SIZE_TEST) and return `model([inputs])[0]`, boxes in the frame of the original image.

What differs here: the resize runs on the device.  The frame goes to the model as a raw record ("image_raw" / "resize_hw",
the records of a mapper built with INPUT.DEVICE_RESIZE); the RGB reversal is a view with channel stride -1 that the resize
kernel reads as it is, so the host touches the pixels once, for the pinned upload.  The result equals what the host resize
gives: the resized bytes are identical (ops.resize_u8)."""
import numpy as np
import torch

from ..checkpoint import DetectionCheckpointer
from ..data import MetadataCatalog
from ..data import transforms as T
from ..modeling.meta_arch.build import build_model

__all__ = ["DefaultPredictor"]


class DefaultPredictor:
    """`pred = DefaultPredictor(cfg); outputs = pred(bgr_image)` -- {"instances": Instances} of that one image"""

    def __init__(self, cfg):
        self.cfg = cfg.clone()      # cfg can be modified by the model
        self.model = build_model(self.cfg)
        self.model.eval()
        if len(cfg.DATASETS.TEST):
            self.metadata = MetadataCatalog.get(cfg.DATASETS.TEST[0])
        DetectionCheckpointer(self.model).load(cfg.MODEL.WEIGHTS)
        self.aug = T.ResizeShortestEdge([cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MIN_SIZE_TEST], cfg.INPUT.MAX_SIZE_TEST)
        self.input_format = cfg.INPUT.FORMAT
        assert self.input_format in ["RGB", "BGR"], self.input_format

    def __call__(self, original_image):
        """original_image: np.ndarray uint8 (H, W, 3) in BGR order"""
        original_image = np.asarray(original_image)
        if original_image.dtype != np.uint8 or original_image.ndim != 3 or original_image.shape[2] != 3:
            raise TypeError(f"DefaultPredictor takes a uint8 (H, W, 3) image, got {original_image.dtype} {original_image.shape}")
        with torch.no_grad():
            if self.input_format == "RGB":
                original_image = original_image[:, :, ::-1]      # a view: the device resize reads channel stride -1
            height, width = original_image.shape[:2]
            size = int(self.aug.short_edge_length[0])
            resize_hw = self.aug.output_size(height, width, size, self.aug.max_size) if size else (height, width)
            inputs = {"image_raw": original_image, "resize_hw": resize_hw, "height": height, "width": width}
            return self.model([inputs])[0]
