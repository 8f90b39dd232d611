"""`CenterNetWithTTA` for raw records (INPUT.DEVICE_RESIZE): the TEST.AUG.MIN_SIZES resize on the device.

modeling/test_time_augmentation.py resizes a record's "image" on the host: the image is copied to the host, resized with
Pillow and copied back.  A record that carries "image_raw" (the uint8 HWC image as read, what the test-time mapper emits with
INPUT.DEVICE_RESIZE) needs none of that: the wrapper only states the size -- "resize_hw", by the same ResizeShortestEdge rule
-- and the model resizes the batch in one launch (CenterNet._stage_raw -> ops.resize_u8), to the bytes Pillow gives.  Records
with "image" take the host code unchanged; `modeling.CenterNetWithTTA` is this class."""
from .test_time_augmentation import CenterNetWithTTA as _HostResizeTTA

__all__ = ["CenterNetWithTTA"]


def refuse_multi_scale_over_warped(cfg):
    """with INPUT.AFFINE.TEST_MODE set: refuses, by name, TEST.AUG.MIN_SIZES and TEST.SOFT_NMS.  Records of that mode arrive
    warped to the network's size: the flip test runs on them as on any input (the flip engine mirrors the warped
    network input, the unwarp follows the merge); a resize of a warped input and the multi-scale merge over warped inputs are
    not built"""
    sizes = tuple(cfg.TEST.AUG.MIN_SIZES)
    test_mode = getattr(getattr(cfg.INPUT, "AFFINE", None), "TEST_MODE", "")
    if test_mode and sizes:
        raise NotImplementedError(
            f"TEST.AUG.MIN_SIZES={sizes} with INPUT.AFFINE.TEST_MODE='{test_mode}': the test-time mapper already warps every "
            "image to the network's size; multi-scale testing over warped inputs is not built. Set TEST.AUG.MIN_SIZES to ().")
    if test_mode and bool(getattr(getattr(cfg.TEST, "SOFT_NMS", None), "ENABLED", False)):
        raise NotImplementedError(
            f"TEST.SOFT_NMS.ENABLED with INPUT.AFFINE.TEST_MODE='{test_mode}': the soft-NMS merge belongs to multi-scale "
            "testing, which is not built over warped inputs. Set TEST.SOFT_NMS.ENABLED to False.")


class CenterNetWithTTA(_HostResizeTTA):
    __doc__ = _HostResizeTTA.__doc__

    def __init__(self, cfg, model):
        refuse_multi_scale_over_warped(cfg)      # before anything else: the refusal names the keys whatever the model is
        super().__init__(cfg, model)

    def _inputs(self, batched_inputs):
        """the inputs at the test size, `height` / `width` pinned to the frame the boxes are wanted in"""
        if self.resize is None or not any("image_raw" in inp for inp in batched_inputs):
            return super()._inputs(batched_inputs)
        out = []
        for inp in batched_inputs:
            if "image_raw" not in inp:
                out.extend(super()._inputs([inp]))
                continue
            h, w = inp["image_raw"].shape[:2]
            size = self.resize.output_size(h, w, self.resize.short_edge_length[0], self.resize.max_size)
            out.append(dict(inp, height=inp.get("height", h), width=inp.get("width", w), resize_hw=size))
        return out
