"""`CenterNetWithTTA` for raw records (INPUT.DEVICE_RESIZE): the TEST.AUG.MIN_SIZES resize on the device.

modeling/test_time_augmentation.py resizes a record's "image" on the host: the image is copied to the host, resized with
Pillow and copied back.  A record that carries "image_raw" (the uint8 HWC image as read, what the test-time mapper emits with
INPUT.DEVICE_RESIZE) needs none of that: the wrapper only states the size -- "resize_hw", by the same ResizeShortestEdge rule
-- and the model resizes the batch in one launch (CenterNet._stage_raw -> ops.resize_u8), to the bytes Pillow gives.  Records
with "image" take the host code unchanged; `modeling.CenterNetWithTTA` is this class."""
from .test_time_augmentation import CenterNetWithTTA as _HostResizeTTA

__all__ = ["CenterNetWithTTA"]


class CenterNetWithTTA(_HostResizeTTA):
    __doc__ = _HostResizeTTA.__doc__

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
