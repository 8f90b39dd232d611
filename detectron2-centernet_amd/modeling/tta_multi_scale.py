"""`CenterNetWithTTA` as the package exports it: multi-scale testing (TEST.SOFT_NMS.ENABLED, CenterNet's `--nms`; DESIGN.md
section 7.10) on top of the single-pass wrappers.

modeling/test_time_augmentation.py (host resize of "image" records) and modeling/tta_device_resize.py (device resize of
"image_raw" records) are the single-pass wrapper: the flip test at no size or one size; they do not read TEST.SOFT_NMS.  This
class adds the rest.  With the switch on, every entry of TEST.AUG.MIN_SIZES is one pass through a single-size wrapper of this
class -- TEST.AUG.FLIP selects the flip engine per pass, `height` / `width` stay pinned to the original frame, so the passes'
boxes are comparable as they come -- and the passes' detections, still on the device, are merged by CenterNet's rule:
per-class Gaussian soft-NMS over their union (pass-major in the order of MIN_SIZES), then the TEST.DETECTIONS_PER_IMAGE best
(ops.soft_nms_merge: two launches, no host read between the last pass and the merge, one host synchronisation per batch).  No
size or one size with the switch on is one pass plus soft-NMS.  The reference holds no CenterNet merge: the rule is pinned by
a float64 restatement and hand-derived answers (tests/soft_nms_cases.py).  With the switch off nothing changes, except that
the refusal of several sizes names the switch."""
import itertools

import torch

from .. import ops
from .tta_device_resize import refuse_multi_scale_over_warped
from .tta_device_resize import CenterNetWithTTA as _SinglePassTTA

__all__ = ["CenterNetWithTTA"]


def _pass_cfg(cfg, min_sizes):
    """the configuration of one pass: a single-size (or no-size) wrapper with the merge off"""
    cfg = cfg.clone()
    cfg.defrost()
    cfg.TEST.AUG.MIN_SIZES, cfg.TEST.SOFT_NMS.ENABLED = tuple(min_sizes), False
    return cfg


class CenterNetWithTTA(_SinglePassTTA):
    __doc__ = _SinglePassTTA.__doc__ + """

    TEST.SOFT_NMS.ENABLED: any number of TEST.AUG.MIN_SIZES entries, one pass each (`self.passes`: single-size wrappers), merged
    by per-class Gaussian soft-NMS (SIGMA, MIN_SCORE) and cut to TEST.DETECTIONS_PER_IMAGE, best score first."""

    def __init__(self, cfg, model):
        refuse_multi_scale_over_warped(cfg)      # INPUT.AFFINE.TEST_MODE: no test sizes, no merge
        sizes = tuple(cfg.TEST.AUG.MIN_SIZES)
        self.soft_nms = bool(cfg.TEST.SOFT_NMS.ENABLED)
        # the single-pass wrapper checks the model, reads FLIP and owns the one-size resize; it is never shown several sizes
        super().__init__(_pass_cfg(cfg, sizes[:1]) if len(sizes) > 1 else cfg, model)
        self.cfg = cfg
        if len(sizes) > 1 and not self.soft_nms:
            raise NotImplementedError(
                f"TEST.AUG.MIN_SIZES={sizes}: multi-scale merging is per-class soft-NMS over the passes and is switched off: "
                "set TEST.SOFT_NMS.ENABLED (CenterNet's --nms) to merge several sizes, give one size, or () to keep the input "
                "size.")
        self.passes = []
        if self.soft_nms:
            self.passes = [CenterNetWithTTA(_pass_cfg(cfg, (s,)), model) for s in sizes] or \
                [CenterNetWithTTA(_pass_cfg(cfg, ()), model)]
            self.resize = self.passes[0].resize if len(sizes) == 1 else None
            self.sigma, self.min_score = float(cfg.TEST.SOFT_NMS.SIGMA), float(cfg.TEST.SOFT_NMS.MIN_SCORE)
            self.max_det = int(cfg.TEST.DETECTIONS_PER_IMAGE)

    def _to_device_once(self, batched_inputs):
        """multi-scale: raw records go to the device once -- the host images of the batch in ONE pinned copy, like
        CenterNet._stage_raw's -- and are resized from there for every size"""
        host = [i for i, inp in enumerate(batched_inputs)
                if "image_raw" in inp and not (isinstance(inp["image_raw"], torch.Tensor) and inp["image_raw"].is_cuda)]
        if not host:
            return batched_inputs
        raws = [torch.as_tensor(batched_inputs[i]["image_raw"]) for i in host]
        assert all(r.dtype == torch.uint8 for r in raws), "image_raw is uint8 [H, W, 3]"
        ends = list(itertools.accumulate(r.numel() for r in raws))
        pinned = torch.empty(ends[-1], dtype=torch.uint8, pin_memory=True)
        for r, end in zip(raws, ends):
            pinned[end - r.numel():end].copy_(r.reshape(-1))
        flat = pinned.to(self.model.device, non_blocking=True)
        out = list(batched_inputs)
        for i, r, end in zip(host, raws, ends):
            out[i] = dict(batched_inputs[i], image_raw=flat[end - r.numel():end].view(r.shape))
        return out

    def _packed(self, results):
        """a finished pass (a ragged batch comes back as Instances) as padded device tensors, what the merge reads"""
        dev = self.model.device
        insts = [r["instances"] for r in results]
        B, K = len(insts), max([len(i) for i in insts] + [1])
        boxes = torch.zeros(B, K, 4, dtype=torch.float32, device=dev)
        scores = torch.zeros(B, K, dtype=torch.float32, device=dev)
        classes = torch.zeros(B, K, dtype=torch.int32, device=dev)
        for b, i in enumerate(insts):
            n = len(i)
            boxes[b, :n], scores[b, :n], classes[b, :n] = i.pred_boxes.tensor, i.scores, i.pred_classes
        counts = torch.tensor([len(i) for i in insts], dtype=torch.int32).to(dev)
        return (boxes, scores, classes, counts), tuple(i.image_size for i in insts)

    def _merged_async(self, batched_inputs):
        """TEST.SOFT_NMS: one pass per test size (one pass as the images come when there is none), the passes' device tensors
        merged by ops.soft_nms_merge; the handle waits once, for the merged counts"""
        from .meta_arch.centernet import _EvalHandle
        if self.model.device.type != "cuda":
            raise NotImplementedError("the CenterNet HIP path has no CPU implementation (MODEL.DEVICE must be cuda)")
        batched_inputs = self._to_device_once(batched_inputs)
        passes, out_sizes = [], None
        for one in self.passes:
            # a pass's handle is only the carrier of its device tensors: no read-back of its counts, no event
            h = self.model.forward_async(one._inputs(batched_inputs), flip=self.flip, read_back=False)
            if isinstance(h, _EvalHandle):
                tensors, sizes = (h.boxes, h.scores, h.classes, h.counts), h.out_sizes
            else:      # a ragged batch ran eagerly and is finished; had it raised, the earlier passes' work is simply dropped
                tensors, sizes = self._packed(h.result())
            out_sizes = sizes if out_sizes is None else out_sizes
            assert tuple(sizes) == tuple(out_sizes), "every pass reports its boxes in the frame of the original image"
            passes.append(tensors)
        merged = ops.soft_nms_merge(passes, self.model.num_classes, self.sigma, self.min_score, self.max_det)
        return _EvalHandle(*merged, out_sizes)

    def forward_async(self, batched_inputs):
        """a handle whose .result() is what __call__ returns"""
        if not self.soft_nms:
            return super().forward_async(batched_inputs)
        self._check()
        return self._merged_async(batched_inputs)

    @torch.no_grad()
    def __call__(self, batched_inputs):
        if not self.soft_nms:
            return super().__call__(batched_inputs)
        self._check()
        return self._merged_async(batched_inputs).result()
