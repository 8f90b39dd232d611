"""What the COCO, Pascal VOC and LVIS box-AP scorers share on the Python side: `cells_csr`, the ground-truth layout the
matchers read; `DeviceScorer`, the base of the device drivers (`COCOevalHIP`; `VOCevalHIP` and `LVISevalHIP`, which also take
their common outputs and their status-word check from it); `BoxEvaluator`, the base of the dataset evaluators.  A refusal
names the class that makes it."""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from .evaluator import DatasetEvaluator


def cells_csr(cell, I, K):
    """cell = image * K + class of every ground truth -> (stable order by cell, CSR offsets i32 [I*K+1], and the image and
    class index of every ground truth in that order)"""
    order = np.argsort(cell, kind="stable")
    off = np.zeros(I * K + 1, dtype=np.int32)
    np.cumsum(np.bincount(cell, minlength=I * K), out=off[1:])
    by_cell = cell[order]
    return order, off, (by_cell // K if K else cell).astype(np.int32), (by_cell % K if K else cell).astype(np.int32)


def ptr(t):
    return C.c_void_p(t.data_ptr() if t is not None else None)


class DeviceScorer:
    """the detections of a whole dataset as DEVICE tensors, normalised in `_dt`: boxes f32 [N,4], scores f32, classes, image i32.
    `IMAGE_LIST`, `status_message`, `_outputs` and `_check_status` serve only the scorers whose match call has a status word
    (`VOCevalHIP`, `LVISevalHIP`); `COCOevalHIP` uses none of them."""

    IMAGE_LIST = "the ground truth's image list"      # what a scorer calls the images its `image` indices point into

    def __init__(self, gt, boxes, scores, classes, image):
        for name, t in (("boxes", boxes), ("scores", scores), ("classes", classes), ("image", image)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise NotImplementedError(f"{type(self).__name__}: `{name}` must be a tensor on the GPU; scoring runs in HIP "
                                          "kernels and there is no CPU fallback")
        self._gt, self._device = gt, boxes.device
        self._dt = (boxes.detach().float().reshape(-1, 4).contiguous(), scores.detach().float().contiguous(),
                    classes.detach().to(torch.int32).contiguous(), image.detach().to(torch.int32).contiguous())

    def _up(self, a, f64=False):
        return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64) if f64 else a).to(self._device)

    def _workspace(self, nbytes, refusal):
        """nbytes of a *_workspace_bytes entry point, 0 = refused: raises refusal(its text) -> (owning tensor, aligned address)"""
        if nbytes == 0:
            raise refusal(_lib.lib().ctdet_last_error().decode())
        ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=self._device)
        return ws, C.c_void_p((ws.data_ptr() + 255) & ~255)

    def _call(self, fn, *args):
        """an entry point on the detections' device and its current stream (the last argument); a failure raises its text"""
        with torch.cuda.device(self._device):
            _lib.check(fn(*args, C.c_void_p(torch.cuda.current_stream(self._device).cuda_stream)), fn.__name__)

    @classmethod
    def status_message(cls, status):
        """the causes in a match call's status word (the EVAL_BAD_* bits of csrc/eval_common.h)"""
        causes = ((1, "a class index outside [0, K)"), (2, f"an image index outside {cls.IMAGE_LIST}"),
                  (4, "a score that is not finite"), (8, "a box coordinate that is not finite"))
        return "; ".join(text for bit, text in causes if status & bit)

    def _outputs(self, N, K, ncol):
        """what every match call writes: order i32 [N], cls_off i32 [K+1], flags u8 [N, ncol], the status word"""
        return (torch.empty(N, dtype=torch.int32, device=self._device), torch.empty(K + 1, dtype=torch.int32, device=self._device),
                torch.empty((N, ncol), dtype=torch.uint8, device=self._device), torch.empty(1, dtype=torch.int32, device=self._device))

    def _check_status(self, status):
        """the one synchronisation of a scorer: reads the status word into `self.status`; invalid detections raise their causes"""
        self.status = int(status.item())
        if self.status:
            raise ValueError(f"{type(self).__name__}: the detections hold " + self.status_message(self.status))


class BoxEvaluator(DatasetEvaluator):
    """`process()` keeps the device tensors of every image's `Instances`; nothing is copied to the host per image"""

    def reset(self):
        self._image_ids, self._counts, self._boxes, self._scores, self._classes = [], [], [], [], []

    def _instances(self, out):
        """the `Instances` of one output dict, or None to pass the image over"""
        return out["instances"]

    def process(self, inputs, outputs):
        for inp, out in zip(inputs, outputs):
            inst = self._instances(out)
            if inst is None:
                continue
            boxes, scores, classes = inst.pred_boxes.tensor, inst.scores, inst.pred_classes
            if not (boxes.is_cuda and scores.is_cuda and classes.is_cuda):
                raise NotImplementedError(f"{type(self).__name__}: the Instances must be on the GPU; scoring runs in HIP "
                                          "kernels and there is no CPU fallback")
            self._image_ids.append(inp["image_id"])
            self._counts.append(int(scores.shape[0]))
            self._boxes.append(boxes.detach())
            self._scores.append(scores.detach())
            self._classes.append(classes.detach())

    def _local(self):
        """this rank's detections, concatenated on the device: (image ids, counts, boxes, scores, classes)"""
        if not self._boxes:
            return [], [], None, None, None
        return (self._image_ids, self._counts, torch.cat(self._boxes).float().reshape(-1, 4), torch.cat(self._scores).float(),
                torch.cat(self._classes).to(torch.int32))

    def _checked(self, ids, boxes, scores, classes, where, refuse=True):
        """refuses predictions for image ids outside the ground truth (`where`); gathered numpy shards go onto the device"""
        known = set(self._gt["image_ids"]) if refuse else ()
        unknown = [i for i in ids if i not in known] if refuse else ()
        if unknown:
            raise ValueError(f"{type(self).__name__}: predictions for image ids that are not in {where}: {unknown[:5]}")
        if isinstance(boxes, torch.Tensor):
            return boxes, scores, classes
        dev = torch.device("cuda", torch.cuda.current_device())
        return tuple(torch.as_tensor(a).to(dev) for a in (boxes, scores, classes))

    def _image_of(self, ids, counts, dev):
        """i32 [N]: the index into the ground truth's images of every detection"""
        index = {v: i for i, v in enumerate(self._gt["image_ids"])}
        per_image = np.array([index[i] for i in ids], dtype=np.int32)
        return torch.as_tensor(np.repeat(per_image, np.array(counts, dtype=np.int64))).to(dev)
