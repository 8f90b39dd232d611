"""Pascal VOC box-AP scoring on the device: `VOCevalHIP` drives the two entry points of libctdet_voceval.so
(ctdet_voceval_match / ctdet_voceval_ap, csrc/voceval.hip) over the detections of a whole dataset, the role `voc_eval` has
in the reference (detectron2/evaluation/pascal_voc_evaluation.py) -- once for every class and threshold instead of once per
(class, threshold).  DESIGN.md 7.16 holds the rule.  There is no CPU fallback: detections on the CPU are refused by name."""
import ctypes as C
import os

import numpy as np
import torch

from .. import _lib
from ..data.pascal_voc import read_voc_ids, read_voc_objects

# status bits of ctdet_voceval_match (CTDET_VOC_BAD_* in include/ctdet_voceval.h)
STATUS_CAUSES = ((1, "a class index outside [0, K)"), (2, "an image index outside the split's image list"),
                 (4, "a score that is not finite"), (8, "a box coordinate that is not finite"))

# the reference's `np.arange(0.0, 1.1, 0.1)`: the recall points of the 11-point form, as numpy rounds them
RECALL_POINTS_07 = np.arange(0.0, 1.1, 0.1)


def prepare_voc_ground_truth(image_ids, class_names, objects):
    """objects: (image index, class index, difficult, [xmin, ymin, xmax, ymax]) in file order -> the arrays the matcher takes:
    stable-sorted by (image, class) cell with CSR offsets [I*K+1]; boxes f64 as written (1-based)"""
    I, K, n = len(image_ids), len(class_names), len(objects)
    cell = np.array([o[0] * K + o[1] for o in objects], dtype=np.int64).reshape(n)
    order = np.argsort(cell, kind="stable")
    boxes = np.array([objects[j][3] for j in order], dtype=np.float64).reshape(n, 4)
    difficult = np.array([1 if objects[j][2] else 0 for j in order], dtype=np.uint8).reshape(n)
    off = np.zeros(I * K + 1, dtype=np.int32)
    np.cumsum(np.bincount(cell, minlength=I * K), out=off[1:])
    return {"image_ids": list(image_ids), "class_names": list(class_names), "boxes": boxes, "difficult": difficult, "off": off,
            "image": (cell[order] // K).astype(np.int32), "classes": (cell[order] % K).astype(np.int32)}


def parse_voc_ground_truth(dirname, split, class_names):
    """Annotations/<id>.xml of the ids in ImageSets/Main/<split>.txt -> `prepare_voc_ground_truth` arrays; objects of a class
    that is not in `class_names` take no part, as in the reference, which selects by name"""
    class_names = list(class_names)
    index = {n: k for k, n in enumerate(class_names)}
    ids = read_voc_ids(dirname, split)
    objects = []
    for i, fileid in enumerate(ids):
        for name, difficult, box in read_voc_objects(os.path.join(dirname, "Annotations", fileid + ".xml"))[2]:
            if name in index:
                objects.append((i, index[name], difficult, box))
    return prepare_voc_ground_truth(ids, class_names, objects)


def status_message(status):
    return "; ".join(text for bit, text in STATUS_CAUSES if status & bit)


def _ptr(t):
    return C.c_void_p(t.data_ptr() if t is not None else None)


class VOCevalHIP:
    """gt: `parse_voc_ground_truth(...)`.  Detections, concatenated over the dataset, as DEVICE tensors: boxes f32 [N,4] XYXY
    (0-based, as the model gives them), scores f32 [N], classes i32 [N] in [0,K), image i32 [N] (index into gt["image_ids"]).

    evaluate(thresholds, year) -> AP table f64 [K, T] (fractions): the 11-point form for 2007, the area form for 2012.  Both
    tables stay in `ap07` / `ap12`; with keep_pr=True `rec` / `prec` [T, N] (by position of the total order `order`) too."""

    def __init__(self, gt, boxes, scores, classes, image):
        for name, t in (("boxes", boxes), ("scores", scores), ("classes", classes), ("image", image)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise NotImplementedError(f"VOCevalHIP: `{name}` must be a tensor on the GPU; scoring runs in HIP kernels and "
                                          "there is no CPU fallback")
        self._gt = gt
        self._dt = (boxes.detach().float().reshape(-1, 4).contiguous(), scores.detach().float().contiguous(),
                    classes.detach().to(torch.int32).contiguous(), image.detach().to(torch.int32).contiguous())
        self.ap07 = self.ap12 = self.rec = self.prec = self.order = self.cls_off = self.npos = self.flags = None
        self.status = 0

    def evaluate(self, thresholds, year, keep_pr=False):
        assert year in (2007, 2012), year
        gt = self._gt
        boxes, scores, classes, image = self._dt
        dev = boxes.device
        thresholds = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
        I, K, T = len(gt["image_ids"]), len(gt["class_names"]), int(thresholds.size)
        N, NG = int(scores.numel()), int(gt["difficult"].size)
        lib = _lib.voceval_lib()
        nbytes = lib.ctdet_voceval_workspace_bytes(N, NG, I, K, T)
        if nbytes == 0:
            raise ValueError(f"voceval: {_lib.lib().ctdet_last_error().decode()}")
        f64 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(dev)     # noqa: E731
        gt_boxes, gt_diff = f64(gt["boxes"]), torch.as_tensor(gt["difficult"]).to(dev)
        gt_off, thrs, points = torch.as_tensor(gt["off"]).to(dev), f64(thresholds), f64(RECALL_POINTS_07)
        ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
        ws_ptr = C.c_void_p((ws.data_ptr() + 255) & ~255)
        order = torch.empty(N, dtype=torch.int32, device=dev)
        cls_off = torch.empty(K + 1, dtype=torch.int32, device=dev)
        flags = torch.empty((N, T), dtype=torch.uint8, device=dev)
        npos = torch.empty(K, dtype=torch.int32, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        ap07 = torch.empty((K, T), dtype=torch.float64, device=dev)
        ap12 = torch.empty((K, T), dtype=torch.float64, device=dev)
        rec = torch.empty((T, N), dtype=torch.float64, device=dev) if keep_pr else None
        prec = torch.empty((T, N), dtype=torch.float64, device=dev) if keep_pr else None
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        with torch.cuda.device(dev):
            _lib.check(lib.ctdet_voceval_match(
                _ptr(boxes), _ptr(scores), _ptr(classes), _ptr(image), N, _ptr(gt_boxes), _ptr(gt_diff), _ptr(gt_off), NG, I, K,
                _ptr(thrs), T, ws_ptr, _ptr(order), _ptr(cls_off), _ptr(flags), _ptr(npos), _ptr(status), stream),
                "ctdet_voceval_match")
            _lib.check(lib.ctdet_voceval_ap(
                _ptr(order), _ptr(cls_off), _ptr(flags), _ptr(npos), N, K, T, _ptr(points), ws_ptr, _ptr(ap07), _ptr(ap12),
                _ptr(rec), _ptr(prec), stream), "ctdet_voceval_ap")
        # the one synchronisation of the scorer: the status word and the two [K, T] tables
        self.status = int(status.item())
        if self.status:
            raise ValueError("VOCevalHIP: the detections hold " + status_message(self.status))
        self.ap07, self.ap12 = ap07.cpu().numpy(), ap12.cpu().numpy()
        self.order, self.cls_off, self.npos, self.flags, self.rec, self.prec = order, cls_off, npos, flags, rec, prec
        return self.ap07 if year == 2007 else self.ap12
