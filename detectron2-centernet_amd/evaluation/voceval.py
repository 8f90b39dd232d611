"""Pascal VOC box-AP scoring on the device: `VOCevalHIP` drives the two entry points of libctdet_voceval.so
(ctdet_voceval_match / ctdet_voceval_ap, csrc/voceval.hip) over the detections of a whole dataset, the role `voc_eval` has
in the reference (detectron2/evaluation/pascal_voc_evaluation.py) -- once for every class and threshold instead of once per
(class, threshold).  DESIGN.md 7.16 holds the rule.  There is no CPU fallback: detections on the CPU are refused by name."""
import os

import numpy as np
import torch

from .. import _lib
from ..data.pascal_voc import read_voc_ids, read_voc_objects
from .box_scoring import DeviceScorer, cells_csr, ptr as _ptr

# the reference's `np.arange(0.0, 1.1, 0.1)`: the recall points of the 11-point form, as numpy rounds them
RECALL_POINTS_07 = np.arange(0.0, 1.1, 0.1)


def prepare_voc_ground_truth(image_ids, class_names, objects):
    """objects: (image index, class index, difficult, [xmin, ymin, xmax, ymax]) in file order -> the arrays the matcher takes:
    stable-sorted by (image, class) cell with CSR offsets [I*K+1]; boxes f64 as written (1-based)"""
    I, K, n = len(image_ids), len(class_names), len(objects)
    cell = np.array([o[0] * K + o[1] for o in objects], dtype=np.int64).reshape(n)
    order, off, image, classes = cells_csr(cell, I, K)
    boxes = np.array([objects[j][3] for j in order], dtype=np.float64).reshape(n, 4)
    difficult = np.array([1 if objects[j][2] else 0 for j in order], dtype=np.uint8).reshape(n)
    return {"image_ids": list(image_ids), "class_names": list(class_names), "boxes": boxes, "difficult": difficult, "off": off,
            "image": image, "classes": classes}


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


class VOCevalHIP(DeviceScorer):
    """gt: `parse_voc_ground_truth(...)`.  Detections, concatenated over the dataset, as DEVICE tensors: boxes f32 [N,4] XYXY
    (0-based, as the model gives them), scores f32 [N], classes i32 [N] in [0,K), image i32 [N] (index into gt["image_ids"]).

    evaluate(thresholds, year) -> AP table f64 [K, T] (fractions): the 11-point form for 2007, the area form for 2012.  Both
    tables stay in `ap07` / `ap12`; with keep_pr=True `rec` / `prec` [T, N] (by position of the total order `order`) too."""

    IMAGE_LIST = "the split's image list"

    def __init__(self, gt, boxes, scores, classes, image):
        super().__init__(gt, boxes, scores, classes, image)
        self.ap07 = self.ap12 = self.rec = self.prec = self.order = self.cls_off = self.npos = self.flags = None
        self.status = 0

    def evaluate(self, thresholds, year, keep_pr=False):
        assert year in (2007, 2012), year
        gt, dev, up = self._gt, self._device, self._up
        boxes, scores, classes, image = self._dt
        thresholds = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
        I, K, T = len(gt["image_ids"]), len(gt["class_names"]), int(thresholds.size)
        N, NG = int(scores.numel()), int(gt["difficult"].size)
        lib = _lib.voceval_lib()
        ws, ws_ptr = self._workspace(lib.ctdet_voceval_workspace_bytes(N, NG, I, K, T), lambda text: ValueError(f"voceval: {text}"))
        gt_boxes, gt_diff, gt_off = up(gt["boxes"], True), up(gt["difficult"]), up(gt["off"])
        thrs, points = up(thresholds, True), up(RECALL_POINTS_07, True)
        order, cls_off, flags, status = self._outputs(N, K, T)
        npos = torch.empty(K, dtype=torch.int32, device=dev)
        ap07 = torch.empty((K, T), dtype=torch.float64, device=dev)
        ap12 = torch.empty((K, T), dtype=torch.float64, device=dev)
        rec = torch.empty((T, N), dtype=torch.float64, device=dev) if keep_pr else None
        prec = torch.empty((T, N), dtype=torch.float64, device=dev) if keep_pr else None
        self._call(lib.ctdet_voceval_match,
                   _ptr(boxes), _ptr(scores), _ptr(classes), _ptr(image), N, _ptr(gt_boxes), _ptr(gt_diff), _ptr(gt_off), NG, I, K,
                   _ptr(thrs), T, ws_ptr, _ptr(order), _ptr(cls_off), _ptr(flags), _ptr(npos), _ptr(status))
        self._call(lib.ctdet_voceval_ap,
                   _ptr(order), _ptr(cls_off), _ptr(flags), _ptr(npos), N, K, T, _ptr(points), ws_ptr, _ptr(ap07), _ptr(ap12),
                   _ptr(rec), _ptr(prec))
        self._check_status(status)     # the one synchronisation of the scorer: the status word and the two [K, T] tables
        self.ap07, self.ap12 = ap07.cpu().numpy(), ap12.cpu().numpy()
        self.order, self.cls_off, self.npos, self.flags, self.rec, self.prec = order, cls_off, npos, flags, rec, prec
        return self.ap07 if year == 2007 else self.ap12


status_message = VOCevalHIP.status_message     # the causes in a status word of ctdet_voceval_match (CTDET_VOC_BAD_*)
