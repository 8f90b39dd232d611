"""LVIS box-AP scoring on the device: `LVISevalHIP` drives the two entry points of libctdet_lviseval.so
(ctdet_lviseval_match / ctdet_lviseval_accumulate, csrc/lviseval.hip) over the detections of a whole dataset, the role the
`lvis` package's `LVISEval` has in the reference (detectron2/evaluation/lvis_evaluation.py).  The rule is restated from LVIS's
published evaluation procedure in DESIGN.md 7.17; parity with the package is not pinned.  "bbox" only; there is no CPU
fallback: detections on the CPU are refused by name."""
import numpy as np
import torch

from .. import _lib
from .box_scoring import DeviceScorer, cells_csr, ptr as _ptr

LIST_NEG, LIST_NEL = 1, 2          # CTDET_LVIS_NEG / CTDET_LVIS_NEL

IOU_THRS = np.linspace(0.5, 0.95, 10)
REC_THRS = np.linspace(0.0, 1.0, 101)
AREA_RNGS = ((0.0, 1e10), (0.0, 1024.0), (1024.0, 9216.0), (9216.0, 1e10))
AREA_LABELS = ("all", "small", "medium", "large")
MAX_DETS = 300


def prepare_lvis_ground_truth(dataset):
    """LVIS json dict -> the arrays the matcher takes.  Images / categories: all ids of the set, sorted.  Ground truth is
    stable-sorted by (image, category) with CSR offsets [I*K+1]; boxes XYWH as written; `area` is the annotation's field (the
    segment's area in LVIS), else w * h; `ignore` is the field, else 0.  `lists` u8 [I, K]: bit 1 = the category is in the
    image's `neg_category_ids`, bit 2 = in its `not_exhaustive_category_ids`.  `frequency`: "r" / "c" / "f" per category ("" where
    the json has none)."""
    images = sorted(dataset["images"], key=lambda im: im["id"])
    cats = sorted(dataset.get("categories", []), key=lambda c: c["id"])
    image_ids, cat_ids = [im["id"] for im in images], [c["id"] for c in cats]
    if len(set(image_ids)) != len(image_ids) or len(set(cat_ids)) != len(cat_ids):
        raise ValueError("prepare_lvis_ground_truth: image or category ids are not unique")
    img_index, cat_index = {v: i for i, v in enumerate(image_ids)}, {v: i for i, v in enumerate(cat_ids)}
    anns = dataset.get("annotations", [])
    I, K, n = len(image_ids), len(cat_ids), len(anns)
    cell = np.array([img_index[a["image_id"]] * K + cat_index[a["category_id"]] for a in anns], dtype=np.int64).reshape(n)
    order, off, image, classes = cells_csr(cell, I, K)
    boxes = np.array([anns[j]["bbox"] for j in order], dtype=np.float64).reshape(n, 4)
    area = np.array([anns[j]["area"] if "area" in anns[j] else anns[j]["bbox"][2] * anns[j]["bbox"][3] for j in order],
                    dtype=np.float64).reshape(n)
    ignore = np.array([1 if anns[j].get("ignore", 0) else 0 for j in order], dtype=np.uint8).reshape(n)
    lists = np.zeros((I, K), dtype=np.uint8)
    for i, im in enumerate(images):
        for field, bit in (("neg_category_ids", LIST_NEG), ("not_exhaustive_category_ids", LIST_NEL)):
            for c in im.get(field, []):
                lists[i, cat_index[c]] |= bit
    return {"image_ids": image_ids, "cat_ids": cat_ids, "boxes": boxes, "area": area, "ignore": ignore, "off": off,
            "image": image, "classes": classes, "lists": lists, "frequency": [c.get("frequency", "") for c in cats]}


def summarize_lvis(precision, recall, frequency):
    """precision [T,R,K,A] and recall [T,K,A] with the ten thresholds and the four area ranges of LVIS -> the nine AP figures
    and the four AR@300 (fractions): means over the entries > -1, -1 where there is none"""
    def mean(s):
        return float(np.mean(s[s > -1])) if (s > -1).any() else -1.0
    t50, t75 = int(np.argmin(np.abs(IOU_THRS - 0.5))), int(np.argmin(np.abs(IOU_THRS - 0.75)))
    res = {"AP": mean(precision[:, :, :, 0]), "AP50": mean(precision[t50, :, :, 0]), "AP75": mean(precision[t75, :, :, 0]),
           "APs": mean(precision[:, :, :, 1]), "APm": mean(precision[:, :, :, 2]), "APl": mean(precision[:, :, :, 3])}
    for f in "rcf":
        sel = [k for k, v in enumerate(frequency) if v == f]
        res["AP" + f] = mean(precision[:, :, sel, 0])
    for a, lbl in enumerate(("", "s", "m", "l")):
        res[f"AR{lbl}@{MAX_DETS}"] = mean(recall[:, :, a])
    return res


class LVISevalHIP(DeviceScorer):
    """gt: `prepare_lvis_ground_truth(...)`.  Detections, concatenated over the dataset, as DEVICE tensors: boxes f32 [N,4]
    XYXY, scores f32 [N], classes i32 [N] (index into the sorted category ids), image i32 [N] (index into the sorted image ids).

    evaluate() -> {AP, AP50, AP75, APs, APm, APl, APr, APc, APf} as fractions (-1: nothing to average); `precision` [T,R,K,A]
    and `recall` [T,K,A] stay on the object, as do `ar` = {AR@300, ARs@300, ARm@300, ARl@300}.  The parameters (`iou_thrs`,
    `rec_thrs`, `area_rngs`, `max_dets`) are settable before evaluate(); the summary needs LVIS's own ten and four."""

    def __init__(self, gt, boxes, scores, classes, image):
        super().__init__(gt, boxes, scores, classes, image)
        self.iou_thrs, self.rec_thrs, self.area_rngs, self.max_dets = IOU_THRS, REC_THRS, AREA_RNGS, MAX_DETS
        self.precision = self.recall = self.results = self.ar = self.order = self.cls_off = self.flags = self.npig = None
        self.status = 0

    def score(self):
        """the two calls and the one synchronisation: precision [T,R,K,A], recall [T,K,A] as numpy arrays"""
        gt, dev, up = self._gt, self._device, self._up
        boxes, scores, classes, image = self._dt
        iou_thrs = np.ascontiguousarray(self.iou_thrs, dtype=np.float64).reshape(-1)
        rec_thrs = np.ascontiguousarray(self.rec_thrs, dtype=np.float64).reshape(-1)
        area_rngs = np.ascontiguousarray(self.area_rngs, dtype=np.float64).reshape(-1, 2)
        I, K, T, R, A = len(gt["image_ids"]), len(gt["cat_ids"]), int(iou_thrs.size), int(rec_thrs.size), int(area_rngs.shape[0])
        N, NG = int(scores.numel()), int(gt["area"].size)
        lib = _lib.lviseval_lib()
        ws, ws_ptr = self._workspace(lib.ctdet_lviseval_workspace_bytes(N, NG, I, K, A, T),
                                     lambda text: ValueError(f"lviseval: {text}"))
        gt_boxes, gt_area, gt_ignore, gt_off = up(gt["boxes"], True), up(gt["area"], True), up(gt["ignore"]), up(gt["off"])
        lists = up(np.ascontiguousarray(gt["lists"], dtype=np.uint8).reshape(I, K))
        thrs, rngs, recs = up(iou_thrs, True), up(area_rngs, True), up(rec_thrs, True)
        order, cls_off, flags, status = self._outputs(N, K, A * T)
        npig = torch.empty((K, A), dtype=torch.int32, device=dev)
        precision = torch.empty((T, R, K, A), dtype=torch.float64, device=dev)
        recall = torch.empty((T, K, A), dtype=torch.float64, device=dev)
        self._call(lib.ctdet_lviseval_match,
                   _ptr(boxes), _ptr(scores), _ptr(classes), _ptr(image), N, _ptr(gt_boxes), _ptr(gt_area), _ptr(gt_ignore),
                   _ptr(gt_off), NG, _ptr(lists), I, K, _ptr(thrs), T, _ptr(rngs), A, int(self.max_dets), ws_ptr, _ptr(order),
                   _ptr(cls_off), _ptr(flags), _ptr(npig), _ptr(status))
        self._call(lib.ctdet_lviseval_accumulate,
                   _ptr(order), _ptr(cls_off), _ptr(flags), _ptr(npig), N, K, A, T, _ptr(recs), R, _ptr(precision), _ptr(recall))
        self._check_status(status)     # the one synchronisation of the scorer: the status word and the two tables
        self.precision, self.recall = precision.cpu().numpy(), recall.cpu().numpy()
        self.order, self.cls_off, self.flags, self.npig = order, cls_off, flags, npig
        return self.precision, self.recall

    def evaluate(self):
        precision, recall = self.score()
        res = summarize_lvis(precision, recall, self._gt["frequency"])
        self.ar = {k: v for k, v in res.items() if k.startswith("AR")}
        self.results = {k: v for k, v in res.items() if not k.startswith("AR")}
        return self.results


status_message = LVISevalHIP.status_message     # the causes in a status word of ctdet_lviseval_match (CTDET_LVIS_BAD_*)
