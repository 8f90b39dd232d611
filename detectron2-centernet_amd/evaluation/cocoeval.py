"""COCO box-AP scoring on the device: `COCOevalHIP` holds the `Params` of COCO and drives the two entry points of the shared
library (ctdet_cocoeval_match / ctdet_cocoeval_accumulate, csrc/cocoeval.hip) the way the reference's `COCOeval_opt`
(detectron2/evaluation/fast_eval_api.py) drives `detectron2._C.COCOevalEvaluateImages` / `COCOevalAccumulate`.  The result is
pinned to that native scorer (precision = tp / (tp + fp); DESIGN.md 7.7 holds the definition).  "bbox" with useCats = 1 only;
there is no CPU fallback: detections on the CPU are refused by name."""
from collections import OrderedDict

import numpy as np
import torch

from .. import _lib
from .box_scoring import DeviceScorer, cells_csr, ptr as _ptr


class Params:
    """pycocotools.cocoeval.Params for iouType "bbox"; every field is settable"""

    def __init__(self, iouType="bbox"):
        if iouType != "bbox":
            raise NotImplementedError(f"COCOevalHIP scores iouType 'bbox' only, not '{iouType}' (segm / keypoints are not built)")
        self.iouType = iouType
        self.imgIds, self.catIds = [], []
        self.iouThrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
        self.recThrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
        self.maxDets = [1, 10, 100]
        self.areaRng = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
        self.areaRngLbl = ["all", "small", "medium", "large"]
        self.useCats = 1


def prepare_ground_truth(image_ids, cat_ids, annotations):
    """COCO annotation dicts -> the arrays the matcher takes.  Images / categories: all ids of the set, sorted.  Ground truth is
    stable-sorted by (image, category) with CSR offsets [I*K+1]; ignore = iscrowd; `area` is the annotation's field."""
    image_ids, cat_ids = sorted(set(image_ids)), sorted(set(cat_ids))
    img_index, cat_index = {v: i for i, v in enumerate(image_ids)}, {v: i for i, v in enumerate(cat_ids)}
    I, K, n = len(image_ids), len(cat_ids), len(annotations)
    cell = np.array([img_index[a["image_id"]] * K + cat_index[a["category_id"]] for a in annotations], dtype=np.int64)
    order, off, image, classes = cells_csr(cell, I, K)
    boxes = np.array([annotations[j]["bbox"] for j in order], dtype=np.float64).reshape(n, 4)
    area = np.array([annotations[j]["area"] for j in order], dtype=np.float64)
    crowd = np.array([int(annotations[j].get("iscrowd", 0)) for j in order], dtype=np.uint8)
    return {"image_ids": image_ids, "cat_ids": cat_ids, "boxes": boxes, "area": area, "crowd": crowd, "off": off,
            "image": image, "classes": classes}


def summarize_stats(precision, recall, params):
    """the twelve `stats` of COCO (pycocotools.cocoeval.COCOeval.summarize, iouType bbox): mean over entries > -1, or -1"""
    iou_thrs, max_dets, labels = np.asarray(params.iouThrs), list(params.maxDets), list(params.areaRngLbl)

    def one(ap, iouThr=None, areaRng="all", maxDets=100):
        a, m = labels.index(areaRng), max_dets.index(maxDets)
        s = precision if ap else recall
        if iouThr is not None:
            s = s[np.where(iouThr == iou_thrs)[0]]
        s = s[:, :, :, a, m] if ap else s[:, :, a, m]
        return float(np.mean(s[s > -1])) if (s > -1).any() else -1.0

    md = max_dets
    return np.array([one(1, maxDets=md[2]), one(1, .5, maxDets=md[2]), one(1, .75, maxDets=md[2]),
                     one(1, areaRng="small", maxDets=md[2]), one(1, areaRng="medium", maxDets=md[2]),
                     one(1, areaRng="large", maxDets=md[2]), one(0, maxDets=md[0]), one(0, maxDets=md[1]), one(0, maxDets=md[2]),
                     one(0, areaRng="small", maxDets=md[2]), one(0, areaRng="medium", maxDets=md[2]),
                     one(0, areaRng="large", maxDets=md[2])])


class COCOevalHIP(DeviceScorer):
    """evaluate() / accumulate() / summarize() with `eval` = {"params", "counts", "precision", "recall", "scores"} and `stats`
    shaped as the reference's COCOeval_opt leaves them.

    gt: `prepare_ground_truth(...)`.  Detections, concatenated over the dataset, as DEVICE tensors: boxes f32 [N,4] XYXY,
    scores f32 [N], classes i32 [N] (index into the sorted category ids), image i32 [N] (index into the sorted image ids)."""

    def __init__(self, gt, boxes, scores, classes, image, iouType="bbox"):
        self.params = Params(iouType)
        self.params.imgIds, self.params.catIds = list(gt["image_ids"]), list(gt["cat_ids"])
        super().__init__(gt, boxes, scores, classes, image)
        self.eval, self.stats, self._dev = {}, None, None

    # ---- device side
    def _upload(self):
        p, gt, dev = self.params, self._gt, self._device
        if int(p.useCats) != 1:
            raise NotImplementedError("COCOevalHIP: useCats = 0 is not built")
        T, A, R, M = len(p.iouThrs), len(p.areaRng), len(p.recThrs), len(p.maxDets)
        I, K, N, NG = len(p.imgIds), len(p.catIds), int(self._dt[1].numel()), int(len(gt["area"]))
        if list(p.maxDets) != sorted(p.maxDets):
            raise ValueError("COCOevalHIP: maxDets must be ascending")
        up = self._up
        d = {"T": T, "A": A, "R": R, "M": M, "I": I, "K": K, "N": N, "NG": NG, "max_det": int(p.maxDets[-1]),
             "gt_boxes": up(gt["boxes"], True), "gt_area": up(gt["area"], True), "gt_crowd": up(gt["crowd"]),
             "gt_off": up(gt["off"]), "iou_thrs": up(p.iouThrs, True), "area_rngs": up(p.areaRng, True),
             "rec_thrs": up(p.recThrs, True), "max_dets": torch.tensor(list(p.maxDets), dtype=torch.int32, device=dev)}
        d["ws"], d["ws_ptr"] = self._workspace(_lib.lib().ctdet_cocoeval_workspace_bytes(N, NG, I, K, A, T),
                                               lambda text: RuntimeError(f"cocoeval: {text}"))
        d["order"] = torch.empty(N, dtype=torch.int32, device=dev)
        d["rank"] = torch.empty(N, dtype=torch.int32, device=dev)
        d["flags"] = torch.empty(N * A * T, dtype=torch.uint8, device=dev)
        d["npig"] = torch.empty(K * A, dtype=torch.int32, device=dev)
        d["status"] = torch.empty(1, dtype=torch.int32, device=dev)
        d["precision"] = torch.empty((T, R, K, A, M), dtype=torch.float64, device=dev)
        d["scores"] = torch.empty((T, R, K, A, M), dtype=torch.float64, device=dev)
        d["recall"] = torch.empty((T, K, A, M), dtype=torch.float64, device=dev)
        self._dev = d

    def _match(self):
        d = self._dev
        boxes, scores, classes, image = self._dt
        self._call(_lib.lib().ctdet_cocoeval_match,
                   _ptr(boxes), _ptr(scores), _ptr(classes), _ptr(image), d["N"], _ptr(d["gt_boxes"]), _ptr(d["gt_area"]),
                   _ptr(d["gt_crowd"]), _ptr(d["gt_off"]), d["NG"], d["I"], d["K"], _ptr(d["iou_thrs"]), d["T"],
                   _ptr(d["area_rngs"]), d["A"], d["max_det"], d["ws_ptr"], _ptr(d["order"]), _ptr(d["rank"]),
                   _ptr(d["flags"]), _ptr(d["npig"]), _ptr(d["status"]))

    def _accumulate(self):
        d = self._dev
        scores, classes = self._dt[1:3]
        self._call(_lib.lib().ctdet_cocoeval_accumulate,
                   _ptr(scores), _ptr(classes), _ptr(d["order"]), _ptr(d["rank"]), _ptr(d["flags"]), _ptr(d["npig"]), d["N"],
                   d["K"], d["A"], d["T"], _ptr(d["rec_thrs"]), d["R"], _ptr(d["max_dets"]), d["M"], d["max_det"], d["ws_ptr"],
                   _ptr(d["precision"]), _ptr(d["scores"]), _ptr(d["recall"]))

    # ---- the COCOeval protocol
    def evaluate(self):
        """upload the ground truth and the parameters, order the detections and match them (no synchronisation)"""
        self._upload()
        self._match()

    def accumulate(self):
        """precision / recall / scores; the one synchronisation of the scorer is the copy of the result arrays"""
        if self._dev is None:
            raise RuntimeError("Please run evaluate() first")
        self._accumulate()
        d, p = self._dev, self.params
        if int(d["status"].item()) != 0:
            raise ValueError("COCOevalHIP: a detection's image or category index is outside the ground-truth set")
        self.eval = {"params": p, "counts": [d["T"], d["R"], d["K"], d["A"], d["M"]],
                     "precision": d["precision"].cpu().numpy(), "recall": d["recall"].cpu().numpy(),
                     "scores": d["scores"].cpu().numpy()}

    def summarize(self):
        if not self.eval:
            raise RuntimeError("Please run accumulate() first")
        self.stats = summarize_stats(self.eval["precision"], self.eval["recall"], self.params)
        return self.stats


def derive_coco_results(stats, precision, class_names=None):
    """`COCOEvaluator._derive_coco_results` for "bbox" (coco_evaluation.py:252-318): the six AP figures x100 (`nan` for -1)
    and, with more than one class, `AP-<class name>` from precision[:, :, k, 0, -1]; `stats` None = no predictions"""
    metrics = ["AP", "AP50", "AP75", "APs", "APm", "APl"]
    if stats is None:
        return OrderedDict((m, float("nan")) for m in metrics)
    res = OrderedDict((m, float(stats[i] * 100 if stats[i] >= 0 else "nan")) for i, m in enumerate(metrics))
    if class_names is None or len(class_names) <= 1:
        return res
    assert len(class_names) == precision.shape[2], (len(class_names), precision.shape)
    for k, name in enumerate(class_names):
        pr = precision[:, :, k, 0, -1]
        pr = pr[pr > -1]
        res["AP-" + "{}".format(name)] = float(np.mean(pr) * 100) if pr.size else float("nan")
    return res
