"""`PascalVOCDetectionEvaluator` with the reference's protocol (detectron2/evaluation/pascal_voc_evaluation.py:20-114): the
VOC2007 (11-point) or VOC2012 (area) box AP of a `voc_*` dataset at the ten thresholds 0.50 ... 0.95, scored by the HIP
matcher and AP kernels (`VOCevalHIP`) where the reference writes a text file per class and runs `voc_eval` per (class,
threshold).  `process()` keeps the device tensors of the `Instances`; nothing is copied to the host per image.  `evaluate()`
gathers every rank's arrays on the main process, scores them on that process's device and returns

    {"bbox": {AP, AP50, AP75}, "bbox_AP": {class: AP}, "bbox_AP50": {class: AP50}, "bbox_AP75": {class: AP75}}

with every AP multiplied by 100 and the means taken with numpy on the host, as the reference does."""
import logging
from collections import OrderedDict

import numpy as np

from ..data.catalog import MetadataCatalog
from .box_scoring import BoxEvaluator
from .coco_evaluation import gather_detections
from .voceval import VOCevalHIP, parse_voc_ground_truth

# the reference's `range(50, 100, 5)`, each divided by 100.0
VOC_THRESHOLDS = tuple(range(50, 100, 5))


def derive_voc_results(ap_table, class_names):
    """AP table [K, 10] (fractions, thresholds 0.50 ... 0.95) -> the result dict; the same numpy reductions over the same
    [threshold, class] layout as the reference's, so that the figures agree to the bit"""
    scaled = np.ascontiguousarray(np.asarray(ap_table, dtype=np.float64).T * 100)        # [T, K]
    per_threshold = [np.mean(row) for row in scaled]
    per_class = np.mean(scaled, axis=0)
    t50, t75 = VOC_THRESHOLDS.index(50), VOC_THRESHOLDS.index(75)
    names = list(class_names)
    return OrderedDict([
        ("bbox", {"AP": np.mean(per_threshold), "AP50": per_threshold[t50], "AP75": per_threshold[t75]}),
        ("bbox_AP", dict(zip(names, per_class))),
        ("bbox_AP50", dict(zip(names, scaled[t50]))),
        ("bbox_AP75", dict(zip(names, scaled[t75])))])


class PascalVOCDetectionEvaluator(BoxEvaluator):
    def __init__(self, dataset_name, distributed=True):
        self._dataset_name, self._distributed = dataset_name, distributed
        meta = MetadataCatalog.get(dataset_name)
        for field in ("dirname", "split", "year", "thing_classes"):
            if not hasattr(meta, field):
                raise ValueError(f"PascalVOCDetectionEvaluator: dataset '{dataset_name}' has no `{field}` in its metadata; "
                                 "register it with register_pascal_voc")
        assert meta.year in (2007, 2012), meta.year
        self._year, self._class_names = meta.year, list(meta.thing_classes)
        self._dirname, self._split = meta.dirname, meta.split
        self._gt = None      # read on the first evaluate(): only the main process needs it
        self._logger = logging.getLogger(__name__)
        self.reset()

    def evaluate(self):
        merged = gather_detections(self._local(), self._distributed)
        if merged is None:
            return None
        ids, counts, boxes, scores, classes = merged
        self._logger.info("Evaluating {} using {} metric. Note that results do not use the official Matlab API.".format(
            self._dataset_name, self._year))
        K, T = len(self._class_names), len(VOC_THRESHOLDS)
        if sum(counts) == 0:      # every class file of the reference is empty: each AP is 0
            return derive_voc_results(np.zeros((K, T)), self._class_names)
        if self._gt is None:
            self._gt = parse_voc_ground_truth(self._dirname, self._split, self._class_names)
        boxes, scores, classes = self._checked(ids, boxes, scores, classes, f"ImageSets/Main/{self._split}.txt")
        image = self._image_of(ids, counts, boxes.device)
        self.voc_eval = ev = VOCevalHIP(self._gt, boxes, scores, classes, image)
        # a class outside thing_classes or a non-finite score or box is the scorer's ValueError, which names the cause
        table = ev.evaluate([t / 100.0 for t in VOC_THRESHOLDS], self._year)
        return derive_voc_results(table, self._class_names)
