"""`LVISEvaluator` with the reference's protocol (detectron2/evaluation/lvis_evaluation.py:21-155), "bbox" task: the LVIS box
AP of an `lvis_*` dataset scored by the HIP matcher and PR kernels (`LVISevalHIP`), the role the `lvis` package's `LVISEval`
has in the reference.  `process()` keeps the device tensors of the `Instances`; nothing is copied to the host per image.
`evaluate()` gathers every rank's arrays on the main process, scores them on that process's device and returns
OrderedDict(bbox={AP, AP50, AP75, APs, APm, APl, APr, APc, APf}), every figure multiplied by 100.

Not built, refused by name: the "segm" task, box proposals, `instances_predictions.pth`, CPU tensors."""
import copy
import json
import logging
import os
from collections import OrderedDict

import torch

from ..data.catalog import MetadataCatalog
from .box_scoring import BoxEvaluator
from .coco_evaluation import create_small_table, gather_detections
from .coco_results import coco_records
from .lviseval import LVISevalHIP, prepare_lvis_ground_truth

METRICS = ("AP", "AP50", "AP75", "APs", "APm", "APl", "APr", "APc", "APf")


class LVISEvaluator(BoxEvaluator):
    def __init__(self, dataset_name, cfg, distributed, output_dir=None):
        self._logger = logging.getLogger(__name__)
        if cfg is not None and cfg.MODEL.get("MASK_ON", False):
            raise NotImplementedError("LVISEvaluator: task 'segm' is not built; only 'bbox' is scored")
        self._distributed, self._output_dir = distributed, output_dir
        self._metadata = MetadataCatalog.get(dataset_name)
        if not hasattr(self._metadata, "json_file"):
            raise ValueError(f"LVISEvaluator: dataset '{dataset_name}' has no `json_file` in its metadata; register it with "
                             "register_lvis_instances")
        with open(self._metadata.json_file) as f:
            dataset = json.load(f)
        self._gt = prepare_lvis_ground_truth(dataset)
        # test-set json files hold no annotations: the results file is all there is to do
        self._do_evaluation = len(dataset.get("annotations", [])) > 0
        self.reset()

    def _instances(self, out):
        if "proposals" in out:
            raise NotImplementedError("LVISEvaluator: box proposals ('proposals' outputs) are not scored")
        return out.get("instances")

    def _category_ids(self):
        """dataset category id of every class index of the model: through the metadata's mapping where it has one (the
        cocofied sets), else class index + 1"""
        if hasattr(self._metadata, "thing_dataset_id_to_contiguous_id"):
            rev = {v: k for k, v in self._metadata.thing_dataset_id_to_contiguous_id.items()}
            if sorted(rev) != list(range(len(rev))):
                raise ValueError("LVISEvaluator: `thing_dataset_id_to_contiguous_id` does not map onto 0 .. K-1")
            return [rev[c] for c in range(len(rev))]
        names = self._metadata.get("thing_classes")
        return [c + 1 for c in range(len(names) if names else len(self._gt["cat_ids"]))]

    def evaluate(self):
        merged = gather_detections(self._local(), self._distributed)
        if merged is None:
            return {}
        ids, counts, boxes, scores, classes = merged
        if len(ids) == 0:
            self._logger.warning("[LVISEvaluator] Did not receive valid predictions.")
            return {}
        boxes, scores, classes = self._checked(ids, boxes, scores, classes, "the ground-truth set")
        self._results = OrderedDict()
        self._eval_predictions(ids, counts, boxes, scores, classes)
        return copy.deepcopy(self._results)

    def _eval_predictions(self, ids, counts, boxes, scores, classes):
        dev = boxes.device
        cat_ids = self._category_ids()
        if self._output_dir:
            os.makedirs(self._output_dir, exist_ok=True)
            path = os.path.join(self._output_dir, "lvis_instances_results.json")
            self._logger.info("Saving results to {}".format(path))
            per_det_ids = [i for i, c in zip(ids, counts) for _ in range(c)]
            with open(path, "w") as f:
                f.write(json.dumps(coco_records(boxes, scores, classes, per_det_ids, dict(enumerate(cat_ids)))))
        if not self._do_evaluation:
            self._logger.info("Annotations are not available for evaluation.")
            return
        self._logger.info("Evaluating predictions with the HIP LVIS scorer...")
        if int(scores.numel()) > 0:
            image = self._image_of(ids, counts, dev)
            cat_index = {c: i for i, c in enumerate(self._gt["cat_ids"])}
            lut = torch.tensor([cat_index.get(c, -1) for c in cat_ids] + [-1], dtype=torch.int32, device=dev)
            n = len(cat_ids)
            cls = lut[classes.long().clamp(min=-1, max=n - 1)]
            cls = torch.where((classes < 0) | (classes >= n), torch.full_like(cls, -1), cls)     # out of range: the scorer reports it
            self.lvis_eval = ev = LVISevalHIP(self._gt, boxes, scores, cls, image)
            res = ev.evaluate()
            res = OrderedDict((m, float(res[m] * 100) if res[m] >= 0 else float("nan")) for m in METRICS)
        else:
            self._logger.warning("No predictions from the model!")
            res = OrderedDict((m, float("nan")) for m in METRICS)
        self._logger.info("Evaluation results for bbox: \n" + create_small_table(res))
        self._results["bbox"] = res
