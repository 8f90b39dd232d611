"""`COCOEvaluator` with the reference's protocol (detectron2/evaluation/coco_evaluation.py:29-318), "bbox" task: box AP of a
dataset scored by the HIP matcher and PR kernels (`COCOevalHIP`), the role pycocotools / `COCOeval_opt` have in the
reference.  `process()` keeps the device tensors of the `Instances`; nothing is copied to the host per image.  `evaluate()`
gathers every rank's arrays on the main process, scores them on that process's device and returns
OrderedDict(bbox={AP, AP50, AP75, APs, APm, APl[, AP-<class>]}).

Not built, refused by name: the "segm" and "keypoints" tasks, box proposals, `instances_predictions.pth`, CPU tensors."""
import copy
import json
import logging
import os
from collections import OrderedDict

import numpy as np
import torch

from ..data.catalog import DatasetCatalog, MetadataCatalog
from ..structures import BoxMode
from ..utils import comm
from .box_scoring import BoxEvaluator
from .coco_results import coco_records
from .cocoeval import COCOevalHIP, derive_coco_results, prepare_ground_truth


def convert_to_coco_dict(dataset_name):
    """DatasetCatalog records -> COCO json dict, boxes only, the way the reference's converter does it
    (data/datasets/coco.py:283-409): XYWH boxes rounded to 3 decimals, area = the box area (f32, as `Boxes.area`), annotation
    ids from 1, `iscrowd` defaults to 0, category ids through the reverse of `thing_dataset_id_to_contiguous_id` if present"""
    records, meta = DatasetCatalog.get(dataset_name), MetadataCatalog.get(dataset_name)
    rev = None
    if hasattr(meta, "thing_dataset_id_to_contiguous_id"):
        rev = {v: k for k, v in meta.thing_dataset_id_to_contiguous_id.items()}
    cat = (lambda c: rev[c]) if rev is not None else (lambda c: c)
    categories = [{"id": cat(i), "name": name} for i, name in enumerate(meta.thing_classes)]
    images, anns = [], []
    for index, rec in enumerate(records):
        image = {"id": rec.get("image_id", index), "width": rec["width"], "height": rec["height"], "file_name": rec["file_name"]}
        images.append(image)
        for a in rec.get("annotations", []):
            bbox = BoxMode.convert(list(a["bbox"]), a["bbox_mode"], BoxMode.XYWH_ABS)
            xyxy = torch.tensor(BoxMode.convert(list(bbox), BoxMode.XYWH_ABS, BoxMode.XYXY_ABS), dtype=torch.float32)
            area = ((xyxy[2] - xyxy[0]) * (xyxy[3] - xyxy[1])).item()
            anns.append({"id": len(anns) + 1, "image_id": image["id"], "bbox": [round(float(x), 3) for x in bbox],
                         "area": float(area), "iscrowd": int(a.get("iscrowd", 0)), "category_id": cat(a["category_id"])})
    out = {"images": images, "categories": categories}
    if anns:
        out["annotations"] = anns
    return out


def load_coco_ground_truth(dataset):
    """COCO json dict (or path) -> (`prepare_ground_truth` arrays, class names by sorted category id, has annotations).
    Read directly: `load_coco_json` drops `area` and `id`."""
    if isinstance(dataset, str):
        with open(dataset) as f:
            dataset = json.load(f)
    cats = sorted(dataset.get("categories", []), key=lambda c: c["id"])
    anns = dataset.get("annotations", [])
    for a in anns:
        assert a.get("ignore", 0) == 0, '"ignore" in COCO json file is not supported.'
    gt = prepare_ground_truth([im["id"] for im in dataset["images"]], [c["id"] for c in cats], anns)
    return gt, [c["name"] for c in cats], "annotations" in dataset


def gather_detections(local, distributed=True):
    """every rank's (image ids, counts, boxes, scores, classes) on the main process, concatenated in rank order; None on
    the other ranks.  A single process keeps its device tensors; gathered arrays travel as numpy."""
    if not distributed or comm.get_world_size() == 1:
        return local
    comm.synchronize()
    mine = tuple(local[:2]) + tuple(None if t is None else t.cpu().numpy() for t in local[2:])
    shards = comm.gather(mine, dst=0)
    if not comm.is_main_process():
        return None
    shards = [s for s in shards if len(s[0])]
    ids, counts = [i for s in shards for i in s[0]], [c for s in shards for c in s[1]]
    arrays = [np.concatenate([s[j] for s in shards]) if shards else None for j in (2, 3, 4)]
    return (ids, counts) + tuple(arrays)


class COCOEvaluator(BoxEvaluator):
    def __init__(self, dataset_name, cfg=None, distributed=True, output_dir=None, *, tasks=None):
        self._logger = logging.getLogger(__name__)
        tasks = tuple(tasks) if tasks is not None else self._tasks_from_config(cfg)
        for t in tasks:
            if t != "bbox":
                raise NotImplementedError(f"COCOEvaluator: task '{t}' is not built; only 'bbox' is scored")
        self._tasks, self._distributed, self._output_dir = tasks, distributed, output_dir
        self._metadata = MetadataCatalog.get(dataset_name)
        if hasattr(self._metadata, "json_file"):
            self._gt, names, self._do_evaluation = load_coco_ground_truth(self._metadata.json_file)
        else:
            self._logger.info(f"'{dataset_name}' is not registered by `register_coco_instances`. Therefore trying to convert "
                              "it to COCO format ...")
            self._gt, names, self._do_evaluation = load_coco_ground_truth(convert_to_coco_dict(dataset_name))
        self._class_names = self._metadata.get("thing_classes") or names
        # contiguous class index of the model -> index into the sorted category ids of the ground truth
        self._rev = None
        if hasattr(self._metadata, "thing_dataset_id_to_contiguous_id"):
            self._rev = {v: k for k, v in self._metadata.thing_dataset_id_to_contiguous_id.items()}
        cat_index = {c: i for i, c in enumerate(self._gt["cat_ids"])}
        n = len(self._class_names) if self._class_names else len(cat_index)
        self._lut = [cat_index.get(self._rev[c] if self._rev is not None else c, -1) if (self._rev is None or c in self._rev)
                     else -1 for c in range(n)]
        self.reset()

    @staticmethod
    def _tasks_from_config(cfg):
        tasks = ("bbox",)
        if cfg is not None and cfg.MODEL.get("MASK_ON", False):
            tasks = tasks + ("segm",)
        if cfg is not None and cfg.MODEL.get("KEYPOINT_ON", False):
            tasks = tasks + ("keypoints",)
        return tasks

    def _instances(self, out):
        if "proposals" in out:
            raise NotImplementedError("COCOEvaluator: box proposals ('proposals' outputs) are not scored")
        return out.get("instances")

    def _gather(self, local):
        return gather_detections(local, self._distributed)

    def evaluate(self):
        merged = self._gather(self._local())
        if merged is None:
            return {}
        ids, counts, boxes, scores, classes = merged
        if len(ids) == 0:
            self._logger.warning("[COCOEvaluator] Did not receive valid predictions.")
            return {}
        boxes, scores, classes = self._checked(ids, boxes, scores, classes, "the ground-truth set", refuse=self._do_evaluation)
        self._results = OrderedDict()
        self._eval_predictions(ids, counts, boxes, scores, classes)
        return copy.deepcopy(self._results)

    def _eval_predictions(self, ids, counts, boxes, scores, classes):
        dev = boxes.device
        if self._output_dir:
            os.makedirs(self._output_dir, exist_ok=True)
            path = os.path.join(self._output_dir, "coco_instances_results.json")
            self._logger.info("Saving results to {}".format(path))
            per_det_ids = [i for i, c in zip(ids, counts) for _ in range(c)]
            with open(path, "w") as f:
                f.write(json.dumps(coco_records(boxes, scores, classes, per_det_ids, self._rev)))
        if not self._do_evaluation:
            self._logger.info("Annotations are not available for evaluation.")
            return
        self._logger.info("Evaluating predictions with the HIP COCO scorer...")
        stats, precision = None, None
        if int(scores.numel()) > 0:
            image = self._image_of(ids, counts, dev)
            lut = torch.tensor(self._lut + [-1], dtype=torch.int32, device=dev)
            cls = lut[classes.long().clamp(min=-1, max=len(self._lut) - 1)]      # out of range -> -1: the scorer reports it
            cls = torch.where((classes < 0) | (classes >= len(self._lut)), torch.full_like(cls, -1), cls)
            self.coco_eval = ev = COCOevalHIP(self._gt, boxes, scores, cls, image)
            ev.evaluate()
            ev.accumulate()        # a class without a category in the ground-truth set (-1 above) is the scorer's ValueError
            stats, precision = ev.summarize(), ev.eval["precision"]
        else:
            self._logger.warning("No predictions from the model!")
        res = derive_coco_results(stats, precision, class_names=self._class_names)
        self._logger.info("Evaluation results for bbox: \n" + create_small_table(
            {k: v for k, v in res.items() if not k.startswith("AP-")}))
        if not np.isfinite(sum(res.values())):
            self._logger.info("Some metrics cannot be computed and is shown as NaN.")
        self._results["bbox"] = res


def create_small_table(small_dict):
    """one header row, one value row (the reference's `create_small_table`, without tabulate)"""
    keys, vals = list(small_dict.keys()), ["{:.3f}".format(v) for v in small_dict.values()]
    w = [max(len(k), len(v)) for k, v in zip(keys, vals)]
    line = lambda cells: "| " + " | ".join(c.ljust(n) for c, n in zip(cells, w)) + " |"     # noqa: E731
    return "\n".join([line(keys), "|" + "|".join(":" + "-" * (n + 1) for n in w) + "|", line(vals)])
