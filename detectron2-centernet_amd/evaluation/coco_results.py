"""Hand-off of the decoded detections to COCO evaluation: the wire format of
detectron2/evaluation/coco_evaluation.py:321-382 (`instances_to_coco_json`: XYWH boxes, one dict per detection) and the
category-id remapping of `COCOEvaluator._eval_predictions` (:147-163).  Scoring itself is in cocoeval.py / coco_evaluation.py."""
import torch


def coco_records(boxes, scores, classes, image_ids, reverse_id_mapping=None):
    """host boxes f32 [n,4] XYXY, scores [n], classes [n] and one image id per detection -> the COCO results list: XYWH in
    f32 (BoxMode.XYXY_ABS -> XYWH_ABS, structures/boxes.py:100-103), contiguous class indices mapped back to dataset category
    ids when the mapping is given.  Shared by `instances_to_coco_json` (per image) and `COCOEvaluator` (whole dataset)."""
    boxes = torch.as_tensor(boxes).detach().float().cpu().reshape(-1, 4).clone()
    boxes[:, 2] -= boxes[:, 0]
    boxes[:, 3] -= boxes[:, 1]
    boxes = boxes.tolist()
    scores = torch.as_tensor(scores).detach().cpu().tolist()
    classes = torch.as_tensor(classes).detach().cpu().tolist()
    if reverse_id_mapping is not None:
        for c in classes:
            assert c in reverse_id_mapping, f"A prediction has category_id={c}, which is not available in the dataset."
        classes = [reverse_id_mapping[c] for c in classes]
    return [{"image_id": image_ids[k], "category_id": classes[k], "bbox": boxes[k], "score": scores[k]} for k in range(len(scores))]


def instances_to_coco_json(instances, img_id):
    """list of {"image_id", "category_id", "bbox" [x, y, w, h], "score"} for one image (boxes only)."""
    n = len(instances) if instances.has("scores") else 0
    if n == 0:
        return []
    return coco_records(instances.pred_boxes.tensor, instances.scores, instances.pred_classes, [img_id] * n)


def results_to_coco_json(outputs, image_ids, dataset_id_to_contiguous_id=None):
    """model outputs (list of {"instances": Instances}) -> flat COCO results list; with the dataset's
    `thing_dataset_id_to_contiguous_id` the contiguous class indices are mapped back to dataset category ids."""
    results = []
    for out, img_id in zip(outputs, image_ids):
        results.extend(instances_to_coco_json(out["instances"], img_id))
    if dataset_id_to_contiguous_id is not None:
        rev = {v: k for k, v in dataset_id_to_contiguous_id.items()}
        for r in results:
            assert r["category_id"] in rev, f"A prediction has category_id={r['category_id']}, which is not available in the dataset."
            r["category_id"] = rev[r["category_id"]]
    return results
