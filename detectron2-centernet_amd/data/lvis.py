"""LVIS instance annotations -> Detectron2 dataset dicts, boxes only, read with the standard library's `json` (the reference
goes through the `lvis` package: detectron2/data/datasets/lvis.py, builtin.py:137-165).

The reference keeps the 1 203-row (v1) and 1 230-row (v0.5) category tables as source; here the metadata comes from the json's
own `categories` when the set is first loaded: `thing_classes` = `synonyms[0]`, else `name`, by ascending id, and
`class_frequency` = the string of their `frequency` letters (r / c / f).  Nothing registers at import: `tools/train_net.py`
calls `register_all_lvis`, which registers a split only where its json exists."""
import json
import os

from ..structures import BoxMode
from .catalog import DatasetCatalog, MetadataCatalog

__all__ = ["LVIS_SPLITS", "load_lvis_json", "lvis_metadata_from_categories", "register_lvis_instances", "register_all_lvis"]

# registered name -> (image root, json file), both under the datasets root
LVIS_SPLITS = {
    "lvis_v1_train": ("coco", "lvis/lvis_v1_train.json"),
    "lvis_v1_val": ("coco", "lvis/lvis_v1_val.json"),
    "lvis_v1_test_dev": ("coco", "lvis/lvis_v1_image_info_test_dev.json"),
    "lvis_v1_test_challenge": ("coco", "lvis/lvis_v1_image_info_test_challenge.json"),
    "lvis_v0.5_train": ("coco", "lvis/lvis_v0.5_train.json"),
    "lvis_v0.5_val": ("coco", "lvis/lvis_v0.5_val.json"),
    "lvis_v0.5_val_rand_100": ("coco", "lvis/lvis_v0.5_val_rand_100.json"),
    "lvis_v0.5_test": ("coco", "lvis/lvis_v0.5_image_info_test.json"),
    "lvis_v0.5_train_cocofied": ("coco", "lvis/lvis_v0.5_train_cocofied.json"),
    "lvis_v0.5_val_cocofied": ("coco", "lvis/lvis_v0.5_val_cocofied.json"),
}


def lvis_metadata_from_categories(categories):
    """the json's `categories` -> {"thing_classes", "class_frequency"}, by ascending category id"""
    cats = sorted(categories, key=lambda c: c["id"])
    return {"thing_classes": [c["synonyms"][0] if c.get("synonyms") else c["name"] for c in cats],
            "class_frequency": "".join(c.get("frequency", "") for c in cats)}


def load_lvis_json(json_file, image_root, dataset_name=None):
    """records in ascending image id: file_name, height, width, image_id, not_exhaustive_category_ids, neg_category_ids (both
    as in the file, dataset ids, [] when missing) and the annotations as {bbox XYWH_ABS, bbox_mode, category_id 0-based};
    segmentations are dropped.  With `dataset_name` the metadata of that name is filled from the json's categories.

    The category ids must be 1 .. K, as the reference asserts of its tables; a set whose metadata carries
    `thing_dataset_id_to_contiguous_id` (the cocofied sets, whose name says so: the mapping is then taken from the json's sorted
    ids) is mapped through it instead."""
    with open(json_file) as f:
        data = json.load(f)
    cats = sorted(data.get("categories", []), key=lambda c: c["id"])
    cat_ids = [c["id"] for c in cats]
    id_map = None
    if dataset_name is not None:
        meta = MetadataCatalog.get(dataset_name)
        if cats:
            meta.set(**{k: v for k, v in lvis_metadata_from_categories(cats).items() if not hasattr(meta, k)})
        if "cocofied" in dataset_name and cats and not hasattr(meta, "thing_dataset_id_to_contiguous_id"):
            meta.thing_dataset_id_to_contiguous_id = {v: i for i, v in enumerate(cat_ids)}
        id_map = meta.get("thing_dataset_id_to_contiguous_id")
    if id_map is None and cat_ids != list(range(1, len(cat_ids) + 1)):
        raise ValueError(f"load_lvis_json: the category ids of '{json_file}' are not 1 .. {len(cat_ids)}, as an LVIS set's are")
    by_image, ann_ids = {}, []
    for ann in data.get("annotations", []):
        by_image.setdefault(ann["image_id"], []).append(ann)
        ann_ids.append(ann.get("id"))
    if len(set(ann_ids)) != len(ann_ids):
        raise ValueError(f"load_lvis_json: annotation ids in '{json_file}' are not unique")
    records = []
    for im in sorted(data["images"], key=lambda im: im["id"]):
        if "coco_url" in im:      # the split folder ("train2017", "val2017", "test2017") is in the url, not in file_name
            file_name = os.path.join(image_root, *im["coco_url"].split("/")[-2:])
        else:
            file_name = os.path.join(image_root, im["file_name"])
        objs = []
        for ann in by_image.get(im["id"], []):
            c = ann["category_id"]
            if id_map is not None and c not in id_map:
                raise ValueError(f"load_lvis_json: annotation {ann.get('id')} of '{json_file}' has category id {c}, which is "
                                 "not in the set's id mapping")
            if id_map is None and not 1 <= c <= len(cat_ids):
                raise ValueError(f"load_lvis_json: annotation {ann.get('id')} of '{json_file}' has category id {c} outside "
                                 f"1 .. {len(cat_ids)}")
            objs.append({"bbox": ann["bbox"], "bbox_mode": BoxMode.XYWH_ABS,
                         "category_id": id_map[c] if id_map is not None else c - 1})
        records.append({"file_name": file_name, "height": im["height"], "width": im["width"], "image_id": im["id"],
                        "not_exhaustive_category_ids": im.get("not_exhaustive_category_ids", []),
                        "neg_category_ids": im.get("neg_category_ids", []), "annotations": objs})
    return records


def register_lvis_instances(name, metadata, json_file, image_root):
    """reference: data/datasets/lvis.py:24-37 (lazy load on first DatasetCatalog.get)"""
    DatasetCatalog.register(name, lambda: load_lvis_json(json_file, image_root, name))
    MetadataCatalog.get(name).set(json_file=json_file, image_root=image_root, evaluator_type="lvis", **metadata)


def register_all_lvis(root):
    """the reference's ten names under `root`; a split whose json does not exist, or whose name is registered already, is left
    alone.  Returns the names added."""
    added = []
    for name, (image_root, json_file) in LVIS_SPLITS.items():
        path = os.path.join(root, json_file)
        if os.path.isfile(path) and name not in DatasetCatalog:
            register_lvis_instances(name, {}, path, os.path.join(root, image_root))
            added.append(name)
    return added
