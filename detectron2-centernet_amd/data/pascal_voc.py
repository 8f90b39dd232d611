"""Pascal VOC detection sets (reference: detectron2/data/datasets/pascal_voc.py and builtin.py:205-218): the devkit tree

    <dirname>/ImageSets/Main/<split>.txt   one image id per line
    <dirname>/Annotations/<id>.xml         size, and per object: name, difficult, bndbox (1-based, inclusive)
    <dirname>/JPEGImages/<id>.jpg

read with the standard library's `xml.etree`.  Nothing registers at import: `tools/train_net.py` calls
`register_all_pascal_voc`, which registers a split only where its VOC2007 / VOC2012 directory exists."""
import os
import xml.etree.ElementTree as ET

from ..structures import BoxMode
from .catalog import DatasetCatalog, MetadataCatalog

__all__ = ["CLASS_NAMES", "VOC_SPLITS", "read_voc_ids", "read_voc_objects", "load_voc_instances", "register_pascal_voc",
           "register_all_pascal_voc"]

# the twenty classes of the VOC devkit, alphabetical
CLASS_NAMES = ("aeroplane", "bicycle", "bird", "boat", "bottle",
               "bus", "car", "cat", "chair", "cow",
               "diningtable", "dog", "horse", "motorbike", "person",
               "pottedplant", "sheep", "sofa", "train", "tvmonitor")

# (registered name, directory under the datasets root, split file, year of the AP form)
VOC_SPLITS = tuple((f"voc_{year}_{split}", f"VOC{year}", split, year)
                   for year, splits in ((2007, ("trainval", "train", "val", "test")), (2012, ("trainval", "train", "val")))
                   for split in splits)


def read_voc_ids(dirname, split):
    """the image ids of a split, in file order"""
    with open(os.path.join(dirname, "ImageSets", "Main", split + ".txt")) as f:
        return [line.split()[0] for line in f if line.strip()]


def read_voc_objects(path):
    """one annotation file -> (height, width, [(name, difficult, [xmin, ymin, xmax, ymax] as written: int, 1-based)])"""
    root = ET.parse(path).getroot()
    size = root.find("size")
    objects = []
    for obj in root.findall("object"):
        box = obj.find("bndbox")
        difficult = obj.find("difficult")
        objects.append((obj.find("name").text.strip(), int(difficult.text) if difficult is not None else 0,
                        [int(float(box.find(k).text)) for k in ("xmin", "ymin", "xmax", "ymax")]))
    return int(size.find("height").text), int(size.find("width").text), objects


def load_voc_instances(dirname, split, class_names):
    """records of a split: file_name, image_id (the id string), height, width and the objects as annotations -- XYXY_ABS with
    xmin - 1, ymin - 1 (the 1-based inclusive pixel box [1, W] becomes the coordinate box [0, W]); difficult objects included"""
    class_names = list(class_names)
    records = []
    for fileid in read_voc_ids(dirname, split):
        height, width, objects = read_voc_objects(os.path.join(dirname, "Annotations", fileid + ".xml"))
        records.append({
            "file_name": os.path.join(dirname, "JPEGImages", fileid + ".jpg"), "image_id": fileid, "height": height,
            "width": width,
            "annotations": [{"category_id": class_names.index(name), "bbox_mode": BoxMode.XYXY_ABS,
                             "bbox": [float(b[0]) - 1.0, float(b[1]) - 1.0, float(b[2]), float(b[3])]}
                            for name, _, b in objects]})
    return records


def register_pascal_voc(name, dirname, split, year, class_names=CLASS_NAMES):
    DatasetCatalog.register(name, lambda: load_voc_instances(dirname, split, class_names))
    MetadataCatalog.get(name).set(thing_classes=list(class_names), dirname=dirname, year=year, split=split,
                                  evaluator_type="pascal_voc")


def register_all_pascal_voc(root):
    """the reference's seven names under `root` (voc_2007_{trainval,train,val,test}, voc_2012_{trainval,train,val}); a split
    whose VOC<year> directory does not exist, or whose name is registered already, is left alone.  Returns the names added."""
    added = []
    for name, sub, split, year in VOC_SPLITS:
        dirname = os.path.join(root, sub)
        if os.path.isdir(dirname) and name not in DatasetCatalog:
            register_pascal_voc(name, dirname, split, year)
            added.append(name)
    return added
