from .catalog import DatasetCatalog, MetadataCatalog
from .build import InferenceSampler, TrainingSampler, build_detection_test_loader, build_detection_train_loader
from .coco import load_coco_json, register_coco_instances
from .pascal_voc import CLASS_NAMES, load_voc_instances, register_all_pascal_voc, register_pascal_voc
from .dataset_mapper import TrafficLightDatasetMapper

__all__ = ["DatasetCatalog", "MetadataCatalog", "InferenceSampler", "TrainingSampler", "build_detection_test_loader",
           "build_detection_train_loader", "load_coco_json",
           "register_coco_instances", "TrafficLightDatasetMapper", "CLASS_NAMES", "load_voc_instances",
           "register_pascal_voc", "register_all_pascal_voc"]
