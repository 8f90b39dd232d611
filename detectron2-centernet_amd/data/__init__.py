from .catalog import DatasetCatalog, MetadataCatalog
from .build import (InferenceSampler, RepeatFactorTrainingSampler, TrainingSampler, build_detection_test_loader,
                    build_detection_train_loader, repeat_factors_from_category_frequency)
from .coco import load_coco_json, register_coco_instances
from .lvis import load_lvis_json, register_all_lvis, register_lvis_instances
from .pascal_voc import CLASS_NAMES, load_voc_instances, register_all_pascal_voc, register_pascal_voc
from .dataset_mapper import TrafficLightDatasetMapper

__all__ = ["DatasetCatalog", "MetadataCatalog", "InferenceSampler", "TrainingSampler", "build_detection_test_loader",
           "build_detection_train_loader", "load_coco_json",
           "register_coco_instances", "TrafficLightDatasetMapper", "CLASS_NAMES", "load_voc_instances",
           "register_pascal_voc", "register_all_pascal_voc", "RepeatFactorTrainingSampler",
           "repeat_factors_from_category_frequency", "load_lvis_json", "register_lvis_instances", "register_all_lvis"]
