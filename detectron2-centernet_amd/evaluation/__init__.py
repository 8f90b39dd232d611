from .coco_evaluation import COCOEvaluator, convert_to_coco_dict, load_coco_ground_truth
from .coco_results import instances_to_coco_json, results_to_coco_json
from .cocoeval import COCOevalHIP, Params, derive_coco_results, prepare_ground_truth, summarize_stats
from .evaluator import COCOResultsWriter, DatasetEvaluator, DatasetEvaluators, inference_context, inference_on_dataset
from .lvis_evaluation import LVISEvaluator
from .lviseval import LVISevalHIP, prepare_lvis_ground_truth, summarize_lvis
from .pascal_voc_evaluation import PascalVOCDetectionEvaluator, derive_voc_results
from .voceval import VOCevalHIP, parse_voc_ground_truth, prepare_voc_ground_truth
from .testing import flatten_results_dict, print_csv_format, verify_results

__all__ = ["instances_to_coco_json", "results_to_coco_json", "DatasetEvaluator", "DatasetEvaluators", "COCOResultsWriter",
           "inference_context", "inference_on_dataset", "COCOEvaluator", "COCOevalHIP", "Params", "convert_to_coco_dict",
           "load_coco_ground_truth", "prepare_ground_truth", "summarize_stats", "derive_coco_results",
           "flatten_results_dict", "print_csv_format", "verify_results", "PascalVOCDetectionEvaluator", "derive_voc_results",
           "VOCevalHIP", "parse_voc_ground_truth", "prepare_voc_ground_truth", "LVISEvaluator", "LVISevalHIP",
           "prepare_lvis_ground_truth", "summarize_lvis"]
