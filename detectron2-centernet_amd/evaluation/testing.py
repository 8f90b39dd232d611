"""What a training script does with an evaluator's result dict (reference: detectron2/evaluation/testing.py): log it in the
"copypaste" csv form, hold it against `TEST.EXPECTED_RESULTS`, flatten it for the event storage."""
import logging
import math
import pprint
import sys
from collections.abc import Mapping

__all__ = ["flatten_results_dict", "print_csv_format", "verify_results"]


def print_csv_format(results):
    """results: {task: {metric: float}} -- three log lines per task; per-category metrics ("AP-name") are left out"""
    assert isinstance(results, Mapping) or not len(results), results
    logger = logging.getLogger(__name__)
    for task, res in results.items():
        important = [(k, v) for k, v in res.items() if "-" not in k]
        logger.info("copypaste: Task: {}".format(task))
        logger.info("copypaste: " + ",".join([k for k, _ in important]))
        logger.info("copypaste: " + ",".join(["{0:.4f}".format(v) for _, v in important]))


def verify_results(cfg, results):
    """TEST.EXPECTED_RESULTS: [(task, metric, expected, tolerance), ...].  True when the list is empty or every metric is
    there, finite and within its tolerance; otherwise the mismatch is logged and the process exits with status 1."""
    expected_results = cfg.TEST.EXPECTED_RESULTS
    if not len(expected_results):
        return True
    ok = True
    for task, metric, expected, tolerance in expected_results:
        actual = results.get(task, {}).get(metric, None)
        if actual is None or not math.isfinite(actual) or abs(actual - expected) > tolerance:
            ok = False
    logger = logging.getLogger(__name__)
    if not ok:
        logger.error("Result verification failed!")
        logger.error("Expected Results: " + str(expected_results))
        logger.error("Actual Results: " + pprint.pformat(results))
        sys.exit(1)
    logger.info("Results verification passed.")
    return ok


def flatten_results_dict(results):
    """{"a": {"b": 1}} -> {"a/b": 1}, to any depth"""
    r = {}
    for k, v in results.items():
        if isinstance(v, Mapping):
            for kk, vv in flatten_results_dict(v).items():
                r[k + "/" + kk] = vv
        else:
            r[k] = v
    return r
