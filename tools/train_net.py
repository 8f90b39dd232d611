#!/usr/bin/env python
"""CenterNet training script (the shape of the reference's projects/CenterNet/train_net.py: setup / main / launch).

    tools/train_net.py --config-file ctdet_dla_34_1x.yaml [--resume] [--eval-only] [--num-gpus N] [KEY VALUE ...]

Trains to OUTPUT_DIR (checkpoints, metrics.json, log.txt, config.yaml), or with --eval-only scores MODEL.WEIGHTS (with
--resume: the last checkpoint of OUTPUT_DIR) on DATASETS.TEST.  With TEST.AUG.ENABLED the model is tested through
CenterNetWithTTA.  With SOLVER.EMA.ENABLED and SOLVER.EMA.EVAL, --eval-only scores the averaged weights a checkpoint carries
under "ema" (a checkpoint without them: its "model", with a warning).  The Pascal VOC splits ("voc_2007_test", ...) are
registered from $DETECTRON2_DATASETS (default "datasets") where VOC2007 / VOC2012 exist there, and scored by
PascalVOCDetectionEvaluator.  The configs' "bulb_train" / "bulb_val" are not distributed: with CTDET_SYNTHETIC_SET="train images,test images,size" in the
environment (e.g. "64,16,512") a dataset the config names but nothing has registered is replaced by the synthetic set, written
once as PNG files under OUTPUT_DIR/synthetic; without it an unregistered name is an error."""
import json
import logging
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import detectron2_centernet_amd  # noqa: E402,F401
from detectron2_centernet_amd.checkpoint import DetectionCheckpointer  # noqa: E402
from detectron2_centernet_amd.config import get_cfg  # noqa: E402
from detectron2_centernet_amd.data import register_all_lvis, register_all_pascal_voc  # noqa: E402
from detectron2_centernet_amd.data.catalog import DatasetCatalog, register_synthetic_files  # noqa: E402
from detectron2_centernet_amd.engine import DefaultTrainer, default_argument_parser, default_setup, launch  # noqa: E402
from detectron2_centernet_amd.evaluation import verify_results  # noqa: E402
from detectron2_centernet_amd.solver.ema import ModelEMA  # noqa: E402
from detectron2_centernet_amd.utils import comm  # noqa: E402

# CTDET_SYNTHETIC_SET="train images,test images,size" (e.g. "64,16,512"): opt-in -- with it, a dataset of the config that
# nothing has registered is replaced by the synthetic set.  Without it such a name is an error, as in the reference: a
# mistyped dataset name must not train on synthetic images
SYNTHETIC_SET = os.environ.get("CTDET_SYNTHETIC_SET", "")


class Trainer(DefaultTrainer):
    """DefaultTrainer already builds what the reference's script overrides: the TrafficLightDatasetMapper loader and the
    COCOEvaluator.  What is added: TEST.AUG."""

    @classmethod
    def test(cls, cfg, model, evaluators=None):
        if cfg.TEST.AUG.ENABLED:
            from detectron2_centernet_amd.modeling import CenterNetWithTTA
            logging.getLogger(__name__).info("Running inference with test-time augmentation ...")
            model = CenterNetWithTTA(cfg, model)
        return super().test(cfg, model, evaluators)


def register_missing_datasets(cfg):
    """CTDET_SYNTHETIC_SET only: the synthetic set under every dataset name of the config that nothing has registered; the
    main process writes the files, the others wait for it"""
    missing = [(n, "train") for n in cfg.DATASETS.TRAIN if n not in DatasetCatalog]
    missing += [(n, "test") for n in cfg.DATASETS.TEST if n not in DatasetCatalog]
    if not missing:
        return
    if not SYNTHETIC_SET:
        raise KeyError("datasets {} of the config are not registered (register them, e.g. with register_coco_instances; "
                       "CTDET_SYNTHETIC_SET=\"train images,test images,size\" replaces them by the synthetic set)".format(
                           sorted({n for n, _ in missing})))
    n_train, n_test, size = (int(v) for v in SYNTHETIC_SET.split(","))
    images = {"train": n_train, "test": n_test}
    root = os.path.join(cfg.OUTPUT_DIR, "synthetic")
    log = logging.getLogger(__name__)
    for rank_turn in (True, False):
        if comm.is_main_process() == rank_turn:
            for name, split in missing:
                register_synthetic_files(name, root, length=images[split], size=size, num_classes=cfg.MODEL.CENTERNET.NUM_CLASSES)
                log.warning("CTDET_SYNTHETIC_SET: dataset '%s' is not registered, using %d synthetic images under %s", name,
                            images[split], root)
        comm.synchronize()


def setup(args):
    cfg = get_cfg()
    cfg.merge_from_file(args.config_file)
    cfg.merge_from_list(args.opts)
    cfg.freeze()
    default_setup(cfg, args)
    # the Pascal VOC splits (voc_2007_*, voc_2012_*) whose VOC2007 / VOC2012 directory exists under the datasets root
    register_all_pascal_voc(os.getenv("DETECTRON2_DATASETS", "datasets"))
    # ... and the LVIS splits (lvis_v1_*, lvis_v0.5_*) whose json exists under it
    register_all_lvis(os.getenv("DETECTRON2_DATASETS", "datasets"))
    register_missing_datasets(cfg)
    return cfg


def main(args):
    cfg = setup(args)
    if args.eval_only:
        model = Trainer.build_model(cfg)
        rest = DetectionCheckpointer(model, save_dir=cfg.OUTPUT_DIR).resume_or_load(cfg.MODEL.WEIGHTS, resume=args.resume)
        if cfg.SOLVER.EMA.ENABLED and cfg.SOLVER.EMA.EVAL:
            if "ema" in rest:
                ModelEMA.load_into_model(model, rest["ema"])
                logging.getLogger(__name__).info("SOLVER.EMA.EVAL: evaluating the checkpoint's averaged weights (%d updates)",
                                                 rest["ema"]["updates"])
            else:
                logging.getLogger(__name__).warning("SOLVER.EMA.EVAL: the checkpoint carries no \"ema\" entry; evaluating "
                                                    "its \"model\" weights")
        res = Trainer.test(cfg, model)
        if comm.is_main_process():
            with open(os.path.join(cfg.OUTPUT_DIR, "eval_results.json"), "w") as f:      # the figures at full precision
                json.dump(res, f)
            verify_results(cfg, res)
        return res
    trainer = Trainer(cfg)
    trainer.resume_or_load(resume=args.resume)
    return trainer.train()


if __name__ == "__main__":
    args = default_argument_parser().parse_args()
    print("Command Line Args:", args)
    launch(main, args.num_gpus, num_machines=args.num_machines, machine_rank=args.machine_rank, dist_url=args.dist_url,
           args=(args,))
