"""`DefaultPredictor`: one image in, its detections out (reference: detectron2/engine/defaults.py:154-218).

Contract of the reference: build the model from the config, load `cfg.MODEL.WEIGHTS` through DetectionCheckpointer, take a
BGR uint8 HWC array, reverse the channel order when `INPUT.FORMAT` is "RGB", resize with ResizeShortestEdge(MIN_SIZE_TEST,
MAX_SIZE_TEST) and return `model([inputs])[0]`, boxes in the frame of the original image.

What differs here: the resize runs on the device.  The frame goes to the model as a raw record ("image_raw" / "resize_hw",
the records of a mapper built with INPUT.DEVICE_RESIZE); the RGB reversal is a view with channel stride -1 that the resize
kernel reads as it is, so the host touches the pixels once, for the pinned upload.  The result equals what the host resize
gives: the resized bytes are identical (ops.resize_u8)."""
import argparse
import contextlib
import logging
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

from ..checkpoint import DetectionCheckpointer
from ..data import MetadataCatalog, TrafficLightDatasetMapper, build_detection_test_loader, build_detection_train_loader
from ..data import transforms as T
from ..data import warp as warp_defs
from ..evaluation import (COCOEvaluator, DatasetEvaluator, LVISEvaluator, PascalVOCDetectionEvaluator, inference_on_dataset,
                          print_csv_format, verify_results)
from ..modeling.meta_arch.build import build_model
from ..solver import build_lr_scheduler, build_optimizer
from ..utils import comm
from ..utils.events import CommonMetricPrinter, JSONWriter, TensorboardXWriter, tensorboard_available
from ..utils.logger import setup_logger
from . import hooks
from .precise_bn import get_bn_modules
from .train_loop import SimpleTrainer

__all__ = ["default_argument_parser", "default_setup", "DefaultPredictor", "DefaultTrainer"]


def default_argument_parser(epilog=None):
    """the command line of a training script (reference: detectron2/engine/defaults.py:49-102)"""
    parser = argparse.ArgumentParser(
        epilog=epilog or f"""
Examples:

Run on single machine:
    $ {sys.argv[0]} --num-gpus 8 --config-file cfg.yaml MODEL.WEIGHTS /path/to/weight.pth

Run on multiple machines:
    (machine0)$ {sys.argv[0]} --machine-rank 0 --num-machines 2 --dist-url <URL> [--other-flags]
    (machine1)$ {sys.argv[0]} --machine-rank 1 --num-machines 2 --dist-url <URL> [--other-flags]
""",
        formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--config-file", default="", metavar="FILE", help="path to config file")
    parser.add_argument("--resume", action="store_true", help="whether to attempt to resume from the checkpoint directory")
    parser.add_argument("--eval-only", action="store_true", help="perform evaluation only")
    parser.add_argument("--num-gpus", type=int, default=1, help="number of gpus *per machine*")
    parser.add_argument("--num-machines", type=int, default=1, help="total number of machines")
    parser.add_argument("--machine-rank", type=int, default=0, help="the rank of this machine (unique per machine)")
    # a port that is a function of the user: a run left behind by the same user shows as an occupied port
    port = 2 ** 15 + 2 ** 14 + hash(os.getuid() if sys.platform != "win32" else 1) % 2 ** 14
    parser.add_argument("--dist-url", default="tcp://127.0.0.1:{}".format(port),
                        help="initialization URL of torch.distributed (see its documentation)")
    parser.add_argument("opts", help="Modify config options using the command-line", default=None, nargs=argparse.REMAINDER)
    return parser


def seed_all_rng(seed):
    """numpy, torch and `random` from one seed"""
    import random
    np.random.seed(seed % 2 ** 32)
    torch.manual_seed(seed)
    random.seed(seed)


def default_setup(cfg, args):
    """the start of a job (defaults.py:105-151): the output directory, the logger (stdout + OUTPUT_DIR/log.txt[.rankN]), rank
    and world size, the command line and the config in the log, the config written to OUTPUT_DIR/config.yaml, and a seed per
    rank when SEED >= 0"""
    output_dir = cfg.OUTPUT_DIR
    if comm.is_main_process() and output_dir:
        os.makedirs(output_dir, exist_ok=True)
    rank = comm.get_rank()
    logger = setup_logger(output_dir, distributed_rank=rank)
    logger.info("Rank of current process: {}. World size: {}".format(rank, comm.get_world_size()))
    logger.info("Command line arguments: " + str(args))
    if hasattr(args, "config_file") and args.config_file != "":
        with open(args.config_file, "r") as f:
            logger.info("Contents of args.config_file={}:\n{}".format(args.config_file, f.read()))
    logger.info("Running with full config:\n{}".format(cfg.dump()))
    if comm.is_main_process() and output_dir:
        path = os.path.join(output_dir, "config.yaml")
        with open(path, "w") as f:
            f.write(cfg.dump())
        logger.info("Full config saved to {}".format(path))
    if cfg.SEED >= 0:      # a different, yet deterministic seed for every worker
        seed_all_rng(cfg.SEED + rank)


class DefaultPredictor:
    """`pred = DefaultPredictor(cfg); outputs = pred(bgr_image)` -- {"instances": Instances} of that one image"""

    def __init__(self, cfg):
        self.cfg = cfg.clone()      # cfg can be modified by the model
        # INPUT.AFFINE.TEST_MODE: CenterNet's test warp in the resize's place (data.warp.test_params), on the device as well;
        # a bad value is refused before the model is built
        self.test_mode = warp_defs.check_test_mode(cfg.INPUT.AFFINE.TEST_MODE, cfg.INPUT.AFFINE.OUTPUT_SIZE,
                                                   cfg.MODEL.CENTERNET.SIZE_DIVISIBILITY)
        self.model = build_model(self.cfg)
        self.model.eval()
        if len(cfg.DATASETS.TEST):
            self.metadata = MetadataCatalog.get(cfg.DATASETS.TEST[0])
        DetectionCheckpointer(self.model).load(cfg.MODEL.WEIGHTS)
        self.aug = T.ResizeShortestEdge([cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MIN_SIZE_TEST], cfg.INPUT.MAX_SIZE_TEST)
        self.input_format = cfg.INPUT.FORMAT
        assert self.input_format in ["RGB", "BGR"], self.input_format

    def __call__(self, original_image):
        """original_image: np.ndarray uint8 (H, W, 3) in BGR order"""
        original_image = np.asarray(original_image)
        if original_image.dtype != np.uint8 or original_image.ndim != 3 or original_image.shape[2] != 3:
            raise TypeError(f"DefaultPredictor takes a uint8 (H, W, 3) image, got {original_image.dtype} {original_image.shape}")
        with torch.no_grad():
            if self.input_format == "RGB":
                original_image = original_image[:, :, ::-1]      # a view: the device resize reads channel stride -1
            height, width = original_image.shape[:2]
            if self.test_mode:
                M, out_h, out_w = warp_defs.test_params(height, width, self.test_mode, self.cfg.INPUT.AFFINE.OUTPUT_SIZE,
                                                        self.cfg.MODEL.CENTERNET.SIZE_DIVISIBILITY)
                inputs = {"image_raw": original_image, "resize_hw": (out_h, out_w), "warp": warp_defs.pack_warp(M, False),
                          "height": height, "width": width}
                return self.model([inputs])[0]
            size = int(self.aug.short_edge_length[0])
            resize_hw = self.aug.output_size(height, width, size, self.aug.max_size) if size else (height, width)
            inputs = {"image_raw": original_image, "resize_hw": resize_hw, "height": height, "width": width}
            return self.model([inputs])[0]


class DefaultTrainer(SimpleTrainer):
    """The standard training run from a config (reference: detectron2/engine/defaults.py:221-533): model, optimizer,
    scheduler and train loader built from `cfg`, `resume_or_load`, the default hooks, `train()`.

        trainer = DefaultTrainer(cfg)
        trainer.resume_or_load()      # the last checkpoint of OUTPUT_DIR, or MODEL.WEIGHTS
        trainer.train()

    What differs from the reference follows from SimpleTrainer here: the data-parallel exchange is the trainer's own bucketed
    reducer (no DistributedDataParallel wrapper), the scheduler is stepped inside the step, a record batch whose images share a
    size replays the captured step, and the step's metrics go through the device-side ring (engine/metric_ring.py): no
    per-step read-back; writers, checkpoints and evaluations flush it."""

    def __init__(self, cfg):
        logger = logging.getLogger(__name__.split(".")[0])
        if not logger.isEnabledFor(logging.INFO):
            setup_logger()
        model = self.build_model(cfg)
        optimizer = self.build_optimizer(cfg, model)
        data_loader = self.build_train_loader(cfg)
        super().__init__(model, data_loader, cfg, optimizer=optimizer, route_records=True)
        self.scheduler = self.build_lr_scheduler(cfg, optimizer)
        self.checkpointer = DetectionCheckpointer(model, cfg.OUTPUT_DIR, optimizer=optimizer, scheduler=self.scheduler)
        if self.ema is not None:      # SOLVER.EMA (built by SimpleTrainer): checkpoints carry it under "ema"
            self.checkpointer.checkpointables["ema"] = self.ema
        self.start_iter = 0
        self.max_iter = cfg.SOLVER.MAX_ITER
        self.cfg = cfg
        self.attach_metric_ring()
        self.register_hooks(self.build_hooks())

    def resume_or_load(self, resume=True):
        """resume and a checkpoint in OUTPUT_DIR: model, optimizer, scheduler and (SOLVER.EMA) the averaged weights from it,
        and training goes on at the iteration after the one it stores.  Otherwise: MODEL.WEIGHTS into the model only, from
        iteration 0.  The EMA restarts from the loaded weights whenever it did not come out of the checkpoint: it was copied
        from the initialisation before the weights arrived."""
        checkpoint = self.checkpointer.resume_or_load(self.cfg.MODEL.WEIGHTS, resume=resume)
        resuming = resume and self.checkpointer.has_checkpoint()
        if self.ema is not None and "ema" not in self.checkpointer.loaded:
            if resuming:
                logging.getLogger(__name__).warning(
                    "SOLVER.EMA is enabled, but %s carries no \"ema\" entry: the average restarts from the loaded weights",
                    self.checkpointer.get_checkpoint_file())
            self.ema.reset()
        if resuming:
            self.start_iter = checkpoint.get("iteration", -1) + 1
            self.iter = self.start_iter

    def build_hooks(self):
        """timer, learning rate, (TEST.PRECISE_BN) precise BatchNorm statistics, checkpoints, evaluation, writers -- the
        reference's order.  Every rank runs the same hooks, because the hooks that act flush the metric ring and a flush of
        several ranks is a collective (PreciseBN's merge of the ranks' statistics is one too); only the main process writes:
        the checkpointer saves nothing elsewhere, and the other ranks' writer hook has no writers."""
        cfg = self.cfg
        ret = [
            hooks.IterationTimer(),
            hooks.LRScheduler(self.optimizer, self.scheduler),
            # TEST.PRECISE_BN, before the checkpointer so that the files carry the precise statistics.  With SOLVER.EMA.EVAL
            # it runs inside the exchange: the statistics are measured for the averaged weights and go back into the EMA
            # with them ("ema" in the checkpoint); the live running statistics stay what training made them
            hooks.PreciseBN(cfg.TEST.EVAL_PERIOD, self.model, self.build_train_loader(cfg), cfg.TEST.PRECISE_BN.NUM_ITER,
                            around=self.ema.swapped if self.ema is not None and cfg.SOLVER.EMA.EVAL else None)
            if cfg.TEST.PRECISE_BN.ENABLED and get_bn_modules(self.model) else None,
            hooks.PeriodicCheckpointer(self.checkpointer, cfg.SOLVER.CHECKPOINT_PERIOD),
        ]
        ret = [h for h in ret if h is not None]

        def test_and_save_results():
            # SOLVER.EMA.EVAL: the averaged weights are exchanged into the model for the evaluation and back after it
            swapped = self.ema.swapped() if self.ema is not None and cfg.SOLVER.EMA.EVAL else contextlib.nullcontext()
            with swapped:
                self._last_eval_results = self.test(self.cfg, self.model)
            return self._last_eval_results

        # evaluation after the checkpoint: if it fails, the checkpoint is there to debug with
        ret.append(hooks.EvalHook(cfg.TEST.EVAL_PERIOD, test_and_save_results))
        # the writers last, so that the evaluation's metrics are written
        ret.append(hooks.PeriodicWriter(self.build_writers() if comm.is_main_process() else [], period=20))
        return ret

    def build_writers(self):
        """the log line, OUTPUT_DIR/metrics.json and, where `torch.utils.tensorboard` imports, a tensorboard event file"""
        os.makedirs(self.cfg.OUTPUT_DIR, exist_ok=True)
        writers = [CommonMetricPrinter(self.max_iter), JSONWriter(os.path.join(self.cfg.OUTPUT_DIR, "metrics.json"))]
        if tensorboard_available():
            writers.append(TensorboardXWriter(self.cfg.OUTPUT_DIR))
        else:
            logging.getLogger(__name__).info("torch.utils.tensorboard does not import: no tensorboard event file is written")
        return writers

    def train(self):
        """runs the training; returns the last evaluation's results when TEST.EXPECTED_RESULTS is set (after verifying
        them), otherwise nothing"""
        super().train(self.start_iter, self.max_iter)
        if len(self.cfg.TEST.EXPECTED_RESULTS) and comm.is_main_process():
            assert hasattr(self, "_last_eval_results"), "No evaluation results obtained during training!"
            verify_results(self.cfg, self._last_eval_results)
            return self._last_eval_results

    @classmethod
    def build_model(cls, cfg):
        model = build_model(cfg)
        logging.getLogger(__name__).info("Model:\n{}".format(model))
        return model

    @classmethod
    def build_optimizer(cls, cfg, model):
        return build_optimizer(cfg, model)

    @classmethod
    def build_lr_scheduler(cls, cfg, optimizer):
        return build_lr_scheduler(cfg, optimizer)

    @classmethod
    def build_train_loader(cls, cfg):
        """the CenterNet project's loader (projects/CenterNet/train_net.py:102-105): TrafficLightDatasetMapper, this rank's
        share of every batch"""
        mapper = TrafficLightDatasetMapper(cfg, is_train=True)
        return build_detection_train_loader(cfg, mapper=mapper, rank=comm.get_rank(), world_size=comm.get_world_size(),
                                            seed=max(0, int(cfg.SEED)))

    @classmethod
    def build_test_loader(cls, cfg, dataset_name):
        return build_detection_test_loader(cfg, dataset_name, rank=comm.get_rank(), world_size=comm.get_world_size())

    @classmethod
    def build_evaluator(cls, cfg, dataset_name, output_folder=None):
        if output_folder is None:
            output_folder = os.path.join(cfg.OUTPUT_DIR, "inference")
        # the dispatch of the reference's training script on the dataset's `evaluator_type`: "pascal_voc" and "lvis" have
        # their own scorers, every other (or no) type is scored as COCO
        evaluator_type = MetadataCatalog.get(dataset_name).get("evaluator_type")
        if evaluator_type == "pascal_voc":
            return PascalVOCDetectionEvaluator(dataset_name)
        if evaluator_type == "lvis":
            return LVISEvaluator(dataset_name, cfg, True, output_folder)
        return COCOEvaluator(dataset_name, cfg, True, output_folder)

    @classmethod
    def test(cls, cfg, model, evaluators=None):
        """every dataset of DATASETS.TEST through `inference_on_dataset`; evaluators: None (build_evaluator), or one per
        dataset.  Returns {dataset: results}, or the results themselves for a single dataset."""
        logger = logging.getLogger(__name__)
        if isinstance(evaluators, DatasetEvaluator):
            evaluators = [evaluators]
        if evaluators is not None:
            assert len(cfg.DATASETS.TEST) == len(evaluators), "{} != {}".format(len(cfg.DATASETS.TEST), len(evaluators))
        results = OrderedDict()
        for idx, dataset_name in enumerate(cfg.DATASETS.TEST):
            data_loader = cls.build_test_loader(cfg, dataset_name)
            if evaluators is not None:
                evaluator = evaluators[idx]
            else:
                try:
                    evaluator = cls.build_evaluator(cfg, dataset_name)
                except NotImplementedError:
                    logger.warning("No evaluator found. Use `DefaultTrainer.test(evaluators=)`, "
                                   "or implement its `build_evaluator` method.")
                    results[dataset_name] = {}
                    continue
            results_i = inference_on_dataset(model, data_loader, evaluator)
            results[dataset_name] = results_i
            if comm.is_main_process():
                assert isinstance(results_i, dict), \
                    "Evaluator must return a dict on the main process. Got {} instead.".format(results_i)
                logger.info("Evaluation results for {} in csv format:".format(dataset_name))
                print_csv_format(results_i)
        if len(results) == 1:
            results = list(results.values())[0]
        return results
