"""Default values of every config key the CenterNet hot path (and its yamls) reads.
Values follow detectron2/config/defaults.py (CenterNet block :464-494; MODEL/INPUT/DATASETS/SOLVER/TEST
keys at the cited lines of that file); keys of unrelated detectors are out of scope."""
from .config import CfgNode as CN

_C = CN()
_C.VERSION = 2

_C.MODEL = CN()
_C.MODEL.LOAD_PROPOSALS = False
_C.MODEL.MASK_ON = False
_C.MODEL.KEYPOINT_ON = False
_C.MODEL.DEVICE = "cuda"
_C.MODEL.META_ARCHITECTURE = "GeneralizedRCNN"
_C.MODEL.WEIGHTS = ""
_C.MODEL.PIXEL_MEAN = [103.530, 116.280, 123.675]
_C.MODEL.PIXEL_STD = [1.0, 1.0, 1.0]

_C.MODEL.BACKBONE = CN()
_C.MODEL.BACKBONE.NAME = "build_resnet_backbone"
_C.MODEL.BACKBONE.FREEZE_AT = 2

_C.MODEL.RESNETS = CN()
_C.MODEL.RESNETS.DEPTH = 50
_C.MODEL.RESNETS.OUT_FEATURES = ["res4"]
_C.MODEL.RESNETS.NUM_GROUPS = 1
_C.MODEL.RESNETS.NORM = "FrozenBN"
_C.MODEL.RESNETS.WIDTH_PER_GROUP = 64
_C.MODEL.RESNETS.STRIDE_IN_1X1 = True
_C.MODEL.RESNETS.RES5_DILATION = 1
_C.MODEL.RESNETS.RES2_OUT_CHANNELS = 256
_C.MODEL.RESNETS.STEM_OUT_CHANNELS = 64
_C.MODEL.RESNETS.DEFORM_ON_PER_STAGE = [False, False, False, False]
_C.MODEL.RESNETS.DEFORM_MODULATED = False
_C.MODEL.RESNETS.DEFORM_NUM_GROUPS = 1

# VoVNet (defaults.py:497-504)
_C.MODEL.VOVNET = CN()
_C.MODEL.VOVNET.CONV_BODY = "V-39-eSE"
_C.MODEL.VOVNET.OUT_FEATURES = ["stage2", "stage3", "stage4", "stage5"]
_C.MODEL.VOVNET.NORM = "FrozenBN"
_C.MODEL.VOVNET.OUT_CHANNELS = 256
_C.MODEL.VOVNET.BACKBONE_OUT_CHANNELS = 256

# CenterNet (defaults.py:464-494)
_C.MODEL.CENTERNET = CN()
_C.MODEL.CENTERNET.NUM_CLASSES = 80
_C.MODEL.CENTERNET.LEVELS = [1, 1, 1, 2, 2, 1]
_C.MODEL.CENTERNET.CHANNELS = [16, 32, 64, 128, 256, 512]
_C.MODEL.CENTERNET.DOWN_RATIO = 4
_C.MODEL.CENTERNET.LAST_LEVEL = 5
_C.MODEL.CENTERNET.HEAD_CONV = 256
_C.MODEL.CENTERNET.FINAL_KERNEL = 1
_C.MODEL.CENTERNET.SIZE_DIVISIBILITY = 32
_C.MODEL.CENTERNET.HM_WEIGHT = 1
_C.MODEL.CENTERNET.WH_WEIGHT = 0.1
_C.MODEL.CENTERNET.OFF_WEIGHT = 1
_C.MODEL.CENTERNET.FOCAL_LOSS_ALPHA = [0.25]
_C.MODEL.CENTERNET.TASK = CN()
_C.MODEL.CENTERNET.TASK.HM = 80
_C.MODEL.CENTERNET.TASK.WH = 2
_C.MODEL.CENTERNET.TASK.REG = 2
_C.MODEL.CENTERNET.SCORE_THRESH_TEST = 0.05
_C.MODEL.CENTERNET.TOPK_CANDIDATES_TEST = 100
# --- keys of this build (not in the reference): numeric mode of the HIP path and local weights ---
# "f16": f16 storage + f16 MFMA with f32 accumulation (throughput mode); "f32": exact f32 kernels (parity mode)
_C.MODEL.CENTERNET.HIP_PRECISION = "f16"
# the reference downloads ImageNet weights in the backbone constructor (dla.py:297-298); here a local
# .pth path can be given instead, "" = keep the reference initialisers (no network access ever)
_C.MODEL.CENTERNET.PRETRAINED_BACKBONE = ""

_C.INPUT = CN()
_C.INPUT.MIN_SIZE_TRAIN = (800,)
_C.INPUT.MIN_SIZE_TRAIN_SAMPLING = "choice"
_C.INPUT.MAX_SIZE_TRAIN = 1333
_C.INPUT.MIN_SIZE_TEST = 800
_C.INPUT.MAX_SIZE_TEST = 1333
_C.INPUT.FORMAT = "BGR"
_C.INPUT.MASK_FORMAT = "polygon"
# not in the reference (its mapper resizes on the host with Pillow): True = the test-time mapper leaves the image as read and
# the model resizes it on the device, bit for bit what the host resize gives (ops.resize_u8).  The training
# mapper refuses it: its colour jitters run after the resize
_C.INPUT.DEVICE_RESIZE = False
# not in the reference either: True = the TRAINING mapper leaves resize and colour jitters to the model.  Its records carry the
# raw image, the size and the jitter draws it made (the host pipeline's draws, in its order); CenterNet.stage_raw_train produces
# the bytes the host pipeline gives from them (ops.resize_u8, ops.colour_jitter_u8).  The test-time mapper ignores it.
_C.INPUT.DEVICE_AUGMENT = False
# not in the reference either: CenterNet's own training input (data/warp.py).  ENABLED: the TRAINING mapper
# replaces ResizeShortestEdge by one affine warp to OUTPUT_SIZE = (out_h, out_w), each a multiple of
# MODEL.CENTERNET.SIZE_DIVISIBILITY: the source window has side max(h, w) * one of SCALES, its centre is drawn at least
# BORDER pixels from the edges (halved until it fits) and the image is mirrored with FLIP_PROB.  With INPUT.DEVICE_AUGMENT
# the warp runs on the device (ops.warp_affine_u8).  The test-time mapper ignores these keys, TEST_MODE apart.
_C.INPUT.AFFINE = CN()
_C.INPUT.AFFINE.ENABLED = False
_C.INPUT.AFFINE.OUTPUT_SIZE = (512, 512)
_C.INPUT.AFFINE.SCALES = (0.6, 0.7, 0.8, 0.9, 1.0, 1.1, 1.2, 1.3)
_C.INPUT.AFFINE.BORDER = 128
_C.INPUT.AFFINE.FLIP_PROB = 0.5
# CenterNet's TEST input, independent of ENABLED, which stays training-only: "" = off (ResizeShortestEdge);
# "fix_res" = the test-time mapper letterboxes every image to OUTPUT_SIZE by one affine warp; "keep_res" = it pads every image
# to the next multiple of MODEL.CENTERNET.SIZE_DIVISIBILITY (a power of two) above its size.  The boxes come back through the
# inverse map (ops.postprocess_affine).  The training mapper ignores the key.
_C.INPUT.AFFINE.TEST_MODE = ""

_C.DATASETS = CN()
_C.DATASETS.TRAIN = ()
_C.DATASETS.TEST = ()

_C.DATALOADER = CN()
_C.DATALOADER.NUM_WORKERS = 4
_C.DATALOADER.ASPECT_RATIO_GROUPING = True
_C.DATALOADER.SAMPLER_TRAIN = "TrainingSampler"
# frequency threshold of RepeatFactorTrainingSampler: images of a class rarer than this are repeated
_C.DATALOADER.REPEAT_THRESHOLD = 0.0
_C.DATALOADER.FILTER_EMPTY_ANNOTATIONS = True

_C.SOLVER = CN()
_C.SOLVER.LR_SCHEDULER_NAME = "WarmupMultiStepLR"
_C.SOLVER.MAX_ITER = 40000
_C.SOLVER.BASE_LR = 0.001
_C.SOLVER.MOMENTUM = 0.9
_C.SOLVER.NESTEROV = False
_C.SOLVER.WEIGHT_DECAY = 0.0001
_C.SOLVER.WEIGHT_DECAY_NORM = 0.0
_C.SOLVER.GAMMA = 0.1
_C.SOLVER.STEPS = (30000,)
_C.SOLVER.WARMUP_FACTOR = 1.0 / 1000
_C.SOLVER.WARMUP_ITERS = 1000
_C.SOLVER.WARMUP_METHOD = "linear"
_C.SOLVER.CHECKPOINT_PERIOD = 5000
_C.SOLVER.IMS_PER_BATCH = 16
_C.SOLVER.BIAS_LR_FACTOR = 1.0
_C.SOLVER.WEIGHT_DECAY_BIAS = _C.SOLVER.WEIGHT_DECAY
_C.SOLVER.CLIP_GRADIENTS = CN({"ENABLED": False})
_C.SOLVER.CLIP_GRADIENTS.CLIP_TYPE = "value"
_C.SOLVER.CLIP_GRADIENTS.CLIP_VALUE = 1.0
_C.SOLVER.CLIP_GRADIENTS.NORM_TYPE = 2.0
# not in the reference (its builder hard-codes torch.optim.SGD): "SGD" | "ADAM" | "ADAMW" (solver/build.py).
# Adam does not read MOMENTUM and refuses NESTEROV
_C.SOLVER.OPTIMIZER = "SGD"
_C.SOLVER.ADAM = CN()
_C.SOLVER.ADAM.BETAS = (0.9, 0.999)
_C.SOLVER.ADAM.EPS = 1e-8
_C.SOLVER.ADAM.AMSGRAD = False
# not in the reference: an exponential moving average of the weights and of the BatchNorm running statistics, updated behind
# every optimizer step by HIP kernels (solver/ema.py).  e += (1 - d) * (p - e) with d = DECAY, under WARMUP
# d = min(DECAY, (1 + t) / (10 + t)) at update t.  EVAL: the trainer's evaluations and `train_net.py --eval-only` score the
# averaged weights.  Checkpoints carry them under "ema"
_C.SOLVER.EMA = CN()
_C.SOLVER.EMA.ENABLED = False
_C.SOLVER.EMA.DECAY = 0.9998
_C.SOLVER.EMA.WARMUP = True
_C.SOLVER.EMA.EVAL = True

_C.TEST = CN()
_C.TEST.EXPECTED_RESULTS = []
_C.TEST.EVAL_PERIOD = 0
_C.TEST.DETECTIONS_PER_IMAGE = 100
_C.TEST.BATCH_SIZE = 1
# test-time augmentation (detectron2/config/defaults.py:634-638).  Built for the CenterNet meta-architecture as its flip
# test (modeling/test_time_augmentation.py: CenterNetWithTTA): FLIP with at most one entry in MIN_SIZES, any number of entries with TEST.SOFT_NMS
_C.TEST.AUG = CN({"ENABLED": False})
_C.TEST.AUG.MIN_SIZES = (400, 500, 600, 700, 800, 900, 1000, 1100, 1200)
_C.TEST.AUG.MAX_SIZE = 4000
_C.TEST.AUG.FLIP = True
# CenterNet's `--nms`: per-class Gaussian soft-NMS of the detections (sigma, score floor of a decayed detection), the merge of
# multi-scale testing -- with it CenterNetWithTTA takes any number of TEST.AUG.MIN_SIZES (ops.soft_nms_merge)
_C.TEST.SOFT_NMS = CN({"ENABLED": False})
_C.TEST.SOFT_NMS.SIGMA = 0.5
_C.TEST.SOFT_NMS.MIN_SCORE = 0.001
# detectron2/config/defaults.py:640-642: before every evaluation period's checkpoint and after the last iteration, recompute
# the BatchNorm running statistics as the true mean and population variance over NUM_ITER training batches
# (engine/precise_bn.py, hooks.PreciseBN).  With SOLVER.EMA.EVAL they are measured for the averaged weights
_C.TEST.PRECISE_BN = CN({"ENABLED": False})
_C.TEST.PRECISE_BN.NUM_ITER = 200

_C.OUTPUT_DIR = "./output"
_C.SEED = -1
_C.CUDNN_BENCHMARK = False
_C.VIS_PERIOD = 0
