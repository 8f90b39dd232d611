"""CPU tests of the SyncBN / WarmupCosineLR configs (the reference's ctdet_res_*_bot_1x files, tests/golden/g17_configs, made
by tests/golden/make_g17.py): config ingestion, model construction and norm conversion by `freeze`, the state-dict layout
against the reference's, the cosine schedule against the reference formula and its selection by name."""
import math
import os
import shutil

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BOT_YAMLS = ("ctdet_res_18_bot_1x.yaml", "ctdet_res_18_larger_bot_1x.yaml", "ctdet_res_34_larger_bot_1x.yaml")


def _bot_cfg(tmp_path, name):
    from detectron2_centernet_amd.config import get_cfg

    shutil.copy(os.path.join(GOLDEN, "g16_configs", "Base-CenterNet.yaml"), tmp_path / "Base-CenterNet.yaml")
    shutil.copy(os.path.join(GOLDEN, "g17_configs", name), tmp_path / name)
    cfg = get_cfg()
    cfg.merge_from_file(str(tmp_path / name))
    cfg.MODEL.DEVICE = "cpu"
    return cfg


def _build(cfg):
    from detectron2_centernet_amd.data.catalog import register_synthetic
    from detectron2_centernet_amd.modeling import build_model

    register_synthetic(cfg.DATASETS.TRAIN[0], num_classes=1)
    return build_model(cfg)


def _keys(model):
    sd = model.state_dict()
    return sorted(f"{k} {tuple(v.shape)}" for k, v in sd.items() if k.startswith(("backbone.", "deconv_layers.")))


def _golden_keys(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return sorted(line.strip() for line in f if line.strip())


@pytest.mark.parametrize("name", BOT_YAMLS)
def test_bot_yamls_build(tmp_path, name):
    from detectron2_centernet_amd.layers import FrozenBatchNorm2d

    cfg = _bot_cfg(tmp_path, name)
    assert cfg.SOLVER.LR_SCHEDULER_NAME == "WarmupCosineLR" and cfg.DATASETS.TRAIN[0].endswith("bulb_train")
    model = _build(cfg)
    bb = model.backbone
    if cfg.MODEL.RESNETS.NORM == "SyncBN":
        for blk in (bb.stem, *bb.res2):
            norms = [m for m in blk.modules() if isinstance(m, torch.nn.modules.batchnorm._NormBase)
                     or isinstance(m, FrozenBatchNorm2d)]
            assert norms and all(isinstance(m, FrozenBatchNorm2d) for m in norms)
            assert not any(p.requires_grad for p in blk.parameters())
        for blk in (*bb.res3, *bb.res4):
            norms = [m for m in blk.modules() if isinstance(m, (torch.nn.BatchNorm2d, torch.nn.SyncBatchNorm, FrozenBatchNorm2d))]
            assert norms and all(isinstance(m, torch.nn.SyncBatchNorm) for m in norms)
            assert all(p.requires_grad for p in blk.parameters())
        # the deconv layers' norms stay per-GPU BatchNorm2d (centernet.py:_make_deconv_layer)
        assert all(type(m) is torch.nn.BatchNorm2d for m in model.deconv_layers if isinstance(m, torch.nn.BatchNorm2d))


def test_res18_bot_state_dict_matches_reference(tmp_path):
    """key / shape list of the reference's ResNet-18 with norm "SyncBN" and freeze(2), plus deconv layers (G17)"""
    model = _build(_bot_cfg(tmp_path, "ctdet_res_18_bot_1x.yaml"))
    keys = _keys(model)
    assert keys == _golden_keys("g17_resnet18_syncbn_state_dict_keys.txt")
    assert "backbone.res3.0.conv1.norm.num_batches_tracked ()" in keys
    assert "backbone.res2.0.conv1.norm.num_batches_tracked ()" not in keys


def test_frozen_bn_config_unchanged(tmp_path):
    """the same config with NORM FrozenBN: the backbone of ctdet_res_18_1x, key list G10"""
    cfg = _bot_cfg(tmp_path, "ctdet_res_18_bot_1x.yaml")
    cfg.MODEL.RESNETS.NORM = "FrozenBN"
    model = _build(cfg)
    assert _keys(model) == _golden_keys("g10_resnet18_state_dict_keys.txt")
    from detectron2_centernet_amd.layers import FrozenBatchNorm2d
    assert all(isinstance(m.norm, FrozenBatchNorm2d) for m in model.backbone.modules() if hasattr(m, "norm") and m.norm is not None)


def test_get_norm_and_freeze_conversion():
    from detectron2_centernet_amd.layers import FrozenBatchNorm2d, get_norm
    from detectron2_centernet_amd.modeling.backbone.resnet import BasicBlock

    assert type(get_norm("SyncBN", 8)) is torch.nn.SyncBatchNorm
    assert type(get_norm("nnSyncBN", 8)) is torch.nn.SyncBatchNorm
    with pytest.raises(NotImplementedError, match="naiveSyncBN"):
        get_norm("naiveSyncBN", 8)
    for norm in ("BN", "SyncBN"):
        blk = BasicBlock(16, 32, stride=2, norm=norm)
        with torch.no_grad():
            for m in blk.modules():
                if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                    m.weight.uniform_(0.5, 1.5)
                    m.bias.uniform_(-1, 1)
                    m.running_mean.uniform_(-1, 1)
                    m.running_var.uniform_(0.5, 2)
        before = {k: v.clone() for k, v in blk.state_dict().items()}
        rm = blk.conv1.norm.running_mean
        blk.freeze()
        for name in ("shortcut", "conv1", "conv2"):
            n = getattr(blk, name).norm
            assert isinstance(n, FrozenBatchNorm2d) and n.eps == 1e-5
            for k in ("weight", "bias", "running_mean", "running_var"):
                assert torch.equal(getattr(n, k), before[f"{name}.norm.{k}"])
        assert blk.conv1.norm.running_mean.data_ptr() == rm.data_ptr()     # shared, as the reference's conversion does
        assert not any(p.requires_grad for p in blk.parameters())


def _ref_cosine(it, max_iter, warmup_factor, warmup_iters, method):
    """detectron2/solver/lr_scheduler.py:52-116, restated"""
    if it >= warmup_iters:
        w = 1.0
    elif method == "constant":
        w = warmup_factor
    else:
        alpha = it / warmup_iters
        w = warmup_factor * (1 - alpha) + alpha
    return w * 0.5 * (1.0 + math.cos(math.pi * it / max_iter))


class _Opt:
    def __init__(self):
        self.f = None

    def set_lr_factor(self, f):
        self.f = f


@pytest.mark.parametrize("method", ["linear", "constant"])
def test_warmup_cosine_factors(method):
    from detectron2_centernet_amd.solver import WarmupCosineLR

    max_iter, wi, wf = 364000, 1000, 0.001
    opt = _Opt()
    sch = WarmupCosineLR(opt, max_iter, warmup_factor=wf, warmup_iters=wi, warmup_method=method)
    checks = {0: opt.f}
    for it in range(1, wi + 1):
        sch.step()
        checks[it] = opt.f
    for it in (0, wi - 1, wi):
        assert checks[it] == _ref_cosine(it, max_iter, wf, wi, method)
    for it in (max_iter // 2, max_iter):
        sch.load_state_dict({"last_epoch": it})
        assert opt.f == _ref_cosine(it, max_iter, wf, wi, method)
    assert abs(_ref_cosine(max_iter // 2, max_iter, wf, wi, method) - 0.5) < 1e-12
    assert _ref_cosine(max_iter, max_iter, wf, wi, method) < 1e-12


def test_trainer_selects_scheduler_by_name(tmp_path):
    from detectron2_centernet_amd.engine.train_loop import SimpleTrainer
    from detectron2_centernet_amd.solver import WarmupCosineLR, WarmupMultiStepLR, build_lr_scheduler

    cfg = _bot_cfg(tmp_path, "ctdet_res_18_bot_1x.yaml")
    model = _build(cfg)
    tr = SimpleTrainer(model, None, cfg)
    assert type(tr.scheduler) is WarmupCosineLR and tr.scheduler.max_iters == 364000
    assert tr.optimizer.lr == pytest.approx(cfg.SOLVER.BASE_LR * _ref_cosine(0, 364000, cfg.SOLVER.WARMUP_FACTOR,
                                                                              cfg.SOLVER.WARMUP_ITERS, "linear"))
    assert tr.sync_bn and tr.reducer.world == 1 and tr.graph_ddp        # one rank: the captured path stays
    cfg.defrost()
    cfg.SOLVER.LR_SCHEDULER_NAME = "WarmupMultiStepLR"
    assert type(build_lr_scheduler(cfg, tr.optimizer)) is WarmupMultiStepLR
    cfg.SOLVER.LR_SCHEDULER_NAME = "WarmupPolyLR"
    with pytest.raises(ValueError, match="Unknown LR scheduler"):
        build_lr_scheduler(cfg, tr.optimizer)
