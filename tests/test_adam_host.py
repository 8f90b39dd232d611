"""Host side of SOLVER.OPTIMIZER ADAM / ADAMW: the config keys and the refusals of `build_optimizer`, the two new entry points
of the C ABI with their argument checks, the ops wrappers, and the conversion of a `torch.optim.Adam` state dict into the flat
buffers.  Nothing here needs a GPU."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _net():
    return torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.BatchNorm2d(4), torch.nn.Conv2d(4, 2, 1))


# ------------------------------------------------------------------------------------------------------------------------
# 1. config and refusals
# ------------------------------------------------------------------------------------------------------------------------
def test_defaults_still_build_flat_sgd():
    from detectron2_centernet_amd.config import get_cfg
    from detectron2_centernet_amd.solver import FlatAdam, FlatSGD, build_optimizer
    from detectron2_centernet_amd.solver.build import FlatOptimizer

    cfg = get_cfg()
    assert cfg.SOLVER.OPTIMIZER == "SGD" and cfg.SOLVER.ADAM.BETAS == (0.9, 0.999)
    assert cfg.SOLVER.ADAM.EPS == 1e-8 and cfg.SOLVER.ADAM.AMSGRAD is False
    opt = build_optimizer(cfg, _net())
    assert type(opt) is FlatSGD and set(opt.state_dict()) == {"momentum", "first"}
    assert issubclass(FlatSGD, FlatOptimizer) and issubclass(FlatAdam, FlatOptimizer)     # one construction, not two copies


def test_adam_yaml_reaches_the_constructor(tmp_path, monkeypatch):
    from detectron2_centernet_amd.config import get_cfg
    from detectron2_centernet_amd.solver import build as B

    (tmp_path / "adam.yaml").write_text("SOLVER:\n  OPTIMIZER: ADAMW\n  BASE_LR: 0.000125\n  ADAM:\n    BETAS: [0.8, 0.99]\n"
                                        "    EPS: 1.0e-6\n    AMSGRAD: True\n  CLIP_GRADIENTS:\n    ENABLED: True\n"
                                        "    CLIP_TYPE: norm\n    CLIP_VALUE: 0.3\n")
    cfg = get_cfg()
    cfg.merge_from_file(str(tmp_path / "adam.yaml"))
    assert cfg.SOLVER.OPTIMIZER == "ADAMW" and cfg.SOLVER.ADAM.BETAS == (0.8, 0.99)
    assert cfg.SOLVER.ADAM.EPS == 1e-6 and cfg.SOLVER.ADAM.AMSGRAD is True
    seen = {}

    class Spy:
        def __init__(self, groups, base_lr, **kw):
            seen.update(kw, base_lr=base_lr, ngroups=len(list(groups)))

    monkeypatch.setattr(B, "FlatAdam", Spy)
    assert isinstance(B.build_optimizer(cfg, _net()), Spy)
    assert seen == {"betas": (0.8, 0.99), "eps": 1e-6, "decoupled": True, "amsgrad": True, "clip": ("norm", 0.3, 2.0),
                    "base_lr": 0.000125, "ngroups": 6}
    cfg.SOLVER.OPTIMIZER = "ADAM"
    B.build_optimizer(cfg, _net())
    assert seen["decoupled"] is False


def test_build_optimizer_adam_refusals():
    """an unknown optimizer names the three; Nesterov with Adam is refused, not dropped; betas / eps out of range are torch's
    ValueErrors; parameters on the CPU say where the update lives -- and none of them touches the model"""
    from detectron2_centernet_amd.config import get_cfg
    from detectron2_centernet_amd.solver import FlatAdam, build_optimizer

    net = _net()
    before = [p.data_ptr() for p in net.parameters()]
    grads = [p.grad for p in net.parameters()]
    cfg = get_cfg()
    cfg.SOLVER.OPTIMIZER = "RMSPROP"
    with pytest.raises(ValueError, match="SGD, ADAM, ADAMW"):
        build_optimizer(cfg, net)
    for name in ("ADAM", "ADAMW"):
        cfg = get_cfg()
        cfg.SOLVER.OPTIMIZER = name
        cfg.SOLVER.NESTEROV = True
        with pytest.raises(ValueError, match="NESTEROV"):
            build_optimizer(cfg, net)
        cfg.SOLVER.NESTEROV = False
        cfg.SOLVER.MOMENTUM = 123.0                                    # not read
        for betas in ((1.0, 0.999), (0.9, 1.0), (-0.1, 0.999), (0.9, 1.5)):
            cfg.SOLVER.ADAM.BETAS = betas
            with pytest.raises(ValueError, match="Invalid beta parameter"):
                build_optimizer(cfg, net)
        cfg.SOLVER.ADAM.BETAS = (0.9, 0.999)
        for eps in (0.0, -1e-8):
            cfg.SOLVER.ADAM.EPS = eps
            with pytest.raises(ValueError, match="Invalid epsilon value"):
                build_optimizer(cfg, net)
        cfg.SOLVER.ADAM.EPS = 1e-8
        with pytest.raises(NotImplementedError, match="HIP update kernel"):
            build_optimizer(cfg, net)
        cfg.SOLVER.CLIP_GRADIENTS.ENABLED = True                       # the clip refusals are FlatSGD's
        cfg.SOLVER.CLIP_GRADIENTS.CLIP_TYPE = "global_norm"
        with pytest.raises(ValueError, match="global_norm"):
            build_optimizer(cfg, net)
    with pytest.raises(NotImplementedError, match="HIP update kernel"):
        FlatAdam([(p, 1.0, 0.0) for p in net.parameters()], 0.1)
    assert [p.data_ptr() for p in net.parameters()] == before
    assert [p.grad for p in net.parameters()] == grads


# ------------------------------------------------------------------------------------------------------------------------
# 2. the C ABI
# ------------------------------------------------------------------------------------------------------------------------
def test_adam_entry_points_header_binding_library_agree():
    from detectron2_centernet_amd import _lib

    header = open(os.path.join(ROOT, "include", "ctdet_hip.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("ctdet_adam_advance", 5), ("ctdet_adam_runs", 21)):
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*)\);", header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
        assert m.group(1).split(",")[-1].strip() == "void* stream"
        assert hasattr(raw, name), name
    # betas and eps travel as f64: (float)0.999 is 4.7e-5 (relative) away from 1 - 0.001
    assert _lib.SIGNATURES["ctdet_adam_runs"][1][12:15] == [ctypes.c_double] * 3
    assert _lib.lib().ctdet_abi_version() == 8                # additions only


def test_adam_argument_checks_come_before_any_launch():
    from detectron2_centernet_amd import _lib

    l = _lib.lib()
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(20)

    def err():
        return l.ctdet_last_error()

    assert l.ctdet_adam_advance(None, one, 0.9, 0.999, None) == -22 and b"null" in err()
    assert l.ctdet_adam_advance(one, None, 0.9, 0.999, None) == -22 and b"null" in err()
    for betas in ((1.0, 0.999), (0.9, -0.5), (float("nan"), 0.999)):
        assert l.ctdet_adam_advance(one, one, *betas, None) == -22 and b"betas" in err()

    def runs(param=one, grad=one, m=one, v=one, vmax=None, run_end=one, bias=one, betas=(0.9, 0.999), eps=1e-8, amsgrad=0,
             clip_type=_lib.CLIP_NONE, clip_value=0.0, coefs=None):
        return l.ctdet_adam_runs(param, grad, m, v, vmax, 4, run_end, one, one, one, 1, bias, betas[0], betas[1], eps, 0, amsgrad,
                                 clip_type, clip_value, coefs, None)

    for kw in ({"param": None}, {"grad": None}, {"m": None}, {"v": None}, {"run_end": None}, {"bias": None}):
        assert runs(**kw) == -22 and b"null" in err(), kw
    assert runs(amsgrad=1) == -22 and b"max_exp_avg_sq" in err()
    for kw in ({"param": odd}, {"grad": odd}, {"m": odd}, {"v": odd}, {"vmax": odd, "amsgrad": 1}):
        assert runs(**kw) == -22 and b"aligned" in err(), kw
    for betas in ((1.0, 0.999), (0.9, 1.0), (-0.1, 0.5)):
        assert runs(betas=betas) == -22 and b"betas" in err()
    for eps in (0.0, -1.0):
        assert runs(eps=eps) == -22 and b"eps" in err()
    assert runs(clip_type=5, clip_value=1.0) == -22 and b"clip type" in err()
    assert runs(clip_type=_lib.CLIP_VALUE, clip_value=-1.0) == -22 and b"clip value" in err()
    assert runs(clip_type=_lib.CLIP_NORM, clip_value=1.0) == -22 and b"coefs" in err()


# ------------------------------------------------------------------------------------------------------------------------
# 3. ops
# ------------------------------------------------------------------------------------------------------------------------
def test_adam_ops_refuse_cpu_tensors():
    import detectron2_centernet_amd.ops as ops

    z, i64, i32 = torch.zeros(8), torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(NotImplementedError):
        ops.adam_advance_(i64, torch.zeros(2), 0.9, 0.999)
    with pytest.raises(NotImplementedError):
        ops.adam_runs_(z, z, z, z, None, i64, i32, torch.zeros(1), torch.zeros(1), torch.zeros(2), 0.9, 0.999, 1e-8)
    with pytest.raises(NotImplementedError):
        ops.adam_runs_(z, z, z, z, z, i64, i32, torch.zeros(1), torch.zeros(1), torch.zeros(2), 0.9, 0.999, 1e-8, amsgrad=True)


# ------------------------------------------------------------------------------------------------------------------------
# 4. torch.optim.Adam state -> flat buffers
# ------------------------------------------------------------------------------------------------------------------------
def _stepped_torch_adam(cls=torch.optim.Adam, steps=2, **kw):
    torch.manual_seed(7)
    net = torch.nn.Sequential(torch.nn.Linear(5, 4), torch.nn.Linear(4, 3), torch.nn.Linear(3, 2, bias=False))
    params = list(net.parameters())
    opt = cls([{"params": [p]} for p in params], lr=0.01, **kw)
    for _ in range(steps):
        opt.zero_grad()
        net(torch.randn(6, 5)).square().sum().backward()
        opt.step()
    return params, opt


def test_torch_adam_state_converts_to_reversed_flat_buffers():
    from detectron2_centernet_amd.solver import adam_state_from_torch

    params, ref = _stepped_torch_adam(amsgrad=True)
    sd = ref.state_dict()
    assert torch.is_tensor(sd["state"][0]["step"])                          # torch keeps a tensor per parameter
    numels = [p.numel() for p in reversed(params)]
    out = adam_state_from_torch(sd, numels, amsgrad=True)
    assert set(out) == {"exp_avg", "exp_avg_sq", "max_exp_avg_sq", "step"} and out["step"] == 2
    for key in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
        want = torch.cat([ref.state[p][key].reshape(-1) for p in reversed(params)])
        assert out[key].dtype == torch.float32 and torch.equal(out[key], want) and want.abs().sum() > 0
    assert set(adam_state_from_torch(sd, numels)) == {"exp_avg", "exp_avg_sq", "step"}
    # int steps (older torch), and a parameter that never had a gradient
    sd2 = ref.state_dict()
    for st in sd2["state"].values():
        st["step"] = 2
    del sd2["state"][4]
    out2 = adam_state_from_torch(sd2, numels, amsgrad=True)
    assert out2["step"] == 2 and torch.equal(out2["exp_avg"][:numels[0]], torch.zeros(numels[0]))
    assert torch.equal(out2["exp_avg"][numels[0]:], out["exp_avg"][numels[0]:])


def test_torch_adam_state_conversion_refusals():
    from detectron2_centernet_amd.solver import adam_state_from_torch

    params, ref = _stepped_torch_adam(amsgrad=True)
    numels = [p.numel() for p in reversed(params)]
    sd = ref.state_dict()
    sd["state"][1]["step"] = torch.tensor(3.0)
    with pytest.raises(ValueError, match="step"):
        adam_state_from_torch(sd, numels, amsgrad=True)
    sd = ref.state_dict()
    with pytest.raises(ValueError, match="5 parameters"):
        adam_state_from_torch(sd, numels + [1], amsgrad=True)
    wrong = list(numels)
    wrong[2] += 1
    with pytest.raises(ValueError, match="elements"):
        adam_state_from_torch(sd, wrong, amsgrad=True)
    _, plain = _stepped_torch_adam()
    with pytest.raises(KeyError, match="max_exp_avg_sq"):
        adam_state_from_torch(plain.state_dict(), numels, amsgrad=True)
    with pytest.raises(KeyError, match="FlatAdam"):
        adam_state_from_torch({"momentum": torch.zeros(3), "first": False}, numels)
    _, sgd = _stepped_torch_adam(torch.optim.SGD, momentum=0.9)
    with pytest.raises(KeyError, match="exp_avg"):
        adam_state_from_torch(sgd.state_dict(), numels)


def test_flat_sgd_refuses_an_adam_state():
    from detectron2_centernet_amd.solver import FlatSGD

    params, ref = _stepped_torch_adam()
    opt = FlatSGD([(p, 1.0, 0.0) for p in params], 0.1)
    with pytest.raises(KeyError, match="momentum_buffer"):
        opt.load_state_dict(ref.state_dict())
    with pytest.raises(KeyError, match="momentum"):
        opt.load_state_dict({"exp_avg": torch.zeros(1), "exp_avg_sq": torch.zeros(1), "step": 1})
