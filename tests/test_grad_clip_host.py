"""Host side of SOLVER.CLIP_GRADIENTS / SOLVER.NESTEROV: the chunk table of the per-parameter norm reduction, the config
parsing with its refusals, and the new entry points of the C ABI.  Nothing here needs a GPU."""
import ctypes
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _offsets(numels):
    out, off = [], 0
    for n in numels:
        out.append((off, n))
        off += n
    return out


@pytest.mark.parametrize("numels", [
    [1], [4096], [4097], [1, 1, 1], [3, 70001, 1, 4096, 9, 8192, 4095],
    [1, 2359296, 512, 1, 589824, 3, 1179648, 64],          # a 512->512 3x3 weight next to 1-element parameters
    [0, 5, 0], [5, 0, 7],
])
def test_chunk_table_partitions_the_buffer(numels):
    """covers [0, total) exactly once, in order; no chunk crosses a parameter boundary or exceeds the chunk length; every
    parameter owns a contiguous range of chunks"""
    from detectron2_centernet_amd.solver.build import GRAD_CHUNK, grad_chunks

    offsets = _offsets(numels)
    starts, lens, ends = grad_chunks(offsets)
    assert len(starts) == len(lens) and len(ends) == len(numels)
    pos = 0
    for s, l in zip(starts, lens):
        assert s == pos and 1 <= l <= GRAD_CHUNK
        pos += l
    assert pos == sum(numels)
    first = 0
    for (off, n), last in zip(offsets, ends):
        assert last >= first
        assert sum(lens[first:last]) == n
        if n:
            assert starts[first] == off and starts[last - 1] + lens[last - 1] == off + n
            assert last - first == -(-n // GRAD_CHUNK)          # as few chunks as the length allows
        first = last
    assert first == len(starts)


def test_chunk_table_is_a_function_of_offsets_and_chunk_length():
    from detectron2_centernet_amd.solver.build import grad_chunks

    offsets = _offsets([10, 3, 8])
    assert grad_chunks(offsets, chunk=4) == ([0, 4, 8, 10, 13, 17], [4, 4, 2, 3, 4, 4], [3, 4, 6])
    assert grad_chunks(offsets, chunk=4) == grad_chunks(list(offsets), chunk=4)
    assert grad_chunks([], chunk=4) == ([], [], [])


def test_clip_config_parsing(tmp_path):
    from detectron2_centernet_amd import _lib
    from detectron2_centernet_amd.config import get_cfg
    from detectron2_centernet_amd.solver.build import _check_clip, clip_from_cfg

    cfg = get_cfg()
    assert clip_from_cfg(cfg) is None and _check_clip(None) == (_lib.CLIP_NONE, 0.0, 0)
    cfg.SOLVER.CLIP_GRADIENTS.ENABLED = True                        # the defaults: by value, 1.0
    assert _check_clip(clip_from_cfg(cfg)) == (_lib.CLIP_VALUE, 1.0, 0)
    cfg.SOLVER.CLIP_GRADIENTS.CLIP_TYPE, cfg.SOLVER.CLIP_GRADIENTS.CLIP_VALUE = "norm", 0.25
    assert _check_clip(clip_from_cfg(cfg)) == (_lib.CLIP_NORM, 0.25, _lib.NORM_L2)
    for norm, kind in ((1, _lib.NORM_L1), (1.0, _lib.NORM_L1), (2, _lib.NORM_L2), (math.inf, _lib.NORM_INF)):
        cfg.SOLVER.CLIP_GRADIENTS.NORM_TYPE = norm
        assert _check_clip(clip_from_cfg(cfg))[2] == kind
    # `.inf` is how yaml writes it
    (tmp_path / "clip.yaml").write_text("SOLVER:\n  NESTEROV: True\n  CLIP_GRADIENTS:\n    ENABLED: True\n    CLIP_TYPE: norm\n"
                                        "    CLIP_VALUE: 0.3\n    NORM_TYPE: .inf\n")
    cfg = get_cfg()
    cfg.merge_from_file(str(tmp_path / "clip.yaml"))
    assert cfg.SOLVER.NESTEROV is True and cfg.SOLVER.CLIP_GRADIENTS.NORM_TYPE == math.inf
    assert _check_clip(clip_from_cfg(cfg)) == (_lib.CLIP_NORM, pytest.approx(0.3), _lib.NORM_INF)


def _net():
    return torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.BatchNorm2d(4), torch.nn.Conv2d(4, 2, 1))


def test_build_optimizer_refusals():
    """an unknown CLIP_TYPE is a ValueError like the reference's enum; a NORM_TYPE that is not built names the three that are;
    either option for a model on the CPU says where the options live -- and none of them touches the model"""
    from detectron2_centernet_amd.config import get_cfg
    from detectron2_centernet_amd.solver.build import FlatSGD, build_optimizer

    net = _net()
    before = [p.data_ptr() for p in net.parameters()]
    cfg = get_cfg()
    cfg.SOLVER.CLIP_GRADIENTS.ENABLED = True
    cfg.SOLVER.CLIP_GRADIENTS.CLIP_TYPE = "global_norm"
    with pytest.raises(ValueError, match="global_norm"):
        build_optimizer(cfg, net)
    cfg.SOLVER.CLIP_GRADIENTS.CLIP_TYPE = "norm"
    for bad in (3.0, 0.5, 0.0, -math.inf):
        cfg.SOLVER.CLIP_GRADIENTS.NORM_TYPE = bad
        with pytest.raises(NotImplementedError, match="1, 2 and inf"):
            build_optimizer(cfg, net)
    cfg.SOLVER.CLIP_GRADIENTS.NORM_TYPE = 2.0
    cfg.SOLVER.CLIP_GRADIENTS.CLIP_VALUE = 0.0
    with pytest.raises(ValueError, match="CLIP_VALUE"):
        build_optimizer(cfg, net)
    cfg.SOLVER.CLIP_GRADIENTS.CLIP_VALUE = 1.0
    for kind in ("norm", "value"):
        cfg.SOLVER.CLIP_GRADIENTS.CLIP_TYPE = kind
        with pytest.raises(NotImplementedError, match="HIP update kernel"):
            build_optimizer(cfg, net)
    cfg.SOLVER.CLIP_GRADIENTS.ENABLED = False
    cfg.SOLVER.NESTEROV = True
    with pytest.raises(NotImplementedError, match="HIP update kernel"):
        build_optimizer(cfg, net)
    with pytest.raises(NotImplementedError, match="HIP update kernel"):
        FlatSGD([(p, 1.0, 0.0) for p in net.parameters()], 0.1, clip=("norm", 1.0, 1))
    assert [p.data_ptr() for p in net.parameters()] == before       # a refusal leaves the parameters where they were
    # with neither option the CPU optimizer is built as before, and a reference state dict that says nesterov: True loads
    cfg.SOLVER.NESTEROV = False
    opt = build_optimizer(cfg, net)
    assert opt.nesterov is False and opt.grad_norms is None and opt.clip_coefs is None
    params = list(net.parameters())
    ref = torch.optim.SGD([{"params": [p]} for p in params], lr=0.1, momentum=0.9, nesterov=True)
    for p in params:
        p.grad = torch.ones_like(p)
    ref.step()
    assert ref.state_dict()["param_groups"][0]["nesterov"] is True
    opt.load_state_dict(ref.state_dict())
    assert set(opt.state_dict()) == {"momentum", "first"} and opt._first is False


NEW_ENTRY_POINTS = ("ctdet_grad_chunk_norms", "ctdet_grad_clip_coefs", "ctdet_sgd_momentum_runs_clip")


def test_new_entry_points_header_binding_library_agree():
    from detectron2_centernet_amd import _lib

    header = open(os.path.join(ROOT, "include", "ctdet_hip.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_ENTRY_POINTS:
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*)\);", header)
        assert m, name
        nargs = len(m.group(1).split(","))
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
        assert m.group(1).split(",")[-1].strip() == "void* stream"
        assert hasattr(raw, name), name
    # the enums of the header and the binding
    for py, c in (("CLIP_NONE", "CTDET_CLIP_NONE"), ("CLIP_VALUE", "CTDET_CLIP_VALUE"), ("CLIP_NORM", "CTDET_CLIP_NORM"),
                  ("NORM_L1", "CTDET_NORM_L1"), ("NORM_L2", "CTDET_NORM_L2"), ("NORM_INF", "CTDET_NORM_INF")):
        assert int(re.search(c + r"\s*=\s*(\d+)", header).group(1)) == getattr(_lib, py)
    l = _lib.lib()
    assert l.ctdet_abi_version() == 8                # additions only
    # argument checks come before any device work: none of these calls reaches a launch
    one = ctypes.c_void_p(16)
    assert l.ctdet_grad_chunk_norms(None, 0, None, None, 0, _lib.NORM_L2, None, None) == -22
    assert b"null" in l.ctdet_last_error()
    assert l.ctdet_grad_chunk_norms(one, 4, one, one, 1, 7, one, None) == -22 and b"norm type" in l.ctdet_last_error()
    assert l.ctdet_grad_chunk_norms(ctypes.c_void_p(20), 4, one, one, 1, _lib.NORM_L2, one, None) == -22
    assert b"aligned" in l.ctdet_last_error()
    assert l.ctdet_grad_clip_coefs(one, one, 1, 1, _lib.NORM_L1, 0.0, one, one, None) == -22
    assert b"clip value" in l.ctdet_last_error()
    assert l.ctdet_sgd_momentum_runs_clip(one, one, one, 4, one, one, one, one, 1, 0.9, 0, 0, 5, 1.0, None, None) == -22
    assert b"clip type" in l.ctdet_last_error()
    assert l.ctdet_sgd_momentum_runs_clip(one, one, one, 4, one, one, one, one, 1, 0.9, 0, 0, _lib.CLIP_NORM, 1.0, None, None) == -22
    assert b"coefs" in l.ctdet_last_error()
    assert l.ctdet_sgd_momentum_runs_clip(one, one, one, 4, one, one, one, one, 1, 0.9, 0, 1, _lib.CLIP_VALUE, -1.0, None, None) == -22
    assert b"clip value" in l.ctdet_last_error()


def test_ops_wrappers_refuse_cpu_tensors():
    import detectron2_centernet_amd.ops as ops
    from detectron2_centernet_amd import _lib

    z, i64, i32 = torch.zeros(8), torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(NotImplementedError):
        ops.grad_chunk_norms_(z, i64, i32, _lib.NORM_L2, torch.zeros(1))
    with pytest.raises(NotImplementedError):
        ops.grad_clip_coefs_(torch.zeros(1), i32, _lib.NORM_L2, 1.0, torch.zeros(1), torch.zeros(1))
    with pytest.raises(NotImplementedError):
        ops.sgd_momentum_runs_clip_(z, z, z, i64, i32, torch.zeros(1), torch.zeros(1), 0.9, True, nesterov=True)
