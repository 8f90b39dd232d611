"""SOLVER.EMA without a GPU: the error bound of tests/ema_cases.py holds a numpy f32 evaluation and rejects the seeded wrong
formulas; the warm-up schedule as known answers; the naming table and the state dict on a CPU model; config keys, refusals
and the C ABI's symbol table."""
import ctypes

import numpy as np
import pytest
import torch

import ema_cases as EC


# ------------------------------------------------------------------------------------------------------------------------
# 1. bound and wrong formulas
# ------------------------------------------------------------------------------------------------------------------------
def _trajectory(steps=12, n=4096, seed=3):
    """e0 and `steps` snapshots of p: a random walk of relative step 1e-3 (nearby values, p - e exact) over five decades"""
    r = np.random.default_rng(seed)
    p = (r.standard_normal(n) * 10.0 ** r.uniform(-3, 2, n)).astype(np.float32)
    snaps = []
    for _ in range(steps):
        p = (p * (1.0 + 1e-3 * r.standard_normal(n))).astype(np.float32)
        snaps.append(p)
    return snaps[0].copy(), snaps


@pytest.mark.parametrize("warmup", [True, False])
@pytest.mark.parametrize("evaluate", [EC.lerp_f32_unfused, EC.lerp_f32_fused], ids=["unfused", "fused"])
def test_f32_evaluations_stay_inside_the_running_bound(evaluate, warmup):
    e0, snaps = _trajectory()
    chain, e = EC.Chain(e0, warmup=warmup), e0.copy()
    worst = 0.0
    for p in snaps:
        w = chain.update(p)
        e = evaluate(e, p, w)
        worst = max(worst, EC.ratio(e, chain.e, chain.bound))
    print(f"worst |f32 - f64| / bound over {len(snaps)} steps: {worst:.3f}")
    assert 0.0 < worst <= 1.0
    # the bound is no free pass: it stays within a few ulps of the values
    assert (chain.bound <= 16 * EC.U * np.abs(chain.e) + 1e-30).all()


@pytest.mark.parametrize("wrong", EC.WRONG)
def test_every_wrong_formula_leaves_the_bound(wrong):
    e0, snaps = _trajectory()
    chain, bad = EC.Chain(e0), EC.Chain(e0, wrong=wrong)
    for p in snaps:
        chain.update(p)
        bad.update(p)
    r = EC.ratio(bad.e.astype(np.float32), chain.e, chain.bound)
    print(f"{wrong}: {r:.3g} bounds away")
    assert r > 100.0


def test_wrong_schedules_differ_only_where_they_should():
    assert EC.weight_at(0, wrong="weight_of_previous_update") == EC.weight_at(0)
    assert EC.weight_at(3, wrong="weight_of_previous_update") == EC.weight_at(2)
    assert EC.weight_at(5, wrong="updates_not_advanced") == EC.weight_at(0)
    assert EC.weight_at(0, wrong="warmup_ignored") == EC.f32(1.0 - EC.DECAY)


# ------------------------------------------------------------------------------------------------------------------------
# 2. the schedule
# ------------------------------------------------------------------------------------------------------------------------
def test_warmup_known_answers():
    from detectron2_centernet_amd.solver.ema import ema_decay

    assert EC.decay_at(0) == 0.1 and EC.weight_at(0) == float(np.float32(0.9))
    assert EC.decay_at(1) == 2.0 / 11.0 and EC.decay_at(90) == 0.91
    # (1 + t) / (10 + t) >= 0.9998  <=>  t >= (10 * 0.9998 - 1) / 0.0002 = 44989 (up to rounding: the search decides)
    t = EC.crossover()
    assert t in (44989, 44990)
    assert EC.decay_at(t - 1) < EC.DECAY == EC.decay_at(t) == EC.decay_at(10 ** 9)
    assert EC.weight_at(t) == float(np.float32(1.0 - 0.9998))
    assert EC.decay_at(0, warmup=False) == EC.DECAY and EC.weight_at(0, warmup=False) == float(np.float32(1.0 - 0.9998))
    assert EC.crossover(0.5) == 8 and EC.decay_at(8, 0.5) == 0.5 and EC.decay_at(7, 0.5) == 8.0 / 17.0
    for t in (0, 1, 7, 8, 44988, 44990):
        for warm in (True, False):
            assert ema_decay(t, EC.DECAY, warm) == EC.decay_at(t, EC.DECAY, warm)


# ------------------------------------------------------------------------------------------------------------------------
# 3. naming table and state dict on the CPU
# ------------------------------------------------------------------------------------------------------------------------
class _Frozen(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("running_mean", torch.zeros(4))
        self.register_buffer("running_var", torch.ones(4))


def _cpu_net():
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 6, 3), torch.nn.BatchNorm2d(6), torch.nn.Conv2d(6, 5, 1), torch.nn.BatchNorm2d(5),
                              _Frozen(), torch.nn.BatchNorm2d(5, track_running_stats=False), torch.nn.BatchNorm2d(3))
    for p in net[6].parameters():      # a norm layer whose parameters are frozen: not covered
        p.requires_grad_(False)
    net.register_buffer("pixel_mean", torch.zeros(3, 1, 1))
    return net


def _table(net):
    from detectron2_centernet_amd.solver.ema import EmaTable

    params = [p for p in reversed(list(net.parameters())) if p.requires_grad]
    offsets, off = [], 0
    for p in params:
        offsets.append((off, p.numel()))
        off += p.numel()
    return EmaTable(net, params, offsets), params, off


def test_table_names_cover_what_training_writes():
    from detectron2_centernet_amd.solver.ema import STAT_ALIGN, covered_buffers, stat_layout

    net = _cpu_net()
    assert [n for n, _ in covered_buffers(net)] == ["1.running_mean", "1.running_var", "3.running_mean", "3.running_var"]
    table, params, total = _table(net)
    names = [n for n, _, _, _ in table.params]
    assert names == ["5.bias", "5.weight", "3.bias", "3.weight", "2.bias", "2.weight", "1.bias", "1.weight", "0.bias", "0.weight"]
    assert set(names) | {n for n, _, _, _ in table.buffers} <= set(net.state_dict())
    # segments of 6, 6, 5, 5 elements start on multiples of STAT_ALIGN
    assert STAT_ALIGN == 4 and stat_layout([6, 6, 5, 5]) == ([0, 8, 16, 24], 32)
    assert [off for _, off, _, _ in table.buffers] == [0, 8, 16, 24] and table.stats_total == 32
    with pytest.raises(ValueError, match="do not belong"):
        from detectron2_centernet_amd.solver.ema import EmaTable
        EmaTable(net, [torch.nn.Parameter(torch.zeros(2))], [(0, 2)])


def test_state_dict_round_trip_and_refusals():
    net = _cpu_net()
    table, params, total = _table(net)
    g = torch.Generator().manual_seed(1)
    flat_p, flat_s = torch.randn(total, generator=g), torch.randn(table.stats_total, generator=g)
    sd = table.pack(flat_p, flat_s, 7, 0.999)
    assert set(sd) == {"params", "buffers", "updates", "decay"} and sd["updates"] == 7 and sd["decay"] == 0.999
    assert set(sd["params"]) == {n for n, p in net.named_parameters() if p.requires_grad}
    assert set(sd["buffers"]) == {"1.running_mean", "1.running_var", "3.running_mean", "3.running_var"}
    for name, off, n, shape in table.params + table.buffers:
        t = sd["params"].get(name, sd["buffers"].get(name))
        assert t.dtype == torch.float32 and t.device.type == "cpu" and tuple(t.shape) == shape
    off = dict((n, o) for n, o, _, _ in table.params)["0.weight"]
    assert torch.equal(sd["params"]["0.weight"].reshape(-1), flat_p[off:off + 6 * 3 * 9])
    assert torch.equal(sd["buffers"]["3.running_var"], flat_s[24:29])
    back_p, back_s = torch.zeros(total), torch.full((table.stats_total,), -1.0)
    assert table.unpack(sd, back_p, back_s) == 7
    assert torch.equal(back_p, flat_p)
    pad = torch.ones(table.stats_total, dtype=torch.bool)
    for _, o, n, _ in table.buffers:
        pad[o:o + n] = False
    assert torch.equal(back_s[~pad], flat_s[~pad]) and (back_s[pad] == -1.0).all()      # the padding is nobody's
    # refusals name the entry and write nothing
    for kind, name, exc in (("params", "2.weight", KeyError), ("buffers", "1.running_var", KeyError)):
        bad = {k: dict(v) if isinstance(v, dict) else v for k, v in sd.items()}
        del bad[kind][name]
        untouched = torch.zeros(total)
        with pytest.raises(exc, match=name):
            table.unpack(bad, untouched, torch.zeros(table.stats_total))
        assert not untouched.any()
    bad = {k: dict(v) if isinstance(v, dict) else v for k, v in sd.items()}
    bad["params"]["0.bias"] = torch.zeros(7)
    with pytest.raises(ValueError, match="0.bias"):
        table.unpack(bad, torch.zeros(total), torch.zeros(table.stats_total))


def test_load_into_model_on_the_cpu():
    from detectron2_centernet_amd.solver.ema import ModelEMA

    net = _cpu_net()
    table, params, total = _table(net)
    g = torch.Generator().manual_seed(2)
    sd = table.pack(torch.randn(total, generator=g), torch.randn(table.stats_total, generator=g), 3, 0.9)
    other = _cpu_net()
    frozen_before = other[6].weight.clone()
    ModelEMA.load_into_model(other, sd)
    got = other.state_dict()
    for name, t in list(sd["params"].items()) + list(sd["buffers"].items()):
        assert torch.equal(got[name], t), name
    assert torch.equal(other[6].weight, frozen_before) and int(other[1].num_batches_tracked) == 0
    with pytest.raises(KeyError, match="nope"):
        ModelEMA.load_into_model(other, {"params": {"nope": torch.zeros(1)}, "buffers": {}})
    with pytest.raises(ValueError, match="0.bias"):
        ModelEMA.load_into_model(other, {"params": {"0.bias": torch.zeros(2)}, "buffers": {}})


# ------------------------------------------------------------------------------------------------------------------------
# 4. config, refusals, ABI
# ------------------------------------------------------------------------------------------------------------------------
def test_config_keys_and_builder():
    from detectron2_centernet_amd.config import get_cfg
    from detectron2_centernet_amd.solver import build_model_ema

    cfg = get_cfg()
    e = cfg.SOLVER.EMA
    assert (e.ENABLED, e.DECAY, e.WARMUP, e.EVAL) == (False, 0.9998, True, True)
    assert build_model_ema(cfg, None, None) is None            # disabled: nothing is touched
    cfg.merge_from_list(["SOLVER.EMA.ENABLED", "True", "SOLVER.EMA.DECAY", "0.99"])
    assert cfg.SOLVER.EMA.ENABLED is True and cfg.SOLVER.EMA.DECAY == 0.99


def test_refusals_on_the_host():
    from detectron2_centernet_amd.solver import FlatSGD, ModelEMA
    from detectron2_centernet_amd.solver.ema import check_decay

    for bad in (1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="DECAY"):
            check_decay(bad)
    assert check_decay(0) == 0.0 and check_decay(0.9998) == 0.9998
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 1), torch.nn.BatchNorm2d(4))
    opt = FlatSGD([(p, 1.0, 0.0) for p in net.parameters()], 0.1)
    assert opt.ema is None
    with pytest.raises(ValueError, match="DECAY"):
        ModelEMA(net, opt, decay=1.0)
    with pytest.raises(NotImplementedError, match="no CPU implementation"):
        ModelEMA(net, opt)


def test_symbols_and_abi_version():
    from detectron2_centernet_amd import _lib

    vp, i32, i64, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    assert _lib.SIGNATURES["ctdet_ema_advance"] == (i32, [vp, vp, f64, i32, vp])
    assert _lib.SIGNATURES["ctdet_ema_lerp_segments"] == (i32, [vp, vp, vp, i32, i64, vp, vp])
    assert _lib.SIGNATURES["ctdet_ema_swap_segments"] == (i32, [vp, vp, vp, i32, i64, vp])
    lib = _lib.lib()
    assert lib.ctdet_abi_version() == 8
    # the refusals that need no device: checked before anything is launched
    assert lib.ctdet_ema_advance(None, None, 0.5, 1, None) == -22 and b"null pointer" in lib.ctdet_last_error()
    assert lib.ctdet_ema_lerp_segments(None, None, None, 0, 0, None, None) == 0
    assert lib.ctdet_ema_swap_segments(None, None, None, 0, 0, None) == 0
    assert lib.ctdet_ema_lerp_segments(None, None, None, 1, 0, None, None) == -22
    assert lib.ctdet_ema_swap_segments(None, None, None, -1, 0, None) == -22 and b"nseg=-1" in lib.ctdet_last_error()
    assert lib.ctdet_ema_lerp_segments(None, None, None, 0, -1, None, None) == -22
