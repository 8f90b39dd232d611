"""TEST.PRECISE_BN without a GPU: the float64 restatement of tests/precise_bn_cases.py against a direct two-pass evaluation
over the rows, its bound against seeded wrong formulas, the config keys, get_bn_modules, the hook's schedule, and the
refusals of the wrappers and entry points."""
import ctypes
import math
import types

import numpy as np
import pytest
import torch

import precise_bn_cases as PC


# ------------------------------------------------------------------------------------------------------------------------
# 1. the restatement and its bound
# ------------------------------------------------------------------------------------------------------------------------
C = 6
ROWS = {"unequal": [2, 7, 300, 50, 3], "one-batch": [41], "pairs": [2, 2, 2, 2]}


def _rows(regime, counts, seed):
    """synthetic batches: [M, C] f64 rows per batch.  The batches of a regime differ in mean and spread, so that every term
    of the merge matters"""
    rng = np.random.default_rng(seed)
    out = []
    for k, M in enumerate(counts):
        if regime == "unit":
            x = rng.standard_normal((M, C)) * (0.5 + 0.25 * k) + 0.7 * k
        elif regime == "cancel":
            x = 1e3 + 1e-3 * rng.standard_normal((M, C))
        elif regime == "zero-var":
            x = np.broadcast_to(0.25 * np.arange(C) - 0.5, (M, C)).copy()      # dyadic: the two-pass sums are exact
        else:
            x = (-1.0) ** k * (1.5 + rng.standard_normal((M, C)))
        out.append(x)
    return out


def _two_pass(x):
    """mean and population variance of the rows of x [N, C], every sum exactly rounded (math.fsum): the mean carries two
    roundings, a squared deviation three, the division one"""
    N = x.shape[0]
    mean = np.array([math.fsum(x[:, c]) / N for c in range(x.shape[1])])
    var = np.array([math.fsum((x[:, c] - mean[c]) ** 2) / N for c in range(x.shape[1])])
    return mean, var


def _batch_triples(batches):
    """(M, m, u, em, eu) per batch: m and u rounded to f32 as the kernels will see them, em / eu what that rounding (and the
    f64 evaluation before it) may have cost"""
    out = []
    for x in batches:
        M = x.shape[0]
        mean, var = _two_pass(x)
        m32 = mean.astype(np.float32).astype(np.float64)
        u32 = (var * M / (M - 1)).astype(np.float32).astype(np.float64)
        out.append((np.full(C, float(M)), m32, u32, (PC.F32 + PC.g(4)) * np.abs(m32) + PC.F32_TINY,
                    (PC.F32 + PC.g(8)) * np.abs(u32) + PC.F32_TINY))
    return out


def _restated(triples):
    acc = PC.Acc(C)
    for M, m, u, em, eu in triples:
        acc.merge(M, m, u, em, eu)
    # through finish with world 1: the state is an input there, and keeps the bounds it has
    (mu, v), (emu, ev), has = acc.outputs()
    assert has.all()
    return mu, v, emu, ev


@pytest.mark.parametrize("counts", list(ROWS), ids=list(ROWS))
@pytest.mark.parametrize("regime", PC.REGIMES)
def test_restatement_matches_two_pass_over_all_rows(regime, counts):
    batches = _rows(regime, ROWS[counts], seed=11)
    mu, v, emu, ev = _restated(_batch_triples(batches))
    mean, var = _two_pass(np.concatenate(batches))
    r_mean = PC.ratio(mu, mean, emu + PC.g(3) * np.abs(mean))
    r_var = PC.ratio(v, var, ev + PC.g(8) * var)
    print(f"{regime} / {counts}: error / bound, mean {r_mean:.3g}, variance {r_var:.3g}; bound of the variance relative to it "
          f"{float(np.max(ev / np.maximum(var, 1e-300))):.3g}")
    assert r_mean <= 1.0 and r_var <= 1.0
    if regime == "zero-var":
        assert (v == 0).all() and np.array_equal(mu, mean)


def test_first_merge_is_exact_and_empty_blocks_are_skipped():
    acc = PC.Acc(3)
    m, u = np.float32([0.1, -3.0, 1e3]), np.float32([0.3, 0.0, 1e-6])
    acc.merge(np.float64([5, 2, PC.BIG]), m, u)
    assert np.array_equal(acc.mu, m.astype(np.float64)) and np.array_equal(acc.n, [5, 2, PC.BIG])
    assert np.array_equal(acc.m2, u.astype(np.float64) * np.float64([4, 1, PC.BIG - 1]))
    assert (acc.emu == 0).all() and np.array_equal(acc.em2, PC.g(1) * acc.m2)
    before = acc.state().copy()
    acc.step(0.0, 123.0, 456.0)                      # an empty slot: nothing moves, nothing divides by zero
    assert np.array_equal(acc.state(), before)
    slots = np.stack([before, np.zeros_like(before), before])
    two = PC.finish64(slots)
    assert np.array_equal(two.n, 2 * before[0]) and np.allclose(two.mu, before[1], rtol=1e-15)
    none = PC.finish64(np.zeros((2, 3, 4)))
    assert not none.outputs()[2].any()


@pytest.mark.parametrize("kind", ["no-weight", "biased-u", "mean-of-means"])
def test_every_wrong_formula_leaves_the_bound(kind):
    """unit scale, unequal row counts, batch means that differ: the right formula stays inside the bound, each seeded mistake
    -- the n M / n' factor dropped, u taken as the biased variance, the unweighted mean of the means -- leaves it"""
    batches = _rows("unit", ROWS["unequal"], seed=23)
    triples = _batch_triples(batches)
    mu, v, emu, ev = _restated(triples)
    mean, var = _two_pass(np.concatenate(batches))
    bound_mean, bound_var = emu + PC.g(3) * np.abs(mean), ev + PC.g(8) * var
    assert PC.ratio(mu, mean, bound_mean) <= 1.0 and PC.ratio(v, var, bound_var) <= 1.0
    wmu, wv = PC.wrong_chain(kind, [(M, m, u) for M, m, u, _, _ in triples])
    r_mean, r_var = PC.ratio(wmu, mean, bound_mean), PC.ratio(wv, var, bound_var)
    print(f"{kind}: error / bound, mean {r_mean:.3g}, variance {r_var:.3g}")
    if kind == "mean-of-means":
        assert r_mean > 1.0
    else:
        assert r_mean <= 1.0 and r_var > 1.0
    # the seeded formulas are the right one but for their mistake
    rmu, rv = PC.wrong_chain("none", [(M, m, u) for M, m, u, _, _ in triples])
    assert PC.ratio(rmu, mean, bound_mean) <= 1.0 and PC.ratio(rv, var, bound_var) <= 1.0


def test_case_tables_are_what_they_claim():
    assert sorted(PC.EDGES.lens) == [0, 1, 3, 4, 5, 64, 65, 257] and PC.EMPTY.total == 0 and PC.EMPTY.starts == [0]
    assert PC.SHORT_GRID.max_len < max(PC.SHORT_GRID.lens) and max(PC.CAPPED.lens) > 64 * 256
    for t in PC.TABLES:
        nseg = len(t.lens)
        per_merge = [PC.rows_of(k, nseg) for k in range(7)]
        flat = [r for rows in per_merge for r in rows]
        assert min(flat) == 2 and max(flat) >= 4 * 10 ** 6 and len(set(map(tuple, per_merge))) == 7
        assert 2 in per_merge[0] and any(r >= 4 * 10 ** 6 for r in per_merge[0])      # already in the chain of one merge
        assert all(len(set(rows)) > 1 for rows in per_merge)
        m, u = PC.batch_stats("unit", 0, t.total, 5)
        buf = t.live(m, u)
        assert t.guards_intact(buf) and all(np.array_equal(a, b) for a, b in zip(t.gather(buf), (m, u)))


# ------------------------------------------------------------------------------------------------------------------------
# 2. config, get_bn_modules, the hook
# ------------------------------------------------------------------------------------------------------------------------
def test_config_defaults_and_yaml(tmp_path):
    from detectron2_centernet_amd.config import get_cfg

    cfg = get_cfg()
    assert cfg.TEST.PRECISE_BN.ENABLED is False and cfg.TEST.PRECISE_BN.NUM_ITER == 200
    path = tmp_path / "precise.yaml"
    path.write_text("TEST:\n  PRECISE_BN:\n    ENABLED: True\n    NUM_ITER: 7\n")
    cfg.merge_from_file(str(path))
    assert cfg.TEST.PRECISE_BN.ENABLED is True and cfg.TEST.PRECISE_BN.NUM_ITER == 7


def _net():
    from detectron2_centernet_amd.layers.batch_norm import FrozenBatchNorm2d

    net = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 1), torch.nn.BatchNorm2d(4), FrozenBatchNorm2d(4), torch.nn.BatchNorm2d(4),
                              torch.nn.BatchNorm2d(4), torch.nn.SyncBatchNorm(4),
                              torch.nn.BatchNorm2d(4, track_running_stats=False), torch.nn.BatchNorm2d(4, affine=False))
    net.train()
    net[3].eval()                                   # eval mode: excluded
    for p in net[4].parameters():                   # not trainable: excluded
        p.requires_grad_(False)
    return net


def test_get_bn_modules_rule():
    from detectron2_centernet_amd.engine.precise_bn import get_bn_modules
    from detectron2_centernet_amd.solver.ema import covered_buffers

    net = _net()
    got = get_bn_modules(net)
    assert [id(m) for m in got] == [id(net[1]), id(net[5]), id(net[7])]
    # the EMA's rule with m.training added: eval mode is the only difference
    covered = {id(b) for _, b in covered_buffers(net)}
    assert covered == {id(b) for m in got + [net[3]] for b in (m.running_mean, m.running_var)}
    net.eval()
    assert get_bn_modules(net) == []


def test_update_bn_stats_has_no_cpu_implementation():
    from detectron2_centernet_amd.engine.precise_bn import update_bn_stats

    net = _net()
    before = [b.clone() for b in net.buffers()]
    with pytest.raises(NotImplementedError, match="no CPU implementation"):
        update_bn_stats(net, iter([]), 2)
    assert all(torch.equal(a, b) for a, b in zip(net.buffers(), before)) and net[1].momentum == 0.1
    update_bn_stats(net.eval(), iter([]), 2)         # nothing to do: returns before it looks at the loader or the device


def _fired(period, max_iter, model=None):
    from detectron2_centernet_amd.engine import hooks

    fired = []

    class Stubbed(hooks.PreciseBN):
        def update_stats(self):
            fired.append(self.trainer.iter + 1)

    hook = Stubbed(period, _net() if model is None else model, [], 3)
    hook.trainer = types.SimpleNamespace(iter=0, max_iter=max_iter)
    for it in range(max_iter):
        hook.trainer.iter = it
        hook.after_step()
    return fired, hook


def test_hook_schedule():
    assert _fired(0, 7)[0] == [7]                                   # period 0: only after the last iteration
    assert _fired(3, 7)[0] == [3, 6, 7]
    assert _fired(3, 6)[0] == [3, 6]                                # the last iteration on the period: once
    assert _fired(10, 4)[0] == [4]


def test_hook_is_disabled_without_covered_layers(caplog):
    import logging
    from detectron2_centernet_amd.engine import hooks

    with caplog.at_level(logging.INFO):
        lg = logging.getLogger(hooks.__name__)
        lg.addHandler(caplog.handler)
        try:
            hook = hooks.PreciseBN(1, _net().eval(), None, 3)
        finally:
            lg.removeHandler(caplog.handler)
    assert hook._disabled and "PreciseBN is disabled" in caplog.text
    hook.trainer = types.SimpleNamespace(iter=0, max_iter=1)
    hook.after_step()                                # does nothing: there is no loader to touch
    assert "PreciseBN" in hooks.__all__


def test_hook_keeps_one_iterator_and_a_throw_away_storage(monkeypatch):
    from detectron2_centernet_amd.engine import hooks
    from detectron2_centernet_amd.utils.events import EventStorage, get_event_storage

    calls = []

    def fake_update(model, loader, num_iter):
        calls.append(([next(loader) for _ in range(num_iter)], get_event_storage()))

    monkeypatch.setattr(hooks, "update_bn_stats", fake_update)
    entered = []

    class Around:
        def __enter__(self):
            entered.append("in")

        def __exit__(self, *exc):
            entered.append("out")

    hook = hooks.PreciseBN(2, _net(), list(range(10)), 3, around=Around)
    with EventStorage() as outer:
        hook.update_stats()
        hook.update_stats()
    assert [c[0] for c in calls] == [[0, 1, 2], [3, 4, 5]]            # the second run goes on where the first stopped
    assert all(c[1] is not outer for c in calls) and entered == ["in", "out", "in", "out"]


# ------------------------------------------------------------------------------------------------------------------------
# 3. refusals that need no device
# ------------------------------------------------------------------------------------------------------------------------
def test_wrappers_refuse_on_the_host():
    from detectron2_centernet_amd import ops

    i64 = lambda *v: torch.tensor(v, dtype=torch.int64)      # noqa: E731
    ptrs, starts, state = i64(0, 0, 0), i64(0, 4, 8, 12), torch.zeros(3, 12, dtype=torch.float64)
    with pytest.raises(ValueError, match=r"rows\[2\] = 1"):
        ops.precise_bn_merge_(ptrs, ptrs, starts, [2, 5, 1], 4, state)
    with pytest.raises(ValueError, match=r"rows\[0\] = 0"):
        ops.precise_bn_merge_(ptrs, ptrs, starts, [0, 5, 1], 4, state)
    with pytest.raises(ValueError, match="3 segments, 2 row counts"):
        ops.precise_bn_merge_(ptrs, ptrs, starts, [2, 5], 4, state)
    with pytest.raises(ValueError, match="offsets"):
        ops.precise_bn_merge_(ptrs, ptrs, starts[:3], [2, 5, 3], 4, state)
    with pytest.raises(ValueError, match="variance pointers"):
        ops.precise_bn_merge_(ptrs, ptrs[:2], starts, [2, 5, 3], 4, state)
    with pytest.raises(TypeError, match="float64"):
        ops.precise_bn_merge_(ptrs, ptrs, starts, [2, 5, 3], 4, state.float())
    with pytest.raises(TypeError, match="int64"):
        ops.precise_bn_merge_(ptrs.int(), ptrs, starts, [2, 5, 3], 4, state)
    with pytest.raises(TypeError, match="int64"):
        ops.precise_bn_merge_(ptrs, ptrs, starts, torch.tensor([2.0, 5.0, 3.0]), 4, state)
    with pytest.raises(ValueError, match=r"\[3, total\]"):
        ops.precise_bn_merge_(ptrs, ptrs, starts, [2, 5, 3], 4, state[:2])
    slots = torch.zeros(2, 3, 12, dtype=torch.float64)
    with pytest.raises(ValueError, match=r"\[world, 3, total\]"):
        ops.precise_bn_finish_(ptrs, ptrs, starts, 4, state)
    with pytest.raises(TypeError, match="float64"):
        ops.precise_bn_finish_(ptrs, ptrs, starts, 4, slots.float())
    with pytest.raises(ValueError, match="offsets"):
        ops.precise_bn_finish_(ptrs, ptrs, starts[:2], 4, slots)
    # everything in order, but on the CPU: no implementation
    with pytest.raises(NotImplementedError, match="no CPU implementation"):
        ops.precise_bn_merge_(ptrs, ptrs, starts, [2, 5, 3], 4, state)
    with pytest.raises(NotImplementedError, match="no CPU implementation"):
        ops.precise_bn_finish_(ptrs, ptrs, starts, 4, slots)


def test_symbols_and_refusals_of_the_entry_points():
    from detectron2_centernet_amd import _lib

    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert _lib.SIGNATURES["ctdet_precise_bn_merge_segments"] == (i32, [vp, vp, vp, vp, i32, i64, vp, i64, vp])
    assert _lib.SIGNATURES["ctdet_precise_bn_finish_segments"] == (i32, [vp, vp, vp, i32, i64, vp, i32, i64, vp])
    lib = _lib.lib()
    merge, finish = lib.ctdet_precise_bn_merge_segments, lib.ctdet_precise_bn_finish_segments
    # nseg == 0 returns 0 before anything is looked at; the other refusals come before any launch
    assert merge(None, None, None, None, 0, 0, None, 0, None) == 0
    assert finish(None, None, None, 0, 0, None, 1, 0, None) == 0
    assert merge(None, None, None, None, 1, 1, None, 1, None) == -22 and b"null pointer" in lib.ctdet_last_error()
    assert finish(None, None, None, 1, 1, None, 1, 1, None) == -22 and b"null pointer" in lib.ctdet_last_error()
    assert merge(None, None, None, None, -1, 0, None, 0, None) == -22 and b"nseg=-1" in lib.ctdet_last_error()
    assert merge(None, None, None, None, 0, -1, None, 0, None) == -22 and b"max_len=-1" in lib.ctdet_last_error()
    assert merge(None, None, None, None, 0, 0, None, -1, None) == -22 and b"total=-1" in lib.ctdet_last_error()
    assert finish(None, None, None, -1, 0, None, 1, 0, None) == -22 and b"nseg=-1" in lib.ctdet_last_error()
    assert finish(None, None, None, 0, -1, None, 1, 0, None) == -22
    assert finish(None, None, None, 0, 0, None, 1, -1, None) == -22
    one = ctypes.c_void_p(8)                          # never dereferenced: world is refused first
    assert finish(one, one, one, 1, 1, one, 0, 1, None) == -22 and b"world=0" in lib.ctdet_last_error()
