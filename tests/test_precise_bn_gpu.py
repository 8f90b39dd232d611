"""TEST.PRECISE_BN on the GPU: the two kernels of csrc/precise_bn.hip against the float64 restatement and the derived bound of
tests/precise_bn_cases.py, `update_bn_stats` end to end on DLA-34 and on a ResNet with frozen and trainable norms, the
trainer's hook with and without SOLVER.EMA, and two ranks on one device.

The kernel and the restatement both obey the bound, so they may differ by twice its f64 part (precise_bn_cases.py); finish
adds the f32 rounding of its stores."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

import precise_bn_cases as PC
from test_trainer_gpu import clean_logger  # noqa: F401 -- DefaultTrainer sets the package logger up for the whole process

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------------
# 1. the kernels
# ------------------------------------------------------------------------------------------------------------------------
class Device:
    """a Table on the device: the live f32 buffer (means and variances between sentinel guards), the pointer / offset tables
    and a guarded f64 buffer of `lead` x total channels (the state: lead 3; the slots: 3 * world)"""

    def __init__(self, table, dev, lead=3):
        self.table, self.dev = table, dev
        self.live = torch.full((table.live_size,), PC.SENTINEL, dtype=torch.float32, device=dev)
        at = lambda offs: torch.tensor([self.live.data_ptr() + 4 * o for o in offs], dtype=torch.int64, device=dev)  # noqa: E731
        self.mean_ptrs, self.var_ptrs = at(table.mean_off), at(table.var_off)
        self.starts = torch.tensor(table.starts, dtype=torch.int64, device=dev)
        self.full = torch.full((2 * PC.GUARD + lead * table.total,), PC.SENTINEL, dtype=torch.float64, device=dev)
        self.body = self.full[PC.GUARD:PC.GUARD + lead * table.total]
        self.body.zero_()
        assert self.body.data_ptr() % 8 == 0

    def put_live(self, buf):
        self.live.copy_(torch.from_numpy(buf))

    def guards_intact(self):
        full = self.full.cpu().numpy()
        return bool((full[:PC.GUARD] == PC.SENTINEL).all() and (full[-PC.GUARD:] == PC.SENTINEL).all())


def _channel_rows(table, k):
    rows = PC.rows_of(k, len(table.lens))
    return rows, np.asarray(rows, dtype=np.float64)[table.seg_of()]


@pytest.mark.parametrize("regime", PC.REGIMES)
@pytest.mark.parametrize("chain", PC.CHAINS)
@pytest.mark.parametrize("table", PC.TABLES, ids=lambda t: t.name)
def test_merge_against_the_restatement(dev, table, chain, regime):
    from detectron2_centernet_amd import ops

    d = Device(table, dev)
    state = d.body.view(3, table.total)
    acc, worst = PC.Acc(table.total), 0.0
    for k in range(chain):
        m, u = PC.batch_stats(regime, k, table.total, seed=31)
        rows, M = _channel_rows(table, k)
        live0 = table.live(m, u)
        d.put_live(live0)
        ops.precise_bn_merge_(d.mean_ptrs, d.var_ptrs, d.starts, rows, table.max_len, state)
        acc.merge(M, m, u)
        torch.cuda.synchronize()
        got = state.cpu().numpy()
        assert np.array_equal(d.live.cpu().numpy().view(np.uint32), live0.view(np.uint32))      # merge only reads the live side
        assert d.guards_intact()
        assert np.array_equal(got[0], acc.n)
        if k == 0:      # into a zero state: mu = m and M2 = u (M - 1), bit for bit
            assert np.array_equal(got[1], m.astype(np.float64)) and np.array_equal(got[2], u.astype(np.float64) * (M - 1.0))
        r_mu, r_m2 = PC.ratio(got[1], acc.mu, 2 * acc.emu), PC.ratio(got[2], acc.m2, 2 * acc.em2)
        worst = max(worst, r_mu, r_m2)
        assert r_mu <= 1.0 and r_m2 <= 1.0, (k, r_mu, r_m2)
    print(f"{table.name}, {chain} merges, {regime}: worst error / (2 x running bound) {worst:.3f}")
    if regime == "zero-var":
        assert (got[2] == 0).all()


def test_no_segments_is_a_no_op(dev):
    from detectron2_centernet_amd import ops

    none, start = torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    state = torch.full((3, 4), PC.SENTINEL, dtype=torch.float64, device=dev)
    slots = torch.full((2, 3, 4), PC.SENTINEL, dtype=torch.float64, device=dev)
    ops.precise_bn_merge_(none, none, start, [], 0, state)
    ops.precise_bn_finish_(none, none, start, 0, slots)
    torch.cuda.synchronize()
    assert (state == PC.SENTINEL).all() and (slots == PC.SENTINEL).all()


def _slot_states(table, world, seed):
    """`world` states as chains of 1 .. 3 merges leave them, as exact f64 inputs of finish: [world][3][total]"""
    out = []
    for r in range(world):
        acc = PC.Acc(table.total)
        for k in range(1 + r % 3):
            m, u = PC.batch_stats("unit" if r % 2 == 0 else "alt-sign", k, table.total, seed=seed + r)
            acc.merge(_channel_rows(table, k + r)[1], m, u)
        out.append(acc.state())
    return np.stack(out)


def _finish(d, slots):
    from detectron2_centernet_amd import ops

    table = d.table
    world = slots.shape[0]
    dd = Device(table, d.dev, lead=3 * world)
    dd.body.copy_(torch.from_numpy(slots.reshape(-1)))
    ops.precise_bn_finish_(dd.mean_ptrs, dd.var_ptrs, dd.starts, table.max_len, dd.body.view(world, 3, table.total))
    torch.cuda.synchronize()
    live = dd.live.cpu().numpy()
    assert table.guards_intact(live) and dd.guards_intact()
    assert np.array_equal(dd.body.cpu().numpy(), slots.reshape(-1))            # the slots are only read
    return table.gather(live)


def _check_finish(got, acc, what):
    """got (mean, var) f32 against the restatement's f64 values: twice the f64 part, then the f32 store"""
    (mu, v), (emu, ev), has = acc.outputs()
    mean, var = (a.astype(np.float64) for a in got)
    r_mean = PC.ratio(mean[has], mu[has], 2 * emu[has] + PC.f32_part(np.abs(mu[has]) + 2 * emu[has]))
    r_var = PC.ratio(var[has], v[has], 2 * ev[has] + PC.f32_part(v[has] + 2 * ev[has]))
    print(f"{what}: error / bound, mean {r_mean:.3f}, variance {r_var:.3f} over {int(has.sum())} channels")
    assert r_mean <= 1.0 and r_var <= 1.0, what
    assert (mean[~has] == PC.SENTINEL).all() and (var[~has] == PC.SENTINEL).all(), what       # n = 0: left untouched
    return has


@pytest.mark.parametrize("table", [PC.EDGES, PC.SHORT_GRID], ids=lambda t: t.name)
def test_finish_against_the_restatement(dev, table):
    d = Device(table, dev)
    one = _slot_states(table, 1, seed=50)
    assert _check_finish(_finish(d, one), PC.finish64(one), f"{table.name}, world 1").all()
    # world 1 is a conversion: (float)mu and (float)(M2 / n), bit for bit
    mean, var = _finish(d, one)
    assert np.array_equal(mean, one[0, 1].astype(np.float32)) and np.array_equal(var, (one[0, 2] / one[0, 0]).astype(np.float32))

    three = _slot_states(table, 3, seed=60)
    a, b = table.starts[1], table.starts[2]                 # segment 1 has no rows on any rank: its statistics stay
    three[:, :, a:b] = 0.0
    got3 = _finish(d, three)
    has = _check_finish(got3, PC.finish64(three), f"{table.name}, world 3")
    assert not has[a:b].any() and has[:a].all() and has[b:].all()
    # an all-zero slot in the middle changes nothing, bit for bit -- wherever it sits
    pair = three[[0, 2]]
    got2 = _finish(d, pair)
    zero = np.zeros_like(pair[0])
    for where, padded in (("middle", [pair[0], zero, pair[1]]), ("first", [zero, pair[0], pair[1]]), ("last", [pair[0], pair[1], zero])):
        got = _finish(d, np.stack(padded))
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(got, got2)), where
    # the slots in another rank order: each within its own bound, hence both near each other
    perm = three[[2, 0, 1]]
    gotp = _finish(d, perm)
    _check_finish(gotp, PC.finish64(perm), f"{table.name}, world 3 permuted")
    (mu, v), (emu, ev), _ = PC.finish64(three).outputs()
    for x, y, val, e in ((got3[0], gotp[0], mu, emu), (got3[1], gotp[1], v, ev)):
        assert PC.ratio(x[has], y[has], 2 * (2 * e[has] + PC.f32_part(np.abs(val[has]) + 2 * e[has]))) <= 1.0


def test_entry_points_refuse_bad_arguments(dev):
    from detectron2_centernet_amd import _lib

    lib = _lib.lib()
    live = torch.full((16,), 3.0, device=dev)
    ptrs = torch.tensor([live.data_ptr()], dtype=torch.int64, device=dev)
    vptrs = torch.tensor([live.data_ptr() + 32], dtype=torch.int64, device=dev)
    starts = torch.tensor([0, 8], dtype=torch.int64, device=dev)
    rows = torch.tensor([5], dtype=torch.int64, device=dev)
    state = torch.ones(3, 8, dtype=torch.float64, device=dev)
    slots = torch.ones(2, 3, 8, dtype=torch.float64, device=dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())       # noqa: E731
    null = ctypes.c_void_p(0)

    def refused(rc, words):
        assert rc == -22 and words in lib.ctdet_last_error().decode(), (rc, lib.ctdet_last_error())

    good = [P(ptrs), P(vptrs), P(starts), P(rows), 1, 8, P(state), 8, None]
    for i in (0, 1, 2, 3, 6):
        refused(lib.ctdet_precise_bn_merge_segments(*(good[:i] + [null] + good[i + 1:])), "null pointer")
    refused(lib.ctdet_precise_bn_merge_segments(*(good[:4] + [-1] + good[5:])), "nseg=-1")
    refused(lib.ctdet_precise_bn_merge_segments(*(good[:5] + [-1] + good[6:])), "max_len=-1")
    refused(lib.ctdet_precise_bn_merge_segments(*(good[:7] + [-1] + good[8:])), "total=-1")
    refused(lib.ctdet_precise_bn_merge_segments(*(good[:6] + [ctypes.c_void_p(state.data_ptr() + 4)] + good[7:])), "aligned")
    good = [P(ptrs), P(vptrs), P(starts), 1, 8, P(slots), 2, 8, None]
    for i in (0, 1, 2, 5):
        refused(lib.ctdet_precise_bn_finish_segments(*(good[:i] + [null] + good[i + 1:])), "null pointer")
    refused(lib.ctdet_precise_bn_finish_segments(*(good[:3] + [-1] + good[4:])), "nseg=-1")
    refused(lib.ctdet_precise_bn_finish_segments(*(good[:4] + [-1] + good[5:])), "max_len=-1")
    refused(lib.ctdet_precise_bn_finish_segments(*(good[:7] + [-1] + good[8:])), "total=-1")
    for world in (0, -3):
        refused(lib.ctdet_precise_bn_finish_segments(*(good[:6] + [world] + good[7:])), f"world={world}")
    assert lib.ctdet_precise_bn_merge_segments(null, null, null, null, 0, 0, null, 0, None) == 0
    assert lib.ctdet_precise_bn_finish_segments(null, null, null, 0, 0, null, 1, 0, None) == 0
    torch.cuda.synchronize()
    assert (live == 3).all() and (state == 1).all() and (slots == 1).all()          # a refusal launches nothing


# ------------------------------------------------------------------------------------------------------------------------
# 2. update_bn_stats end to end
# ------------------------------------------------------------------------------------------------------------------------
def _records(B, h, w, seed):
    """B training records of one size: random bytes (every BatchNorm input then has spread) and one box each"""
    from detectron2_centernet_amd.structures import Boxes, Instances

    g = torch.Generator().manual_seed(seed)
    recs = []
    for b in range(B):
        inst = Instances((h, w))
        inst.gt_boxes = Boxes(torch.tensor([[4.0, 4.0, w - 6.0, h - 6.0]]))
        inst.gt_classes = torch.zeros(1, dtype=torch.int64)
        image = torch.randint(0, 256, (3, h, w), generator=g, dtype=torch.uint8)
        image[:, : h // 2] //= (2 + b)              # not stationary: the batches' statistics differ
        recs.append({"image": image, "instances": inst, "height": h, "width": w})
    return recs


def _batches():
    """B = 2 at 64 x 64, B = 1 at 64 x 96, B = 3 at 32 x 64: every layer, the stride-32 ones included, sees >= 2 rows"""
    return [_records(2, 64, 64, 1), _records(1, 64, 96, 2), _records(3, 32, 64, 3)]


def _stats(mods):
    torch.cuda.synchronize()
    return (torch.cat([m.running_mean.detach().reshape(-1) for m in mods]).cpu().numpy(),
            torch.cat([m.running_var.detach().reshape(-1) for m in mods]).cpu().numpy())


def _bits(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def _own_batch_stats(model, mods, batch):
    """what the project's own momentum-1 forward leaves for ONE batch: per covered layer (m, u) f32, and the row count of the
    map its BatchNorm kernel was handed -- taken from that tensor's shape at the kernel's wrapper, not from the walk
    `update_bn_stats` records.  -> (m [total], u [total], rows per layer, synchronised per layer); the model is left as found"""
    from detectron2_centernet_amd import ops_train
    from detectron2_centernet_amd.engine import train_step

    seen = {}
    fwd, sync = ops_train.bn_train_fwd, ops_train.bn_sync_fwd

    def spy_fwd(y, gamma, beta, running_mean, *a, **k):
        seen[running_mean.data_ptr()] = (y.shape[0] * y.shape[1] * y.shape[2], False)
        return fwd(y, gamma, beta, running_mean, *a, **k)

    def spy_sync(y, stats, gamma, beta, running_mean, *a, **k):
        seen[running_mean.data_ptr()] = (y.shape[0] * y.shape[1] * y.shape[2], True)
        return sync(y, stats, gamma, beta, running_mean, *a, **k)

    before = _bits(model)
    momenta = [m.momentum for m in mods]
    ops_train.bn_train_fwd, ops_train.bn_sync_fwd = spy_fwd, spy_sync
    try:
        for m in mods:
            m.momentum = 1.0
        with torch.no_grad():
            train_step.centernet_stats_forward(model, batch)
        mean, var = _stats(mods)
    finally:
        ops_train.bn_train_fwd, ops_train.bn_sync_fwd = fwd, sync
        for m, mom in zip(mods, momenta):
            m.momentum = mom
        model.load_state_dict(before)
    rows, synced = zip(*(seen[m.running_mean.data_ptr()] for m in mods))
    return mean, var, list(rows), list(synced)


def _restate(per_rank, numels):
    """per_rank[r]: that rank's batches as (m, u, rows per layer) with the rows its merge uses -> the Acc after finish"""
    total = int(sum(numels))
    final = PC.Acc(total)
    for batches in per_rank:
        acc = PC.Acc(total)
        for m, u, rows in batches:
            acc.merge(np.repeat(np.asarray(rows, dtype=np.float64), numels), m, u)
        final.step(acc.n, acc.mu, acc.m2, acc.emu, acc.em2)
    return final


@pytest.fixture(scope="module")
def dla(tmp_path_factory, dev):
    """DLA-34 in f32 mode after update_bn_stats over the three batches, with everything the checks below compare -- computed
    once, left unchanged"""
    from test_model_gpu import make_model
    from detectron2_centernet_amd import ops
    from detectron2_centernet_amd.engine.precise_bn import get_bn_modules, update_bn_stats

    tmp = tmp_path_factory.mktemp("precise_bn")
    model, cfg = make_model(tmp, "f32", seed=8, calibrated=False)
    model.train()
    mods = get_bn_modules(model)
    batches = _batches()
    x_eval = ops.preprocess(torch.stack([r["image"] for r in batches[0]]).to(dev), cfg.MODEL.PIXEL_MEAN, cfg.MODEL.PIXEL_STD, 64,
                            64, out_dtype=model._ctx.dtype)

    def eval_out():
        model.eval()
        out = [t.clone() for t in model._network_outputs(x_eval, apply_sigmoid=False)]
        model.train()
        return out

    own = [_own_batch_stats(model, mods, b) for b in batches]
    inputs = [model.preprocess_image(b)[0].nhwc[..., :3].double().cpu() for b in batches]
    out_before = eval_out()                 # also warms the eval caches with the old statistics
    before = _bits(model)
    update_bn_stats(model, batches, 3)
    torch.cuda.synchronize()
    return dict(model=model, cfg=cfg, mods=mods, batches=batches, own=own, inputs=inputs, before=before, after=_bits(model),
                out_before=out_before, out_after=eval_out(), x_eval=x_eval, tmp=tmp)


def test_dla34_statistics_equal_the_restatement_of_its_own_batch_statistics(dla):
    """(a) order, row counts and plumbing of all 55 layers: the restatement is fed what the momentum-1 forward leaves for
    each batch on its own, with the row counts of the maps"""
    mods, own = dla["mods"], dla["own"]
    assert len(mods) == 55 and not any(s for o in own for s in o[3])      # every BatchNorm of this DLA-34
    numels = [m.running_mean.numel() for m in mods]
    rows = [o[2] for o in own]
    assert min(min(r) for r in rows) == 6 and rows[0][0] == 2 * 64 * 64 and rows[1][0] == 64 * 96 and rows[2][0] == 3 * 32 * 64
    acc = _restate([[(o[0], o[1], o[2]) for o in own]], numels)
    names = {id(m): n for n, m in dla["model"].named_modules()}
    mean = torch.cat([dla["after"][names[id(m)] + ".running_mean"].reshape(-1) for m in mods]).cpu().numpy()
    var = torch.cat([dla["after"][names[id(m)] + ".running_var"].reshape(-1) for m in mods]).cpu().numpy()
    assert _check_finish((mean, var), acc, "DLA-34, three batches").all()
    assert np.array_equal(acc.n, np.repeat(np.sum(rows, axis=0).astype(np.float64), numels))


def test_dla34_first_layer_against_a_float64_convolution(dla):
    """(b) the independent anchor: the stem's 7x7 conv + BatchNorm.  torch CPU float64 convolution of the same preprocessed
    images, mean and population variance over all rows of all three batches.

    Tolerance: the rule tests/bn_cases.py applies to the f32 BatchNorm statistics -- per batch, with K the batch's first row
    and n = bn_cases.n_red(M, CV) f32 additions,
        b_dm = (n + 1) U mean |y - K|,   b_var = (n + 3) U mean (y - K)^2 + 2 |dm| b_dm + b_dm^2,
    4 U |value| for the running-statistic store -- combined over the batches by its rank rule (weights M_b / N: averaging
    does not amplify), plus U |value| for PreciseBN's own f32 store.  The f32 convolution's own rounding is not in it."""
    import bn_cases as T

    model, mods = dla["model"], dla["mods"]
    conv, bn = model.backbone.base.base_layer[0], model.backbone.base.base_layer[1]
    assert any(bn is m for m in mods)
    w = conv.weight.detach().double().cpu()
    ys = [torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), w, None, conv.stride, conv.padding).permute(0, 2, 3, 1)
          .reshape(-1, w.shape[0]) for x in dla["inputs"]]
    allrows = torch.cat(ys)
    N = allrows.shape[0]
    mean, var = allrows.mean(0), allrows.var(0, unbiased=False)
    U = 2.0 ** -24
    b_mean, b_var = U * mean.abs(), U * var
    for y in ys:
        M = y.shape[0]
        f = y - y[0]
        n, dm = T.n_red(M, w.shape[0] // 4), f.mean(0)
        b_dm = (n + 1) * U * f.abs().mean(0)
        b_v = (n + 3) * U * f.square().mean(0) + 2 * dm.abs() * b_dm + b_dm ** 2
        wgt = M / N
        b_mean = b_mean + wgt * (b_dm + 4 * U * y.mean(0).abs())
        b_var = b_var + wgt * (b_v + 4 * U * y.var(0, unbiased=False) + 2 * (y.mean(0) - mean).abs() * b_dm + b_dm ** 2)
    got_mean = dla["after"]["backbone.base.base_layer.1.running_mean"].double().cpu()
    got_var = dla["after"]["backbone.base.base_layer.1.running_var"].double().cpu()
    r_mean, r_var = PC.ratio(got_mean, mean, b_mean), PC.ratio(got_var, var, b_var)
    print(f"stem BatchNorm over {N} rows: error / bound, mean {r_mean:.3f}, variance {r_var:.3f}; relative error, mean "
          f"{float(((got_mean - mean).abs() / mean.abs()).max()):.2e}, variance {float(((got_var - var).abs() / var).max()):.2e}")
    assert r_mean <= 1.0 and r_var <= 1.0
    # the biased / unbiased distinction is far outside it: 1 / N of the variance
    assert PC.ratio(got_var, var * N / (N - 1), b_var) > 1.0


def test_dla34_nothing_else_changes(dla, dev):
    """(c) parameters bit-unchanged, no .grad, momenta restored, num_batches_tracked + 3; the eval output differs and equals
    that of a fresh model loaded with the new state dict"""
    from test_model_gpu import make_model

    model, before, after = dla["model"], dla["before"], dla["after"]
    changed = 0
    for k in before:
        if k.endswith("num_batches_tracked"):
            assert int(after[k]) == int(before[k]) + 3, k
        elif k.endswith("running_mean") or k.endswith("running_var"):
            changed += not torch.equal(before[k], after[k])
        else:
            assert torch.equal(before[k].view(torch.uint8), after[k].view(torch.uint8)), k
    assert changed == 2 * len(dla["mods"])
    assert all(p.grad is None for p in model.parameters())
    assert all(m.momentum == 0.1 for m in dla["mods"]) and model.training
    assert not any(torch.equal(a, b) for a, b in zip(dla["out_before"], dla["out_after"]))
    fresh, _ = make_model(dla["tmp"], "f32", seed=9, calibrated=False)
    fresh.load_state_dict(after)
    out = fresh._network_outputs(dla["x_eval"], apply_sigmoid=False)
    for a, b in zip(out, dla["out_after"]):
        assert torch.equal(a, b)


def test_a_failing_loader_leaves_no_trace(dla):
    """(d) two batches, then the loader raises: momenta, running statistics (and counters) are back to their bits"""
    from detectron2_centernet_amd.engine.precise_bn import update_bn_stats

    model, batches = dla["model"], dla["batches"]
    start = _bits(model)

    def loader():
        yield batches[0]
        yield batches[1]
        raise OSError("the disk went away")

    with pytest.raises(OSError, match="disk went away"):
        update_bn_stats(model, loader(), 3)
    # the loader ends early: the same
    with pytest.raises(RuntimeError, match="2 of 3 batches"):
        update_bn_stats(model, batches[:2], 3)
    torch.cuda.synchronize()
    for k, v in _bits(model).items():
        assert torch.equal(v.reshape(-1).view(torch.uint8), start[k].reshape(-1).view(torch.uint8)), k
    assert all(m.momentum == 0.1 for m in dla["mods"])
    from detectron2_centernet_amd.engine import train_step
    assert train_step._STATS_WALK is None


def test_frozen_norms_are_left_alone(tmp_path, dev):
    """a res_18_bot-shaped model: FrozenBN in the stem and res2, trainable SyncBN in res3 / res4, BatchNorm in the deconv
    layers.  Only the trainable layers are written; every other buffer keeps its bits"""
    from test_syncbn_gpu import _bot_model
    from detectron2_centernet_amd.engine.precise_bn import get_bn_modules, update_bn_stats
    from detectron2_centernet_amd.layers.batch_norm import FrozenBatchNorm2d

    model, cfg, _ = _bot_model(str(tmp_path), "f32")
    mods = get_bn_modules(model)
    frozen = [m for m in model.modules() if isinstance(m, FrozenBatchNorm2d)]
    assert frozen and mods and any(isinstance(m, torch.nn.SyncBatchNorm) for m in mods)
    written = {id(b) for m in mods for b in (m.running_mean, m.running_var, m.num_batches_tracked)}
    batches = [_records(2, 64, 64, 4), _records(1, 64, 96, 5)]
    own = [_own_batch_stats(model, mods, b) for b in batches]
    before = {k: v.detach().clone() for k, v in model.named_buffers()}
    params = {k: v.detach().clone() for k, v in model.named_parameters()}
    update_bn_stats(model, batches, 2)
    torch.cuda.synchronize()
    for k, v in model.named_buffers():
        if id(v) in written:
            assert not torch.equal(v, before[k]), k
        else:
            assert torch.equal(v.view(torch.uint8), before[k].view(torch.uint8)), k
    for k, v in model.named_parameters():
        assert torch.equal(v, params[k]) and v.grad is None, k
    acc = _restate([[(o[0], o[1], o[2]) for o in own]], [m.running_mean.numel() for m in mods])
    assert _check_finish(_stats(mods), acc, "res_18_bot, two batches").all()


# ------------------------------------------------------------------------------------------------------------------------
# 3. the trainer
# ------------------------------------------------------------------------------------------------------------------------
def _cycle_trainer(batches, seen=None):
    """DefaultTrainer on a fixed cycle of batches (the training loader and PreciseBN's loader each get their own iterator),
    without the evaluation hook; seen: a list that receives the live statistics right before PreciseBN's after_step"""
    from detectron2_centernet_amd.engine import DefaultTrainer, hooks
    from detectron2_centernet_amd.engine.precise_bn import get_bn_modules

    class Cycle(DefaultTrainer):
        @classmethod
        def build_model(cls, cfg):
            import bench
            return bench.build_model(cfg.MODEL.CENTERNET.HIP_PRECISION, torch.device("cuda:0"), seed=3, calibrate=False)[0]

        @classmethod
        def build_train_loader(cls, cfg):
            return itertools.cycle(batches)

        def build_hooks(self):
            ret = [h for h in super().build_hooks() if not isinstance(h, hooks.EvalHook)]
            if seen is not None:
                at = next(i for i, h in enumerate(ret) if isinstance(h, hooks.PreciseBN))
                ret.insert(at, hooks.CallbackHook(after_step=lambda tr: seen.append(_stats(get_bn_modules(tr.model)))))
            return ret
    return Cycle


def _train_batches():
    from test_trainer_gpu import _records as records
    return [records(2, 128), records(2, 128, first=2)]


def _hook_types(trainer):
    return [type(h).__name__ for h in trainer._hooks]


def test_trainer_checkpoint_carries_the_precise_statistics(tmp_path, dev, clean_logger):  # noqa: F811
    from test_trainer_gpu import _cfg
    from detectron2_centernet_amd.data.catalog import register_synthetic
    from detectron2_centernet_amd.engine.precise_bn import get_bn_modules, update_bn_stats

    register_synthetic("bulb_train")
    out = tmp_path / "out"
    cfg = _cfg(tmp_path, out, "TEST.PRECISE_BN.ENABLED", True, "TEST.PRECISE_BN.NUM_ITER", 2, "SOLVER.MAX_ITER", 2)
    batches = _train_batches()
    trainer = _cycle_trainer(batches)(cfg)
    names = _hook_types(trainer)
    assert names == ["IterationTimer", "LRScheduler", "PreciseBN", "PeriodicCheckpointer", "PeriodicWriter"]
    trainer.train()
    torch.cuda.synchronize()
    final = torch.load(out / "model_final.pth", weights_only=False)
    # a manual replay: the final weights, the same two batches
    fresh = type(trainer).build_model(cfg)
    fresh.load_state_dict(final["model"])
    fresh.train()
    tracked = {k: int(v) for k, v in final["model"].items() if k.endswith("num_batches_tracked")}
    assert set(tracked.values()) == {4}                          # two training steps, two PreciseBN batches
    for m in get_bn_modules(fresh):                              # the replay must not depend on what it overwrites
        m.running_mean.fill_(5.0)
        m.running_var.fill_(7.0)
    update_bn_stats(fresh, batches, 2)
    torch.cuda.synchronize()
    for k, v in fresh.state_dict().items():
        if "running_" in k:
            assert torch.equal(v.cpu(), final["model"][k].cpu()), k
    # and the model the trainer holds is the one it saved
    for k, v in trainer.model.state_dict().items():
        assert torch.equal(v.cpu(), final["model"][k].cpu()), k


def test_trainer_with_ema_measures_the_averaged_weights(tmp_path, dev, clean_logger):  # noqa: F811
    from test_trainer_gpu import _cfg
    from detectron2_centernet_amd.data.catalog import register_synthetic
    from detectron2_centernet_amd.engine.precise_bn import get_bn_modules, update_bn_stats
    from detectron2_centernet_amd.solver import ModelEMA

    register_synthetic("bulb_train")
    out = tmp_path / "out"
    cfg = _cfg(tmp_path, out, "TEST.PRECISE_BN.ENABLED", True, "TEST.PRECISE_BN.NUM_ITER", 2, "SOLVER.MAX_ITER", 2,
               "SOLVER.EMA.ENABLED", True, "SOLVER.WARMUP_FACTOR", 0.1)
    assert cfg.SOLVER.EMA.EVAL is True
    batches, seen = _train_batches(), []
    trainer = _cycle_trainer(batches, seen)(cfg)
    trainer.resume_or_load(resume=False)
    assert _hook_types(trainer) == ["IterationTimer", "LRScheduler", "CallbackHook", "PreciseBN", "PeriodicCheckpointer",
                                    "PeriodicWriter"]
    trainer.train()
    torch.cuda.synchronize()
    final = torch.load(out / "model_final.pth", weights_only=False)
    mods = get_bn_modules(trainer.model)
    names = {id(m): n for n, m in trainer.model.named_modules()}
    # the live statistics are what training left: those of the moment before the hook ran, in the model and in the file
    live_mean, live_var = _stats(mods)
    assert np.array_equal(live_mean, seen[-1][0]) and np.array_equal(live_var, seen[-1][1])
    file_mean = torch.cat([final["model"][names[id(m)] + ".running_mean"].reshape(-1) for m in mods]).cpu().numpy()
    assert np.array_equal(file_mean, live_mean)
    # "ema" holds the precise statistics of the averaged weights: a fresh model with the file's averaged weights, replayed
    fresh = type(trainer).build_model(cfg)
    ModelEMA.load_into_model(fresh, final["ema"])
    fresh.train()
    for m in get_bn_modules(fresh):
        m.running_mean.fill_(5.0)
        m.running_var.fill_(7.0)
    update_bn_stats(fresh, batches, 2)
    torch.cuda.synchronize()
    sd = fresh.state_dict()
    differ = 0
    for k, v in final["ema"]["buffers"].items():
        assert torch.equal(sd[k].cpu(), v), k
        differ += not torch.equal(v, final["model"][k].cpu())
    assert differ == len(final["ema"]["buffers"]) == 2 * len(mods)


def test_trainer_without_the_key_has_the_parents_hooks(tmp_path, dev, clean_logger):  # noqa: F811
    from test_trainer_gpu import _cfg
    from detectron2_centernet_amd.data.catalog import register_synthetic
    from detectron2_centernet_amd.engine import DefaultTrainer

    register_synthetic("bulb_train")
    cfg = _cfg(tmp_path, tmp_path / "out", "SOLVER.MAX_ITER", 1)
    assert cfg.TEST.PRECISE_BN.ENABLED is False

    class Fixed(DefaultTrainer):
        @classmethod
        def build_train_loader(cls, cfg):
            return itertools.cycle(_train_batches())

    trainer = Fixed(cfg)
    assert _hook_types(trainer) == ["IterationTimer", "LRScheduler", "PeriodicCheckpointer", "EvalHook", "PeriodicWriter"]


# ------------------------------------------------------------------------------------------------------------------------
# 4. two ranks on one device
# ------------------------------------------------------------------------------------------------------------------------
def _rank_batches(rank):
    """every rank feeds other batches, of other sizes"""
    return [_records(2, 64, 64, 10 + rank), _records(1 + rank, 64, 96 - 32 * rank, 20 + rank)]


def _two_rank_worker(outdir, kind):
    import torch.distributed as dist
    from detectron2_centernet_amd.engine.precise_bn import get_bn_modules, update_bn_stats

    torch.cuda.set_device(0)
    rank = dist.get_rank()
    if kind == "dla34":
        from test_model_gpu import make_model
        model = make_model(_Path(os.path.join(outdir, f"cfg{rank}")), "f32", seed=8, calibrated=False)[0].train()
    else:
        from test_syncbn_gpu import _bot_model
        d = os.path.join(outdir, f"cfg{rank}")
        os.makedirs(d, exist_ok=True)
        model = _bot_model(d, "f32")[0]
    mods = get_bn_modules(model)
    batches = _rank_batches(rank)
    own = [_own_batch_stats(model, mods, b) for b in batches]         # collective forwards where the model has SyncBN
    update_bn_stats(model, batches, 2)
    mean, var = _stats(mods)
    tracked = sorted({int(m.num_batches_tracked) for m in mods})
    torch.save({"own": own, "mean": mean, "var": var, "numels": [m.running_mean.numel() for m in mods], "tracked": tracked},
               os.path.join(outdir, f"rank{rank}.pt"))


def _Path(p):
    import pathlib
    path = pathlib.Path(p)
    path.mkdir(parents=True, exist_ok=True)
    return path


@pytest.mark.parametrize("kind", ["dla34", "res_18_bot"])
def test_two_ranks_hold_bit_equal_statistics(dev, tmp_path, kind):
    """both ranks end with the same bits; they are the restatement of what each rank's own momentum-1 forwards left (a SyncBN
    layer's statistics are global already: its rows are the ranks' sum and both ranks merge the same triple, d = 0).  DLA-34
    (no SyncBN): also the single-process result over the union of the four batches, within the bound"""
    from detectron2_centernet_amd.engine import launch
    from detectron2_centernet_amd.engine.precise_bn import get_bn_modules, update_bn_stats

    launch(_two_rank_worker, 2, num_machines=1, machine_rank=0, dist_url="auto", args=(str(tmp_path), kind), backend="gloo")
    r0, r1 = (torch.load(tmp_path / f"rank{r}.pt", weights_only=False) for r in range(2))
    for k in ("mean", "var"):
        assert np.array_equal(r0[k].view(np.uint32), r1[k].view(np.uint32)), k
    assert r0["tracked"] == r1["tracked"] == [2] and r0["numels"] == r1["numels"]
    synced = r0["own"][0][3]
    assert any(synced) == (kind == "res_18_bot") and synced == r1["own"][0][3]
    per_rank = []
    for mine, other in ((r0, r1), (r1, r0)):
        per_rank.append([(a[0], a[1], [ra + rb if s else ra for ra, rb, s in zip(a[2], b[2], synced)])
                         for a, b in zip(mine["own"], other["own"])])
    for i, s in enumerate(synced):      # what a SyncBN layer leaves is the same on both ranks
        if s:
            a = int(np.sum(r0["numels"][:i]))
            sl = slice(a, a + r0["numels"][i])
            assert all(np.array_equal(x[0][sl], y[0][sl]) and np.array_equal(x[1][sl], y[1][sl])
                       for x, y in zip(r0["own"], r1["own"]))
    acc = _restate(per_rank, r0["numels"])
    assert _check_finish((r0["mean"], r0["var"]), acc, f"{kind}, two ranks").all()
    if kind != "dla34":
        return
    from test_model_gpu import make_model
    model = make_model(_Path(tmp_path / "single"), "f32", seed=8, calibrated=False)[0].train()
    update_bn_stats(model, _rank_batches(0) + _rank_batches(1), 4)
    one = _restate([per_rank[0] + per_rank[1]], r0["numels"])
    got = _stats(get_bn_modules(model))
    _check_finish(got, one, "DLA-34, the union in one process")
    # both within their bounds of the same exact value, the bounds of two merge orders
    (mu, v), (emu, ev), _ = acc.outputs()
    (_, _), (emu1, ev1), _ = one.outputs()
    assert PC.ratio(got[0], r0["mean"], 2 * (emu + emu1 + PC.f32_part(np.abs(mu) + emu + emu1))) <= 1.0
    assert PC.ratio(got[1], r0["var"], 2 * (ev + ev1 + PC.f32_part(v + ev + ev1))) <= 1.0
