"""SOLVER.EMA on the GPU: the three kernels of csrc/ema.hip against the float64 oracle and bound of tests/ema_cases.py, ModelEMA
behind eager, captured and two-rank steps, the in-place exchange of `swapped()`, and DefaultTrainer with the EMA on and off."""
import ctypes
import os

import numpy as np
import pytest
import torch

import ema_cases as EC
from test_trainer_gpu import clean_logger  # noqa: F401 -- DefaultTrainer sets the package logger up for the whole process

pytestmark = pytest.mark.gpu

W_FIRST = EC.weight_at(0)                      # 0.9: the first update under warm-up
W_LATE = EC.weight_at(10 ** 6)                 # f32(1 - 0.9998)


# ------------------------------------------------------------------------------------------------------------------------
# 1. the kernels
# ------------------------------------------------------------------------------------------------------------------------
class Device:
    """a SegTable's buffers on the device: the live buffer, the EMA buffer with its guards, and the two tables"""

    def __init__(self, table, live, ema, dev):
        self.table = table
        self.live, self.ema_full = torch.from_numpy(live).to(dev), torch.from_numpy(ema).to(dev)
        self.ema = self.ema_full[EC.GUARD:EC.GUARD + table.total]
        assert self.live.data_ptr() % 16 == 0 and self.ema.data_ptr() % 16 == 0
        self.ptrs = torch.tensor([self.live.data_ptr() + 4 * off for off in table.live_off], dtype=torch.int64, device=dev)
        self.starts = torch.tensor(table.starts, dtype=torch.int64, device=dev)

    def host(self):
        torch.cuda.synchronize()
        return self.live.cpu().numpy(), self.ema_full.cpu().numpy()


def _weight(w, dev):
    return torch.tensor([w], dtype=torch.float32, device=dev)


@pytest.fixture(scope="module")
def table_inputs():
    """every table's inputs, generated once and left unchanged"""
    return {t.name: t.inputs(seed=100 + i) for i, t in enumerate(EC.TABLES)}


@pytest.mark.parametrize("w", [W_FIRST, W_LATE], ids=["w0.9", "w2e-4"])
@pytest.mark.parametrize("table", EC.TABLES, ids=lambda t: t.name)
def test_lerp_against_the_oracle(dev, table, w, table_inputs):
    from detectron2_centernet_amd import ops

    live0, ema0 = table_inputs[table.name]
    d = Device(table, live0, ema0, dev)
    ops.ema_lerp_segments_(d.ptrs, d.ema, d.starts, table.max_len, _weight(w, dev))
    live, ema = d.host()
    assert np.array_equal(live.view(np.uint32), live0.view(np.uint32))                # p is read only, its sentinels too
    body = slice(EC.GUARD, EC.GUARD + table.total)
    assert (ema[:EC.GUARD] == EC.SENTINEL).all() and (ema[body.stop:] == EC.SENTINEL).all()
    x, q = EC.lerp64(ema0[body], table.gather(live0), w)
    r = EC.ratio(ema[body], x, EC.step_bound(x, q, w))
    print(f"{table.name}, w = {w:.4g}: {table.total} elements in {len(table.lens)} segments, worst error / bound {r:.3f}")
    assert r <= 1.0
    if table.total:
        assert not np.array_equal(ema[body], ema0[body])


@pytest.mark.parametrize("table", [EC.PACKED, EC.ALIGNED, EC.LOOPS], ids=lambda t: t.name)
def test_equal_values_come_back_bit_for_bit(dev, table, table_inputs):
    from detectron2_centernet_amd import ops

    live0, ema0 = table_inputs[table.name]
    ema0 = ema0.copy()
    ema0[EC.GUARD:EC.GUARD + table.total] = table.gather(live0)
    d = Device(table, live0, ema0, dev)
    ops.ema_lerp_segments_(d.ptrs, d.ema, d.starts, table.max_len, _weight(W_FIRST, dev))
    assert np.array_equal(d.host()[1].view(np.uint32), ema0.view(np.uint32))


def test_non_finite_values_follow_the_formula(dev):
    from detectron2_centernet_amd import ops

    table = EC.NONFINITE_TABLE
    live0, ema0 = table.inputs(seed=7)
    for i, p, e in EC.NONFINITE:
        live0[table.live_off[0] + i], ema0[EC.GUARD + i] = p, e
    d = Device(table, live0, ema0, dev)
    ops.ema_lerp_segments_(d.ptrs, d.ema, d.starts, table.max_len, _weight(W_LATE, dev))
    ema = d.host()[1][EC.GUARD:EC.GUARD + table.total]
    x, q = EC.lerp64(ema0[EC.GUARD:EC.GUARD + table.total], table.gather(live0), W_LATE)
    assert np.isnan(x).sum() == 7 and np.isinf(x).sum() == 2              # the cases are what they claim to be
    assert EC.ratio(ema, x, EC.step_bound(x, q, W_LATE)) <= 1.0           # NaN and Inf in place, the neighbours in bound


def test_advance_counts_and_follows_the_schedule(dev):
    from detectron2_centernet_amd import ops

    updates, weight = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.float32, device=dev)
    for warmup, decay in ((True, EC.DECAY), (False, EC.DECAY), (True, 0.5), (True, 0.0)):
        cross = EC.crossover(decay) if decay > 0.1 else 0
        for t0 in (0, 7, max(cross - 2, 0), 2 ** 40):
            updates.fill_(t0)
            for t in range(t0, t0 + 4):
                ops.ema_advance_(updates, weight, decay, warmup)
                assert int(updates) == t + 1
                assert float(weight) == EC.weight_at(t, decay, warmup), (t, decay, warmup)
    updates.zero_()
    ops.ema_advance_(updates, weight, EC.DECAY, True)
    assert float(weight) == float(np.float32(0.9)) and int(updates) == 1


_SWAP_BITS = [0x7FC12345, 0xFF800001, 0x80000000, 0x00000001, 0x7F800000, 0xFFFFFFFF]   # NaN payloads (quiet, signalling), -0,
                                                                                          # a subnormal, Inf, all ones


@pytest.mark.parametrize("table", EC.TABLES, ids=lambda t: t.name)
def test_swap_exchanges_bits_and_twice_is_the_identity(dev, table, table_inputs):
    from detectron2_centernet_amd import ops

    live0, ema0 = (a.copy() for a in table_inputs[table.name])
    lv, ev = live0.view(np.uint32), ema0.view(np.uint32)
    for k, bits in enumerate(_SWAP_BITS):              # special bit patterns on both sides, first and last elements included
        for s, n in enumerate(table.lens):
            if n > k:
                lv[table.live_off[s] + k] = bits
                ev[EC.GUARD + table.starts[s] + n - 1 - k] = bits
    d = Device(table, live0, ema0, dev)
    ops.ema_swap_segments_(d.ptrs, d.ema, d.starts, table.max_len)
    live, ema = d.host()
    body = slice(EC.GUARD, EC.GUARD + table.total)
    mask = table.live_mask()
    assert np.array_equal(ema.view(np.uint32)[body], table.gather(live0).view(np.uint32))
    assert np.array_equal(table.gather(live).view(np.uint32), ev[body])
    assert (live[~mask] == EC.SENTINEL).all() and (ema[:EC.GUARD] == EC.SENTINEL).all() and (ema[body.stop:] == EC.SENTINEL).all()
    ops.ema_swap_segments_(d.ptrs, d.ema, d.starts, table.max_len)
    live, ema = d.host()
    assert np.array_equal(live.view(np.uint32), lv) and np.array_equal(ema.view(np.uint32), ev)


def test_no_segments_is_a_no_op(dev):
    from detectron2_centernet_amd import ops

    ema = torch.full((16,), EC.SENTINEL, device=dev)
    none, start = torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    ops.ema_lerp_segments_(none, ema, start, 0, _weight(0.5, dev))
    ops.ema_swap_segments_(none, ema, start, 0)
    torch.cuda.synchronize()
    assert (ema == EC.SENTINEL).all()


def test_entry_points_refuse_bad_arguments(dev):
    from detectron2_centernet_amd import _lib

    lib = _lib.lib()
    live, ema = torch.ones(8, device=dev), torch.zeros(8, device=dev)
    ptrs = torch.tensor([live.data_ptr()], dtype=torch.int64, device=dev)
    starts = torch.tensor([0, 8], dtype=torch.int64, device=dev)
    updates, weight = torch.zeros(1, dtype=torch.int64, device=dev), torch.full((1,), 0.5, device=dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())       # noqa: E731
    null = ctypes.c_void_p(0)

    def refused(rc, words):
        assert rc == -22 and words in lib.ctdet_last_error().decode(), (rc, lib.ctdet_last_error())

    good = [P(ptrs), P(ema), P(starts), 1, 8, P(weight), None]
    for i in (0, 1, 2, 5):
        refused(lib.ctdet_ema_lerp_segments(*(good[:i] + [null] + good[i + 1:])), "null pointer")
    refused(lib.ctdet_ema_lerp_segments(*(good[:3] + [-1] + good[4:])), "nseg=-1")
    refused(lib.ctdet_ema_lerp_segments(*(good[:4] + [-1] + good[5:])), "max_len=-1")
    good = [P(ptrs), P(ema), P(starts), 1, 8, None]
    for i in (0, 1, 2):
        refused(lib.ctdet_ema_swap_segments(*(good[:i] + [null] + good[i + 1:])), "null pointer")
    refused(lib.ctdet_ema_swap_segments(*(good[:3] + [-1] + good[4:])), "nseg=-1")
    refused(lib.ctdet_ema_swap_segments(*(good[:4] + [-1] + good[5:])), "max_len=-1")
    refused(lib.ctdet_ema_advance(null, P(weight), 0.5, 1, None), "null pointer")
    refused(lib.ctdet_ema_advance(P(updates), null, 0.5, 1, None), "null pointer")
    for decay in (1.0, -1e-9, 2.0, float("nan")):
        refused(lib.ctdet_ema_advance(P(updates), P(weight), decay, 1, None), "outside [0, 1)")
    # nseg == 0 returns 0 before anything is looked at
    assert lib.ctdet_ema_lerp_segments(null, null, null, 0, 0, null, None) == 0
    assert lib.ctdet_ema_swap_segments(null, null, null, 0, 0, None) == 0
    torch.cuda.synchronize()
    assert int(updates) == 0 and float(weight) == 0.5 and (ema == 0).all() and (live == 1).all()     # a refusal launches nothing


# ------------------------------------------------------------------------------------------------------------------------
# 2. ModelEMA on a small net
# ------------------------------------------------------------------------------------------------------------------------
def _small(dev, kind):
    """tests/test_adam_gpu.py's small net with a BatchNorm of 5 channels behind it: statistics segments of 8 and 5 elements,
    the second kind padded to the float4 boundary"""
    from test_adam_gpu import small_net
    from detectron2_centernet_amd.solver import FlatAdam, FlatSGD, ModelEMA

    net = torch.nn.Sequential(*small_net(dev), torch.nn.BatchNorm2d(5).to(dev))
    groups = [(p, 1.0, 0.0) for p in net.parameters()]
    opt = FlatSGD(groups, 0.05, 0.9) if kind == "sgd" else FlatAdam(groups, 0.01)
    ema = ModelEMA(net, opt, decay=EC.DECAY, warmup=True)
    opt.ema = ema
    return net, opt, ema


def _stats(ema):
    """(live statistics, averaged statistics), both in the order of the table, on the host"""
    live = torch.cat([b.detach().reshape(-1) for _, b in ema.table.buffers_live])
    avg = torch.cat([ema.ema_stats[off:off + n] for _, off, n, _ in ema.table.buffers])
    return live.cpu().numpy(), avg.cpu().numpy()


def _check_chains(ema, chains, what):
    torch.cuda.synchronize()
    got = (ema.ema_param.cpu().numpy(), _stats(ema)[1])
    for name, g, c in zip(("parameters", "statistics"), got, chains):
        r = EC.ratio(g, c.e, c.bound)
        print(f"{what}, {name}: worst error / running bound {r:.3f} after {c.t} updates")
        assert r <= 1.0, (what, name, r)


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_eager_steps_follow_the_recurrence(dev, kind):
    net, opt, ema = _small(dev, kind)
    assert [n for n, _, _, _ in ema.table.buffers] == ["1.running_mean", "1.running_var", "3.running_mean", "3.running_var"]
    assert [off for _, off, _, _ in ema.table.buffers] == [0, 8, 16, 24] and ema.ema_stats.numel() == 32
    assert ema._stat_ptrs.numel() == 6                       # the two 5-element buffers have a padding segment behind them
    assert torch.equal(ema.ema_param, opt.flat_param) and int(ema.updates) == 0
    chains = (EC.Chain(opt.flat_param.cpu().numpy()), EC.Chain(_stats(ema)[0]))
    g = torch.Generator().manual_seed(5)
    for step in range(6):
        x = torch.randn(4, 3, 9, 9, generator=g).to(dev) * (1.0 + step)
        opt.zero_grad()
        net(x).square().mean().backward()
        opt.step()
        torch.cuda.synchronize()
        chains[0].update(opt.flat_param.cpu().numpy())
        chains[1].update(_stats(ema)[0])
        assert int(ema.updates) == step + 1 and float(ema.weight) == EC.weight_at(step)
        _check_chains(ema, chains, f"{kind} eager step {step}")
    assert not torch.equal(ema.ema_param, opt.flat_param)
    assert int(net[1].num_batches_tracked) == 6              # stays live, is not averaged


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_captured_step_holds_kernels_only_and_keeps_counting(dev, kind):
    """`optimizer.step()` with the EMA behind it, captured alone: kernels only, three more of them than without the EMA;
    five replays on five gradients and five sets of statistics follow the recurrence, the count advancing on the device"""
    from detectron2_centernet_amd.engine import graph_nodes

    def capture(o):
        graph = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(graph):
            o.step()
        nodes = graph_nodes.inspect(graph, "optimizer step")
        graph.instantiate()
        return graph, nodes

    net, opt, ema = _small(dev, kind)
    g = torch.Generator().manual_seed(6)
    n = opt.flat_grad.numel()
    opt.flat_grad.copy_(torch.randn(n, generator=g).to(dev))
    opt.ema = None
    opt.step()                                                # the first step, and the plain node count
    torch.cuda.synchronize()
    _, plain_nodes = capture(opt)
    opt.ema = ema
    ema.reset()
    chains = (EC.Chain(opt.flat_param.cpu().numpy()), EC.Chain(_stats(ema)[0]))
    graph, nodes = capture(opt)
    assert set(nodes) <= {"kernel", "empty"}, nodes
    assert nodes["kernel"] == plain_nodes["kernel"] + 3, (nodes, plain_nodes)
    assert int(ema.updates) == 0                              # the capture itself ran nothing
    with pytest.raises(RuntimeError, match="stream capture"):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            ema.weight.mul_(1.0)                              # (a capture with one kernel in it)
            with ema.swapped():
                pass
    for k in range(5):
        opt.flat_grad.copy_(torch.randn(n, generator=g).to(dev))
        for _, b in ema.table.buffers_live:                   # what a training forward would have written
            b.copy_(torch.rand(b.shape, generator=g).to(dev) + 0.5 * k)
        graph.replay()
        torch.cuda.synchronize()
        chains[0].update(opt.flat_param.cpu().numpy())
        chains[1].update(_stats(ema)[0])
        assert int(ema.updates) == k + 1 and float(ema.weight) == EC.weight_at(k)
        _check_chains(ema, chains, f"{kind} replay {k}")


def test_state_dict_reset_and_model_state_dict(dev):
    net, opt, ema = _small(dev, "sgd")
    g = torch.Generator().manual_seed(8)
    for _ in range(2):
        opt.flat_grad.copy_(torch.randn(opt.flat_grad.numel(), generator=g).to(dev))
        opt.step()
    sd = ema.state_dict()
    assert sd["updates"] == 2 and sd["decay"] == EC.DECAY and set(sd["params"]) == {n for n, _ in net.named_parameters()}
    full = ema.model_state_dict()
    assert set(full) == set(net.state_dict())
    assert torch.equal(full["0.weight"], sd["params"]["0.weight"]) and not torch.equal(full["0.weight"], net[0].weight.cpu())
    assert torch.equal(full["1.num_batches_tracked"], net[1].num_batches_tracked.cpu())
    net2, opt2, ema2 = _small(dev, "sgd")
    ema2.load_state_dict(sd)
    assert torch.equal(ema2.ema_param, ema.ema_param) and torch.equal(ema2.ema_stats, ema.ema_stats) and int(ema2.updates) == 2
    ema2.reset()
    assert torch.equal(ema2.ema_param, opt2.flat_param) and int(ema2.updates) == 0
    with pytest.raises(KeyError, match="2.weight"):
        ema2.load_state_dict({"params": {k: v for k, v in sd["params"].items() if k != "2.weight"}, "buffers": sd["buffers"],
                              "updates": 1})


# ------------------------------------------------------------------------------------------------------------------------
# 3. the trainer's captured step, and swapped()
# ------------------------------------------------------------------------------------------------------------------------
def _ema_trainer(tmp_path, precision, dev):
    from test_model_gpu import make_model
    from detectron2_centernet_amd.engine.bench_train import synthetic_batch
    from detectron2_centernet_amd.engine.train_loop import SimpleTrainer

    model, cfg = make_model(tmp_path, precision, seed=12, calibrated=False)
    cfg.SOLVER.IMS_PER_BATCH = 2
    cfg.SOLVER.EMA.ENABLED = True
    tr = SimpleTrainer(model, None, cfg)
    return tr, synthetic_batch(2, 128, 0, dev)


def test_trainer_captured_step_updates_the_ema(dev, tmp_path):
    """six steps of SimpleTrainer (two eager, the capture, three replays): after each, the EMA equals the f64 recurrence over
    snapshots of flat_param and of the BatchNorm statistics; the captured step holds kernels only"""
    tr, batch = _ema_trainer(tmp_path, "f16x3", dev)
    ema, opt = tr.ema, tr.optimizer
    assert ema is not None and opt.ema is ema and len(ema.table.buffers) > 50
    chains = (EC.Chain(opt.flat_param.cpu().numpy()), EC.Chain(_stats(ema)[0]))
    for step in range(6):
        tr.run_step_tensors(*batch)
        torch.cuda.synchronize()
        chains[0].update(opt.flat_param.cpu().numpy())
        chains[1].update(_stats(ema)[0])
        assert int(ema.updates) == step + 1
        _check_chains(ema, chains, f"trainer step {step} ({tr.graph_state})")
    assert tr.graph_state == "captured"
    nodes = next(g["nodes"] for g in tr._graphs.values() if g["graph"] is not None)
    assert set(nodes) <= {"kernel", "empty"}, nodes


def _packed(opt):
    """clones of every packed operand (and row scale) the captured step reads"""
    out = []
    for e in opt._packs.entries.values():
        out.append(e[1].clone())
        if e[4] is not None:
            out.append(e[4].clone())
    return out


def _loss(tr, batch):
    with torch.no_grad():
        losses = tr.model.train_batch_tensor(*batch)
    torch.cuda.synchronize()
    return torch.stack([losses[k].float().reshape(()) for k in sorted(losses)]).cpu()


@pytest.mark.parametrize("precision", ["f16x3", "f16"])
def test_swapped_exchanges_in_place_and_repacks(dev, tmp_path, precision):
    tr, batch = _ema_trainer(tmp_path, precision, dev)
    ema, opt = tr.ema, tr.optimizer
    for _ in range(4):
        tr.run_step_tensors(*batch)
    # four warm-up steps at a thousandth of the learning rate move the weights by less than an f16 ulp: the averaged side is
    # pushed away by hand, so that every packed operand and the losses must differ inside the block
    ema.ema_param.mul_(1.01)
    ema.ema_stats.mul_(1.05)
    torch.cuda.synchronize()
    assert tr.graph_state == "captured" and len(opt._packs.entries) > 50
    bits = lambda t: t.detach().clone().view(torch.int32)      # noqa: E731
    live_p, avg_p = bits(opt.flat_param), bits(ema.ema_param)
    live_s = [bits(b) for _, b in ema.table.buffers_live]
    avg_s = bits(ema.ema_stats)
    assert not torch.equal(live_p, avg_p)
    address = opt.flat_param.data_ptr(), [b.data_ptr() for _, b in ema.table.buffers_live]
    packed_before = _packed(opt)

    def restored():
        torch.cuda.synchronize()
        assert torch.equal(bits(opt.flat_param), live_p) and torch.equal(bits(ema.ema_param), avg_p)
        assert all(torch.equal(bits(b), s) for (_, b), s in zip(ema.table.buffers_live, live_s))
        assert torch.equal(bits(ema.ema_stats), avg_s)
        assert all(torch.equal(a, b) for a, b in zip(_packed(opt), packed_before))       # the re-pack behind the exchange back

    with ema.swapped():
        torch.cuda.synchronize()
        assert torch.equal(bits(opt.flat_param), avg_p) and torch.equal(bits(ema.ema_param), live_p)
        for (name, b), (_, off, n, _), s in zip(ema.table.buffers_live, ema.table.buffers, live_s):
            assert torch.equal(bits(b).reshape(-1), avg_s[off:off + n]), name              # the module holds the averaged stats
            assert torch.equal(bits(ema.ema_stats[off:off + n]), s.reshape(-1)), name
        inside = _packed(opt)
        assert sum(not torch.equal(a, b) for a, b in zip(inside, packed_before)) > len(inside) // 2
        assert (opt.flat_param.data_ptr(), [b.data_ptr() for _, b in ema.table.buffers_live]) == address
    restored()
    with pytest.raises(ZeroDivisionError):          # an exception inside the block still swaps back
        with ema.swapped():
            1 / 0
    restored()
    # the training forward on the fixed batch: the same losses before and after, others inside.  (Its BatchNorm layers write
    # their running statistics, which the losses of a training forward do not read; the bit checks above ran without it.)
    before = _loss(tr, batch)
    again = _loss(tr, batch)
    with ema.swapped():
        within = _loss(tr, batch)
    after = _loss(tr, batch)
    print(f"{precision}: losses before {before.tolist()}, inside {within.tolist()}, after {after.tolist()}")
    assert torch.equal(before, again), "the training forward is not bit-reproducible: compare the packed operands only"
    assert torch.equal(before, after) and not torch.equal(before, within)
    tr.run_step_tensors(*batch)                     # training goes on, on the captured step
    torch.cuda.synchronize()
    assert tr.graph_state == "captured" and int(ema.updates) == 5


# ------------------------------------------------------------------------------------------------------------------------
# 4. two ranks on one device
# ------------------------------------------------------------------------------------------------------------------------
def _dp_worker(outdir, nsteps=3):
    import bench
    from detectron2_centernet_amd.engine.bench_train import synthetic_batch
    from detectron2_centernet_amd.engine.train_loop import SimpleTrainer
    from detectron2_centernet_amd.utils import comm

    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    model, cfg = bench.build_model("f16x3", dev, seed=5 + comm.get_rank(), calibrate=False)     # the broadcast evens it out
    model.train()
    cfg.SOLVER.EMA.ENABLED = True
    tr = SimpleTrainer(model, None, cfg)
    cfg.SOLVER.IMS_PER_BATCH = 2 * tr.reducer.world
    batch = synthetic_batch(2, 128, 0, dev)        # rank argument fixed: identical data on every rank
    ema, rec = tr.ema, []
    start_equal = bool(torch.equal(ema.ema_param, tr.optimizer.flat_param))
    for _ in range(nsteps):
        tr.run_step_tensors(*batch)
        rec.append([ema.ema_param.clone(), ema.ema_stats.clone(), ema.updates.clone(), tr.optimizer.flat_param.clone()])
    torch.cuda.synchronize()
    torch.save({"world": tr.reducer.world, "graph_state": tr.graph_state, "start_equal": start_equal,
                "steps": [[t.cpu() for t in r] for r in rec]}, os.path.join(outdir, f"rank{comm.get_rank()}.pt"))


def test_two_ranks_keep_bit_equal_averages(dev, tmp_path):
    from detectron2_centernet_amd.engine import launch

    os.environ["CTDET_TRAIN_GRAPH"] = "1"
    try:
        launch(_dp_worker, 2, num_machines=1, machine_rank=0, dist_url="auto", args=(str(tmp_path),), backend="gloo")
    finally:
        os.environ.pop("CTDET_TRAIN_GRAPH", None)
    r0, r1 = torch.load(tmp_path / "rank0.pt"), torch.load(tmp_path / "rank1.pt")
    assert r0["world"] == r1["world"] == 2 and r0["graph_state"] == r1["graph_state"] == "captured"
    assert r0["start_equal"] and r1["start_equal"]             # built behind the broadcast of rank 0's weights
    for step, (a, b) in enumerate(zip(r0["steps"], r1["steps"])):
        for x, y in zip(a, b):
            assert torch.equal(x, y), step
        assert int(a[2]) == step + 1 and torch.isfinite(a[0]).all() and not torch.equal(a[0], a[3])


# ------------------------------------------------------------------------------------------------------------------------
# 5. DefaultTrainer
# ------------------------------------------------------------------------------------------------------------------------
def _recording_trainer(seen):
    """DefaultTrainer whose `test` records the bits of the parameters it is handed"""
    from detectron2_centernet_amd.engine import DefaultTrainer

    class Recording(DefaultTrainer):
        @classmethod
        def test(cls, cfg, model, evaluators=None):
            seen.append({n: p.detach().cpu().clone() for n, p in model.named_parameters()})
            return super().test(cfg, model, evaluators)
    return Recording


def test_default_trainer_evaluates_saves_and_restores_the_ema(tmp_path, dev, clean_logger):  # noqa: F811
    from test_trainer_gpu import _cfg
    from detectron2_centernet_amd.data.catalog import register_synthetic_files
    from detectron2_centernet_amd.engine import DefaultTrainer
    from detectron2_centernet_amd.solver import ModelEMA

    out = tmp_path / "out"
    for name in ("bulb_train", "bulb_val"):
        register_synthetic_files(name, str(out / "synthetic"), length=8, size=128, replace=True)
    # WARMUP_FACTOR 0.1: steps large enough that most averaged parameters differ from the live ones in their f32 bits
    on = ("SOLVER.EMA.ENABLED", True, "SOLVER.MAX_ITER", 6, "SOLVER.CHECKPOINT_PERIOD", 3, "TEST.EVAL_PERIOD", 3,
          "SOLVER.WARMUP_FACTOR", 0.1)
    cfg = _cfg(tmp_path, out, *on)
    seen = []
    torch.manual_seed(3)
    trainer = _recording_trainer(seen)(cfg)
    trainer.model.wh[-1].bias.data.fill_(6.0)       # boxes of non-degenerate size (tests/test_trainer_gpu.py)
    trainer.resume_or_load(resume=False)            # no weights: the EMA restarts from the model as it stands now
    ema = trainer.ema
    assert ema is not None and trainer.optimizer.ema is ema and trainer.checkpointer.checkpointables["ema"] is ema
    assert torch.equal(ema.ema_param, trainer.optimizer.flat_param) and int(ema.updates) == 0
    trainer.train()
    torch.cuda.synchronize()
    assert trainer.graph_state == "captured" and int(ema.updates) == 6 and len(seen) == 2
    final = torch.load(out / "model_final.pth", weights_only=False)
    assert final["iteration"] == 5 and set(final["ema"]) == {"params", "buffers", "updates", "decay"}
    assert final["ema"]["updates"] == 6 and final["ema"]["decay"] == 0.9998
    # the last evaluation (behind the checkpoint of the same iteration) saw the averaged weights, not the live ones
    differs = 0
    for name, t in final["ema"]["params"].items():
        assert torch.equal(seen[-1][name].view(torch.int32), t.view(torch.int32)), name
        differs += not torch.equal(t, final["model"][name])
    assert differs > len(final["ema"]["params"]) // 2
    # ... and the live ones are back under the model afterwards
    for name, p in trainer.model.named_parameters():
        assert torch.equal(p.detach().cpu(), final["model"][name]), name
    state = ema.state_dict()

    # a fresh model with the file's "ema" entry scores what the trainer's evaluation scored
    fresh = DefaultTrainer.build_model(cfg)
    ModelEMA.load_into_model(fresh, final["ema"])
    again = DefaultTrainer.test(cfg, fresh)
    want = trainer._last_eval_results["bbox"]
    for k, v in want.items():
        assert again["bbox"][k] == v or (v != v and again["bbox"][k] != again["bbox"][k]), (k, again["bbox"], want)

    # --resume: the EMA and its count come back bit for bit
    torch.manual_seed(4)
    resumed = DefaultTrainer(_cfg(tmp_path, out, *on))
    assert not torch.equal(resumed.ema.ema_param, ema.ema_param)
    resumed.resume_or_load(resume=True)
    assert resumed.start_iter == 6 and int(resumed.ema.updates) == 6
    back = resumed.ema.state_dict()
    for kind in ("params", "buffers"):
        assert set(back[kind]) == set(state[kind])
        for name, t in state[kind].items():
            assert torch.equal(back[kind][name].view(torch.int32), t.view(torch.int32)), name
    assert torch.equal(resumed.optimizer.flat_param, trainer.optimizer.flat_param)

    # MODEL.WEIGHTS without resume: the EMA restarts from the loaded weights
    torch.manual_seed(5)
    loaded = DefaultTrainer(_cfg(tmp_path, tmp_path / "other", *on, "MODEL.WEIGHTS", out / "model_final.pth"))
    loaded.resume_or_load(resume=False)
    assert loaded.start_iter == 0 and int(loaded.ema.updates) == 0
    assert torch.equal(loaded.ema.ema_param, loaded.optimizer.flat_param)
    assert torch.equal(loaded.optimizer.flat_param, trainer.optimizer.flat_param)
    live_stats, avg_stats = _stats(loaded.ema)
    assert np.array_equal(live_stats, avg_stats)


def test_default_trainer_without_ema_is_unchanged(tmp_path, dev, clean_logger):  # noqa: F811
    from test_trainer_gpu import _cfg, _fixed_batch_trainer, _records
    from detectron2_centernet_amd.data.catalog import register_synthetic

    register_synthetic("bulb_train")
    cfg = _cfg(tmp_path, tmp_path / "out", "SOLVER.MAX_ITER", 1)
    assert cfg.SOLVER.EMA.ENABLED is False
    trainer = _fixed_batch_trainer(_records(2, 128))(cfg)
    assert trainer.ema is None and trainer.optimizer.ema is None and "ema" not in trainer.checkpointer.checkpointables
    trainer.train()
    final = torch.load(tmp_path / "out" / "model_final.pth", weights_only=False)
    assert "ema" not in final and {"model", "optimizer", "scheduler", "iteration"} <= set(final)
