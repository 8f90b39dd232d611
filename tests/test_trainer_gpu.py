"""The training run on the GPU: the metric-push kernel at its edges, the ring against per-step read-backs, no synchronisation
between flushes, the non-finite check at the flush, record batches on the captured step, DefaultTrainer end to end (with
tools/train_net.py --eval-only in a child process), resume, and two ranks on the one GPU."""
import ctypes
import itertools
import json
import logging
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN_PAYLOAD = 0x7FC12345          # a quiet NaN with a payload
SNAN_PAYLOAD = 0xFF800001         # negative, signalling, smallest payload
SENTINEL = 0x5EA7BEEF


@pytest.fixture
def clean_logger():
    """setup_logger changes the package logger for the whole process: put it back, for the tests that run afterwards"""
    from detectron2_centernet_amd.utils import logger as L
    lg = logging.getLogger(L.ROOT_LOGGER)
    saved = (lg.handlers[:], lg.propagate, lg.level)
    yield
    lg.handlers[:], lg.propagate = saved[0], saved[1]
    lg.setLevel(saved[2])
    L.setup_logger.cache_clear()


def _bits(values, dev):
    """u32 bit patterns as one-element f32 device tensors (separate allocations, like a step's loss scalars); the copy to the
    device moves bytes, so a NaN keeps its payload"""
    return [torch.from_numpy(np.asarray([v], dtype=np.uint32).view(np.float32).copy()).to(dev) for v in values]


def _f32_bits(x):
    return int(np.asarray([x], dtype=np.float32).view(np.uint32)[0])


# ---------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("K", [1, 8])
def test_metric_push_kernel_edges(dev, K):
    """rows 62..72 of a 64-row ring (62..65: the wrap-around), K = 1 and 8, words copied bit for bit; NaN (with its payload),
    +inf and -inf each in the first, a middle and the last slot; neighbours and the tail of the row untouched; the first-bad
    word the smallest non-finite iteration whatever the push order"""
    from detectron2_centernet_amd import ops_train
    rows, rf = 64, K + 5                                   # three floats of every row are beyond K + 2: never written
    ring = torch.full((rows + 2, rf), SENTINEL, dtype=torch.int32, device=dev)      # a guard row on either side
    body = ring[1:rows + 1].view(torch.float32)
    first_bad = torch.tensor([ops_train.METRIC_NO_BAD_ITERATION], dtype=torch.int32, device=dev)
    finite = [_f32_bits(v) for v in (0.0, -0.0, 1.5, -3.25e-41, 3.4e38, 1e-30, 7.0, -2.5)]
    # iteration 62 is all finite; 63 .. 71 hold NaN (with a payload), +inf and -inf, each in the first, a middle and the last
    # slot (for K = 1 the three are one); 72 holds a signalling NaN in the first and the last slot at once.  62 .. 65 are the
    # rows on either side of the wrap-around of a 64-row ring
    specials = (NAN_PAYLOAD, _f32_bits(float("inf")), _f32_bits(float("-inf")))
    special = {62: {}, 72: {0: SNAN_PAYLOAD, K - 1: SNAN_PAYLOAD}}
    for v, word in enumerate(specials):
        for p, slot in enumerate((0, K // 2, K - 1)):
            special[63 + 3 * v + p] = {slot: word}
    pushed = {}
    for it in (65, 72, 62, 70, 64, 67, 71, 63, 69, 66, 68):     # not in order: the minimum must not depend on it
        words = [special[it].get(j, finite[(j + it) % 8]) for j in range(K)]
        pushed[it] = words
        ops_train.metric_push(_bits(words, dev), 0.25 * it, body, first_bad, it)
    torch.cuda.synchronize()
    host = ring.cpu().numpy().view(np.uint32)
    assert (host[0] == SENTINEL).all() and (host[rows + 1] == SENTINEL).all()
    for it, words in pushed.items():
        row = host[1 + it % rows]
        assert int(row[0]) == it and [int(w) for w in row[1:1 + K]] == words, (it, row)
        assert int(row[1 + K]) == _f32_bits(0.25 * it) and (row[K + 2:] == SENTINEL).all()
    untouched = [r for r in range(rows) if r not in {it % rows for it in pushed}]
    assert (host[1:rows + 1][untouched] == SENTINEL).all()
    assert int(first_bad.item()) == 63
    # a finite push later leaves the word alone; a smaller non-finite one lowers it
    ops_train.metric_push(_bits([finite[0]] * K, dev), 0.0, body, first_bad, 3)
    assert int(first_bad.item()) == 63
    ops_train.metric_push(_bits([NAN_PAYLOAD] * K, dev), 0.0, body, first_bad, 5)
    assert int(first_bad.item()) == 5


def test_metric_push_rejects_bad_arguments(dev):
    from detectron2_centernet_amd import _lib
    l, m = _lib.lib(), _lib.metrics_lib()
    ring = torch.zeros(64, 10, dtype=torch.float32, device=dev)
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    src = [torch.zeros(1, device=dev) for _ in range(9)]
    R, W = ring.data_ptr(), word.data_ptr()

    def call(n=3, K=3, ring=R, rows=64, rf=10, first_bad=W, it=0, null_at=None, table=True):
        ptrs = (ctypes.c_void_p * 9)(*[None if i == null_at else src[i].data_ptr() for i in range(9)])
        return m.ctdet_metric_push(ptrs if table else None, K, 0.0, ring, rows, rf, first_bad, it, None)

    assert call() == 0
    assert call(K=8, rf=10) == 0 and call(rows=1) == 0 and call(it=2 ** 31 - 1) == 0
    torch.cuda.synchronize()
    before = ring.view(torch.int32).clone()
    assert int(before[63, 0]) == 2 ** 31 - 1                  # the tag of the largest iteration, in row (2^31 - 1) % 64
    for kw, word_in_error in ((dict(K=0), b"K=0"), (dict(K=9, rf=16), b"K=9"), (dict(K=-1), b"K=-1"),
                              (dict(table=False), b"null"), (dict(ring=None), b"null"), (dict(first_bad=None), b"null"),
                              (dict(null_at=0), b"scalar 0"), (dict(null_at=2), b"scalar 2"),
                              (dict(rows=0), b"power of two"), (dict(rows=48), b"power of two"), (dict(rows=-64), b"power of two"),
                              (dict(rf=4), b"row_floats=4"), (dict(K=8, rf=9), b"row_floats=9"),
                              (dict(it=-1), b"iteration -1"), (dict(it=2 ** 31), b"iteration 2147483648")):
        rc = call(**kw)
        err = l.ctdet_last_error()
        assert rc == -22 and err.startswith(b"metric_push:") and word_in_error in err, (kw, rc, err)
    torch.cuda.synchronize()
    assert int(word.item()) == 0 and torch.equal(ring.view(torch.int32), before)        # a rejected call wrote nothing
    with _lib_label_dry_run(l):
        assert call() == 0 and l.ctdet_last_kernel_label() == b"metric_push_kernel"


class _lib_label_dry_run:
    def __init__(self, l):
        self.l = l

    def __enter__(self):
        self.l.ctdet_set_label_mode(2)

    def __exit__(self, *exc):
        self.l.ctdet_set_label_mode(0)
        return False


def test_metric_push_inside_and_outside_a_captured_graph(dev):
    """one ring, pushed by an eager launch, by a launch captured into a HIP graph and replayed, and eagerly again; a launch
    outside the graph is how the trainer serves eager and captured steps alike (the iteration is a kernel argument: a captured
    push would write the same row at every replay, which is what this shows)"""
    from detectron2_centernet_amd import ops_train
    ring = torch.full((64, 10), -1, dtype=torch.int32, device=dev).view(torch.float32)
    first_bad = torch.tensor([ops_train.METRIC_NO_BAD_ITERATION], dtype=torch.int32, device=dev)
    a, b = torch.tensor([1.25], device=dev), torch.tensor([-2.5], device=dev)
    ops_train.metric_push([a, b], 0.5, ring, first_bad, 0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        a.mul_(2.0)                                                        # the "step": its scalars change at every replay
        ops_train.metric_push([a, b], 1.5, ring, first_bad, 1)             # captured: iteration 1 is baked in
    graph.replay()
    ops_train.metric_push([a, b], 2.5, ring, first_bad, 2)                 # outside, behind the replay: sees its result
    graph.replay()
    ops_train.metric_push([a, b], 3.5, ring, first_bad, 3)
    torch.cuda.synchronize()
    host = ring.cpu()
    tags = host[:, 0].view(torch.int32).tolist()
    assert tags[:4] == [0, 1, 2, 3] and set(tags[4:]) == {-1}
    assert host[0, 1:4].tolist() == [1.25, -2.5, 0.5]
    assert host[1, 1:4].tolist() == [5.0, -2.5, 1.5]                       # the replayed push overwrote its one row
    assert host[2, 1:4].tolist() == [2.5, -2.5, 2.5] and host[3, 1:4].tolist() == [5.0, -2.5, 3.5]
    assert int(first_bad.item()) == ops_train.METRIC_NO_BAD_ITERATION


def test_metric_ring_flushes_itself_after_64_pushes(dev):
    """200 pushes and no flush from outside (a writer period above the ring's length): the ring flushes itself whenever 64
    rows are unread, every row comes back once and in order, and every step keeps a step time of its own -- the event a
    pending step is timed from is never re-recorded under it (the times are those between consecutive events, so they are
    not negative and add up to the time between the first event and the last)"""
    from detectron2_centernet_amd.engine.metric_ring import MetricRing
    n = 200
    ring = MetricRing(dev)
    vals = [torch.tensor(float(i) + 0.5, device=dev) for i in range(n)]
    first, last = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(n):
        ring.begin_step()
        if i == 0:
            first.record()                   # right behind the event the first step is timed from
        vals[i].add_(0.0)                    # some device work per step
        ring.push({"loss": vals[i]}, 0.001 * i, 100 + i)
        assert ring.flushes == i // 64
    last.record()
    recs = ring.flush()
    assert ring.flushes == 4 and ring.flush() == []
    assert [r["iteration"] for r in recs] == list(range(100, 100 + n))
    assert [r["losses"]["loss"] for r in recs] == [i + 0.5 for i in range(n)]
    assert [r["data_time"] for r in recs] == [float(np.float32(0.001 * i)) for i in range(n)]
    times = [r["time"] for r in recs]
    assert all(t is not None and t >= 0.0 for t in times), [t for t in times if t is None or t < 0.0]
    total = first.elapsed_time(last) * 1e-3
    assert total > 0 and abs(sum(times) - total) <= 0.02 * total + 2e-4, (sum(times), total)


# ---------------------------------------------------------------------------------------------- helpers: models and batches
def _records(n, size, first=0, max_boxes=8):
    from detectron2_centernet_amd.data.catalog import synthetic_sample
    from detectron2_centernet_amd.structures import Boxes, Instances
    recs = []
    for i in range(n):
        s = synthetic_sample(first + i, size=size, max_boxes=max_boxes)
        inst = Instances((size, size))
        inst.gt_boxes, inst.gt_classes = Boxes(s["boxes"]), s["classes"]
        recs.append({"image": s["image"], "instances": inst, "height": size, "width": size})
    return recs


def _trainer(tmp_path, seed, batch_size, loader=None, calibrated=False, **kw):
    from test_model_gpu import make_model
    from detectron2_centernet_amd.engine.train_loop import SimpleTrainer
    model, cfg = make_model(tmp_path, "f16", seed=seed, calibrated=calibrated)
    cfg.SOLVER.IMS_PER_BATCH = batch_size
    return SimpleTrainer(model, loader, cfg, **kw)


# ---------------------------------------------------------------------------------------------- 2. ring == read-back
def test_ring_equals_per_step_read_back(tmp_path, dev):
    """25 steps of run_step_tensors (two eager, the capture, replays) with a ring attached; the test reads float(v) of the
    losses after every step; after ONE flush the storage's histories are those reads, exactly, and total_loss their sum"""
    from detectron2_centernet_amd.engine.bench_train import synthetic_batch
    from detectron2_centernet_amd.utils.events import EventStorage
    tr = _trainer(tmp_path, 4, 2)
    ring = tr.attach_metric_ring()
    batch = synthetic_batch(2, 128, 0, dev)
    reads, states = [], []
    with EventStorage(0) as tr.storage:
        for _ in range(25):
            losses = tr.run_step_tensors(*batch)
            reads.append({k: float(v) for k, v in losses.items()})
            states.append(tr.graph_state)
        assert ring.flushes == 0 and tr.iter == 25
        recs = tr.flush_metrics()
        assert ring.flushes == 1 and len(recs) == 25
        st = tr.storage
        assert states[:2] == ["eager", "eager"] and set(states[2:]) == {"captured"}
        for k in ("hm_loss", "wh_loss", "off_loss"):
            assert st.history(k).values() == [(r[k], i) for i, r in enumerate(reads)]
        assert st.history("total_loss").values() == [(sum(r.values()), i) for i, r in enumerate(reads)]
        assert [v for v, _ in st.history("data_time").values()] == [0.0] * 25
        assert "time" not in st.histories()                  # no IterationTimer said from where on it counts
        assert all(r["time"] > 0.0 for r in recs)
        assert len({tuple(r.values()) for r in reads}) > 20  # the trajectory moves: 25 equal rows would prove nothing


# ---------------------------------------------------------------------------------------------- 3. no synchronisation
def test_no_synchronisation_between_flushes(tmp_path, dev, monkeypatch):
    """a loop over record batches with the default kind of hooks: once the step is captured, nothing between two flushes
    synchronises with the device -- counted through every host-side door to a synchronisation"""
    from detectron2_centernet_amd.engine import hooks
    from detectron2_centernet_amd.engine.metric_ring import MetricRing
    from detectron2_centernet_amd.utils.events import JSONWriter
    batch = _records(2, 128)
    tr = _trainer(tmp_path, 4, 2, loader=itertools.repeat(batch), route_records=True)
    tr.attach_metric_ring()
    tr.register_hooks([hooks.IterationTimer(), hooks.LRScheduler(tr.optimizer),
                       hooks.PeriodicWriter([JSONWriter(str(tmp_path / "metrics.json"))], period=5)])
    calls, state = [], {"flush": False}

    def counted(owner, name, cuda_only=False):
        orig = getattr(owner, name)

        def wrapper(*a, **kw):
            if not state["flush"] and not (cuda_only and not a[0].is_cuda):
                calls.append((tr.iter, f"{getattr(owner, '__name__', owner)}.{name}"))
            return orig(*a, **kw)
        monkeypatch.setattr(owner, name, wrapper)

    counted(torch.cuda, "synchronize")
    counted(torch.cuda.Stream, "synchronize")
    counted(torch.cuda.Event, "synchronize")
    for name in ("item", "cpu", "tolist", "numpy", "__float__", "__int__", "__bool__"):
        counted(torch.Tensor, name, cuda_only=True)
    fetch = MetricRing._fetch

    def flagged(self):
        state["flush"] = True
        try:
            return fetch(self)
        finally:
            state["flush"] = False
    monkeypatch.setattr(MetricRing, "_fetch", flagged)
    tr.train(0, 14)
    assert tr.graph_state == "captured" and tr.metric_ring.flushes == 3          # after iterations 4, 9 and 13
    late = [c for c in calls if c[0] >= 3]
    assert late == [], late
    lines = [json.loads(l) for l in (tmp_path / "metrics.json").read_text().splitlines()]
    assert [l["iteration"] for l in lines] == [4, 9, 13]
    assert all({"total_loss", "hm_loss", "wh_loss", "off_loss", "lr", "time", "data_time"} <= set(l) for l in lines)
    assert [it for _, it in tr.storage.history("time").values()] == list(range(2, 14))
    assert [it for _, it in tr.storage.history("hm_loss").values()] == list(range(14))


# ---------------------------------------------------------------------------------------------- 4. non-finite
def test_non_finite_loss_raises_at_the_flush_and_nothing_is_saved(tmp_path, dev):
    from detectron2_centernet_amd.checkpoint import DetectionCheckpointer
    from detectron2_centernet_amd.engine import hooks
    from detectron2_centernet_amd.engine.bench_train import synthetic_batch
    tr = _trainer(tmp_path, 4, 2)
    ring = tr.attach_metric_ring()
    batch = synthetic_batch(2, 128, 0, dev)
    tr.run_step = lambda: tr.run_step_tensors(*batch)
    push = ring.push

    def poisoned(loss_dict, data_time, iteration):
        if iteration == 3:
            loss_dict["wh_loss"].fill_(float("nan"))          # on the device, in front of the push: no fault is provoked
        push(loss_dict, data_time, iteration)
    ring.push = poisoned
    out = tmp_path / "ckpt"
    ck = DetectionCheckpointer(tr.model, str(out), save_to_disk=True)
    tr.register_hooks([hooks.PeriodicCheckpointer(ck, 5), hooks.PeriodicWriter([], period=20)])
    with pytest.raises(FloatingPointError) as e:
        tr.train(0, 8)
    msg = str(e.value)
    assert msg.startswith("Loss became infinite or NaN at iteration=3!\nloss_dict = {") and "'wh_loss': nan" in msg
    assert "'hm_loss': " in msg and "'off_loss': " in msg
    assert tr.iter == 4                                       # the step ran on; the checkpoint due after iteration 4 flushed
    assert not out.exists() or os.listdir(out) == []


def test_metrics_sync_switch_is_the_per_step_path(tmp_path, dev, monkeypatch):
    """CTDET_METRICS_SYNC=1, read when the ring is built: every push reads the losses back (no device ring, no flush to wait
    for), the storage gets the same entries, and a non-finite loss raises in the step itself, as in the reference"""
    from detectron2_centernet_amd.engine.bench_train import synthetic_batch
    from detectron2_centernet_amd.utils.events import EventStorage
    monkeypatch.setenv("CTDET_METRICS_SYNC", "1")
    tr = _trainer(tmp_path, 4, 2)
    ring = tr.attach_metric_ring()
    monkeypatch.delenv("CTDET_METRICS_SYNC")
    assert ring.sync_mode
    batch = synthetic_batch(2, 128, 0, dev)
    with EventStorage(0) as tr.storage:
        reads = []
        for _ in range(4):
            reads.append({k: float(v) for k, v in tr.run_step_tensors(*batch).items()})
        assert len(tr.flush_metrics()) == 4 and ring.flushes == 0
        for k in ("hm_loss", "wh_loss", "off_loss"):
            assert tr.storage.history(k).values() == [(r[k], i) for i, r in enumerate(reads)]
        assert tr.storage.history("total_loss").values() == [(sum(r.values()), i) for i, r in enumerate(reads)]
        push = ring.push

        def poisoned(loss_dict, data_time, iteration):
            loss_dict["off_loss"].fill_(float("inf"))
            push(loss_dict, data_time, iteration)
        ring.push = poisoned
        with pytest.raises(FloatingPointError, match="Loss became infinite or NaN at iteration=4!"):
            tr.run_step_tensors(*batch)


# ---------------------------------------------------------------------------------------------- 5. records -> captured step
def test_record_batches_take_the_captured_step(tmp_path, dev):
    """a loader that yields one same-size record batch: routed, `run_step` replays the captured step from the third call on
    and follows the eager trajectory of the same records.  The bound is measured as in test_train_gpu.py::
    test_training_step_graph_replay_matches_eager: two eager runs give the noise, the routed run may deviate by 4x that + 1e-5,
    and the trajectory must move by more than 5x the bound, so that stale parameters cannot hide in it."""
    res = {}
    for mode in ("eager", "eager2", "routed"):
        # the model, the batch shape and the step count of the test this one takes its rule from
        tr = _trainer(tmp_path, 4, 4, loader=itertools.repeat(_records(4, 256, max_boxes=32)), calibrated=True,
                      route_records=mode == "routed")
        hist, states = [], []
        for _ in range(6):
            losses = tr.run_step()
            hist.append(sum(float(v) for v in losses.values()))
            states.append(tr.graph_state)
        res[mode] = (torch.tensor(hist, dtype=torch.float64), states, tr.iter, tr.optimizer.lr)
    (he, se, ite, lre), (he2, _, _, _), (hr, sr, itr, lrr) = res["eager"], res["eager2"], res["routed"]
    assert set(se) == {"eager"} and sr == ["eager", "eager"] + ["captured"] * 4
    assert ite == itr == 6 and lre == lrr
    noise = ((he2 - he).abs() / he.abs()).max().item()
    bound = 4 * noise + 1e-5
    dev_r = ((hr - he).abs() / he.abs()).max().item()
    move = abs(he[-1].item() - he[2].item()) / abs(he[2].item())
    print(f"record batches: run-to-run noise {noise:.2e}, routed vs eager {dev_r:.2e}, movement since the capture step {move:.2e}")
    assert dev_r <= bound, (he.tolist(), hr.tolist(), noise)
    assert move > 5 * bound, (move, bound)


def test_ragged_record_batches_stay_eager(tmp_path, dev):
    """images of unequal sizes: the routing declines, the step is the eager one of a trainer without routing -- the same
    code, so the same losses up to the step's run-to-run noise, measured by a second run without routing"""
    from detectron2_centernet_amd.structures import Boxes, Instances
    g = torch.Generator().manual_seed(12)
    batch = []
    for (h, w) in ((150, 200), (97, 131)):
        inst = Instances((h, w))
        x0, y0 = torch.rand(5, generator=g) * (w - 40), torch.rand(5, generator=g) * (h - 40)
        inst.gt_boxes = Boxes(torch.stack([x0, y0, x0 + 8 + torch.rand(5, generator=g) * 30, y0 + 8 + torch.rand(5, generator=g) * 30], 1))
        inst.gt_classes = torch.randint(0, 80, (5,), generator=g)
        batch.append({"image": torch.randint(0, 256, (3, h, w), generator=g, dtype=torch.uint8), "instances": inst})
    hist = {}
    for mode in ("off", "off2", "on"):
        tr = _trainer(tmp_path, 6, 2, route_records=mode == "on")
        assert tr._record_tensors(batch) is None
        hist[mode] = torch.tensor([sum(float(v) for v in tr.run_step(batch).values()) for _ in range(3)], dtype=torch.float64)
        assert tr.graph_state == "eager" and tr._graphs == {}
    noise = ((hist["off2"] - hist["off"]).abs() / hist["off"].abs()).max().item()
    got = ((hist["on"] - hist["off"]).abs() / hist["off"].abs()).max().item()
    print(f"ragged batch: run-to-run noise {noise:.2e}, routing on vs off {got:.2e}")
    assert got <= 4 * noise + 1e-5 and torch.isfinite(hist["on"]).all()
    # more than 128 objects in one image: declined too
    from detectron2_centernet_amd.engine.train_loop import TARGET_CAPACITY
    big = _records(2, 128)
    inst = Instances((128, 128))
    inst.gt_boxes = Boxes(torch.tensor([[4.0, 4.0, 40.0, 40.0]]).repeat(TARGET_CAPACITY + 1, 1))
    inst.gt_classes = torch.zeros(TARGET_CAPACITY + 1, dtype=torch.int64)
    big[1]["instances"] = inst
    assert tr._record_tensors(big) is None
    images, boxes, classes, counts = tr._record_tensors(_records(2, 128))
    assert images.shape == (2, 3, 128, 128) and images.dtype == torch.uint8 and images.is_cuda
    assert boxes.shape == (2, TARGET_CAPACITY, 4) and classes.shape == (2, TARGET_CAPACITY) and counts.dtype == torch.int32


# ---------------------------------------------------------------------------------------------- DefaultTrainer helpers
OPTS = ["MODEL.CENTERNET.HIP_PRECISION", "f16", "MODEL.CENTERNET.SCORE_THRESH_TEST", "0.0", "INPUT.MIN_SIZE_TRAIN", "(128,)",
        "INPUT.MAX_SIZE_TRAIN", "128", "INPUT.MIN_SIZE_TEST", "128", "INPUT.MAX_SIZE_TEST", "128", "DATALOADER.NUM_WORKERS", "0",
        "SOLVER.IMS_PER_BATCH", "2", "TEST.BATCH_SIZE", "2"]


def _write_yaml(tmp_path):
    from test_model_gpu import BASE, YAML
    (tmp_path / "Base-CenterNet.yaml").write_text(BASE)
    (tmp_path / "ctdet_dla_34_1x.yaml").write_text(YAML)
    return str(tmp_path / "ctdet_dla_34_1x.yaml")


def _cfg(tmp_path, out, *more):
    from detectron2_centernet_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(_write_yaml(tmp_path))
    cfg.merge_from_list(OPTS + ["OUTPUT_DIR", str(out)] + [str(m) for m in more])
    return cfg


def _fixed_batch_trainer(records):
    """DefaultTrainer on one fixed batch, without the evaluation hook"""
    from detectron2_centernet_amd.engine import DefaultTrainer, hooks

    class Fixed(DefaultTrainer):
        @classmethod
        def build_model(cls, cfg):
            # the benchmark's model, the one tests/test_fullsize_gpu.py measures the step's reproducibility on: non-zero DCN
            # offset convs.  With the zero ones of a fresh model every sampling point sits exactly ON a pixel, where bilinear
            # sampling has a kink, and the rounding noise of the first update decides the side.
            import bench
            return bench.build_model(cfg.MODEL.CENTERNET.HIP_PRECISION, torch.device("cuda:0"), seed=3, calibrate=False)[0]

        @classmethod
        def build_train_loader(cls, cfg):
            return itertools.repeat(records)

        def build_hooks(self):
            return [h for h in super().build_hooks() if not isinstance(h, hooks.EvalHook)]
    return Fixed


# ---------------------------------------------------------------------------------------------- 6. end to end
def test_default_trainer_end_to_end_and_eval_only_child(tmp_path, dev, clean_logger):
    from detectron2_centernet_amd.data.catalog import register_synthetic_files
    from detectron2_centernet_amd.engine import DefaultTrainer
    out = tmp_path / "out"
    # the names of the yaml, the files where the child process will look for them: tools/train_net.py registers the same set
    for name in ("bulb_train", "bulb_val"):
        register_synthetic_files(name, str(out / "synthetic"), length=8, size=128, replace=True)
    cfg = _cfg(tmp_path, out, "SOLVER.MAX_ITER", 6, "SOLVER.CHECKPOINT_PERIOD", 3, "TEST.EVAL_PERIOD", 3)
    torch.manual_seed(3)
    trainer = DefaultTrainer(cfg)
    trainer.model.wh[-1].bias.data.fill_(6.0)       # boxes of non-degenerate size: a random-init wh head gives empty boxes,
    trainer.resume_or_load(resume=False)            # which are dropped, and an AP over no detections is NaN
    assert trainer.start_iter == 0 and trainer.route_records and trainer.metric_ring is not None
    assert trainer.train() is None                              # no TEST.EXPECTED_RESULTS
    files = set(os.listdir(out))
    assert {"model_0000002.pth", "model_0000005.pth", "model_final.pth", "last_checkpoint", "metrics.json"} <= files
    assert (out / "last_checkpoint").read_text() == "model_final.pth"
    assert torch.load(out / "model_final.pth", weights_only=False)["iteration"] == 5
    assert trainer.graph_state == "captured"                    # the loader's records (one size after mapping) were routed
    st = trainer.storage
    ap = st.history("bbox/AP").values()
    assert [it for _, it in ap] == [2, 5] and all(math.isfinite(v) for v, _ in ap)
    for k in ("total_loss", "hm_loss", "wh_loss", "off_loss", "data_time", "lr"):
        assert [it for _, it in st.history(k).values()] == list(range(6)), k
    assert [it for _, it in st.history("time").values()] == [2, 3, 4, 5]
    lines = [json.loads(l) for l in (out / "metrics.json").read_text().splitlines()]
    assert [l["iteration"] for l in lines] == [5]               # period 20: the one write after the last iteration
    assert {"total_loss", "hm_loss", "wh_loss", "off_loss", "lr", "time", "data_time", "bbox/AP"} <= set(lines[0])
    assert lines[0]["bbox/AP"] == ap[-1][0] == trainer._last_eval_results["bbox"]["AP"]
    # --eval-only in a fresh process reproduces the last evaluation from model_final.pth
    child_out = tmp_path / "child"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train_net.py"), "--config-file", str(tmp_path / "ctdet_dla_34_1x.yaml"),
           "--eval-only"] + OPTS + ["MODEL.WEIGHTS", str(out / "model_final.pth"), "OUTPUT_DIR", str(child_out)]
    env = dict(os.environ, CTDET_SYNTHETIC_SET="8,8,128")
    done = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    assert done.returncode == 0, done.stdout[-3000:] + done.stderr[-3000:]
    child = json.load(open(child_out / "eval_results.json"))
    assert child["bbox"]["AP"] == ap[-1][0], (child["bbox"], trainer._last_eval_results["bbox"])
    for k, v in trainer._last_eval_results["bbox"].items():     # every figure (NaN where a category has no ground truth)
        assert child["bbox"][k] == v or (v != v and child["bbox"][k] != child["bbox"][k]), k


# ---------------------------------------------------------------------------------------------- 7. resume
# The resume experiment's settings: 3 + 3 iterations as the issue says, the benchmark's model, the config's own learning rate
# and warm-up, f16x3 -- and the full step size, 16 x 512^2, not the 2-4 images at 128^2 / 256^2 the other tests here use.
# A random-init network amplifies the rounding-order noise of the f32 atomics from step to step, the more the smaller the
# batch, and the test needs the weights-only control to clear 5 x 4 = 20 times a noise that is ONE sample (two straight runs).
# Measured, max |.| over the buffer, control (from the checkpoint of iteration 2) against straight over noise:
#     16 x 512^2:  parameters 6.34e-5 / 2.98e-7 = 213x,  momentum 10.1 / 0.105 = 96x    (resumed / noise: 1.23, 1.15)
#      4 x 256^2:  parameters 4.87e-5 / 8.16e-7 =  60x,  momentum 6.89 / 0.291 = 24x    (0.84, 0.91)
#      2 x 128^2:  parameters 5.23e-5 / 7.23e-7 =  72x,  momentum 9.22 / 0.356 = 26x    (1.45, 1.26)
#      4 x 256^2, BASE_LR 2e-3:  15x and 6.5x;   4 x 256^2, 5 + 5 iterations:  33x and 8.1x
# The small sizes separate, but the momentum buffer by 24-26x where 20x is asked, on a one-sample noise: that would be a test
# that fails now and then.  Raising BASE_LR or the iteration count, the issue's remedy for a control that does not show, makes
# it worse here (the noise grows faster than the control's distance).  A model whose BatchNorm weights are randomised too
# (test_model_gpu.randomize) or a 6-iteration warm-up is chaotic at every size tried: two straight runs part by as much as
# the whole movement within six steps.
RESUME_HALF, RESUME_BATCH, RESUME_SIZE = 3, 16, 512


def _resume_experiment(tmp_path, half=RESUME_HALF, batch=RESUME_BATCH, size=RESUME_SIZE, precision="f16x3", more=()):
    """two straight runs of 2 * half iterations (a, b), one of `half` iterations that a second trainer resumes, and the
    control that loads the checkpoint's weights only; all on one fixed batch"""
    from detectron2_centernet_amd.data.catalog import register_synthetic
    register_synthetic("bulb_train")                            # the model takes its class count from DATASETS.TRAIN[0]
    Fixed = _fixed_batch_trainer(_records(batch, size, max_boxes=32))
    solver = ["SOLVER.CHECKPOINT_PERIOD", half, "SOLVER.IMS_PER_BATCH", batch, "MODEL.CENTERNET.HIP_PRECISION", precision, *more]

    def run(out, max_iter, resume=None, weights=""):
        cfg = _cfg(tmp_path, out, "SOLVER.MAX_ITER", max_iter, *(["MODEL.WEIGHTS", weights] if weights else []), *solver)
        torch.manual_seed(3)
        tr = Fixed(cfg)
        if resume is not None:
            tr.resume_or_load(resume=resume)
        start = tr.start_iter
        names = {id(p): n for n, p in tr.model.named_parameters()}
        layout = [(names[id(p)], off, n) for p, (off, n) in zip(tr.optimizer.params, tr.optimizer.offsets)]
        tr.train()
        torch.cuda.synchronize()
        return {"param": tr.optimizer.flat_param.clone(), "mom": tr.optimizer.flat_mom.clone(), "start": start, "layout": layout,
                "lr": dict((it, v) for v, it in tr.storage.history("lr").values()), "iter": tr.iter}

    res = {"a": run(tmp_path / "a", 2 * half), "b": run(tmp_path / "b", 2 * half), "first": run(tmp_path / "c", half)}
    res["files"] = sorted(f for f in os.listdir(tmp_path / "c") if f.endswith(".pth"))
    res["resumed"] = run(tmp_path / "c", 2 * half, resume=True)
    # the control starts from the checkpoint of iteration half - 1.  Its periodic file: the resumed run has rewritten
    # model_final.pth by now (its last iteration is both periodic and final)
    ckpt = tmp_path / "c" / f"model_{half - 1:07d}.pth"
    res["control_from_iteration"] = torch.load(ckpt, weights_only=False)["iteration"]
    res["control"] = run(tmp_path / "d", half, resume=False, weights=str(ckpt))
    return res


def test_resume_continues_the_straight_run(tmp_path, dev, clean_logger):
    """3 iterations, a checkpoint, a new DefaultTrainer that resumes for 3 more == 6 iterations straight, on a fixed batch:
    parameters and momentum within 4x the run-to-run noise of two straight runs.  The control loads the checkpoint's weights
    only (the warm-up and the momentum restart) and must be off by more than 5x that bound."""
    half = RESUME_HALF
    res = _resume_experiment(tmp_path)
    a, b, first, resumed, control = (res[k] for k in ("a", "b", "first", "resumed", "control"))
    assert first["iter"] == half - 1 and res["files"] == [f"model_{half - 1:07d}.pth", "model_final.pth"]
    assert a["start"] == 0 and resumed["start"] == half and control["start"] == 0 and resumed["iter"] == 2 * half - 1
    assert res["control_from_iteration"] == half - 1 and control["iter"] == half - 1
    assert sorted(resumed["lr"]) == list(range(half, 2 * half)) and sorted(a["lr"]) == list(range(2 * half))
    assert resumed["lr"][half] == a["lr"][half] and resumed["lr"] == {it: a["lr"][it] for it in range(half, 2 * half)}
    assert control["lr"][0] == a["lr"][0] != a["lr"][half]      # the control's warm-up restarted
    for key in ("param", "mom"):
        noise = (b[key] - a[key]).abs().max().item()
        bound = 4 * noise
        got = (resumed[key] - a[key]).abs().max().item()
        off = (control[key] - a[key]).abs().max().item()
        print(f"resume, {key}: run-to-run noise {noise:.3e}, resumed vs straight {got:.3e}, weights-only control {off:.3e}")
        assert got <= bound, (key, got, noise)
        assert off > 5 * bound, (key, off, bound)


# ---------------------------------------------------------------------------------------------- 8. two ranks, one GPU
def _two_rank_worker(tmp, steps):
    from detectron2_centernet_amd.engine import DefaultTrainer, hooks
    from detectron2_centernet_amd.utils import comm
    from detectron2_centernet_amd.data.catalog import register_synthetic
    from detectron2_centernet_amd.utils.events import JSONWriter
    import pathlib
    tmp = pathlib.Path(tmp)
    register_synthetic("bulb_train")
    rank = comm.get_rank()
    torch.cuda.set_device(0)
    records = _records(2, 128, first=10 * rank)                 # every rank its own batch: the mean is not either rank's value
    reads = []

    class Fixed(DefaultTrainer):
        @classmethod
        def build_train_loader(cls, cfg):
            return itertools.repeat(records)

        def build_hooks(self):
            return [h for h in super().build_hooks() if not isinstance(h, (hooks.EvalHook, hooks.PeriodicWriter))] + [
                hooks.PeriodicWriter(self.build_writers() if comm.is_main_process() else [], period=1)]

        def build_writers(self):       # window 1: every line holds its own iteration's values
            os.makedirs(self.cfg.OUTPUT_DIR, exist_ok=True)
            return [JSONWriter(os.path.join(self.cfg.OUTPUT_DIR, "metrics.json"), window_size=1)]

        def run_step(self):
            losses = super().run_step()
            reads.append({k: float(v) for k, v in losses.items()})     # this rank's own per-step read
            return losses

    cfg = _cfg(tmp, tmp / "out", "SOLVER.MAX_ITER", steps, "SOLVER.CHECKPOINT_PERIOD", 100, "SOLVER.IMS_PER_BATCH", 4)
    torch.manual_seed(3)
    tr = Fixed(cfg)
    tr.train()
    torch.save({"reads": reads, "world": tr.reducer.world, "graph_state": tr.graph_state,
                "writers": [type(w).__name__ for w in tr._hooks[-1]._writers]}, tmp / f"rank{rank}.pt")


def test_two_ranks_write_the_mean_of_their_losses_once(tmp_path, clean_logger):
    from detectron2_centernet_amd.engine import launch
    steps = 5
    launch(_two_rank_worker, 2, num_machines=1, machine_rank=0, dist_url="auto", args=(str(tmp_path), steps), backend="gloo")
    r0, r1 = torch.load(tmp_path / "rank0.pt"), torch.load(tmp_path / "rank1.pt")
    assert r0["world"] == r1["world"] == 2 and r0["graph_state"] == r1["graph_state"] == "captured"
    assert r0["writers"] == ["JSONWriter"] and r1["writers"] == []
    found = [os.path.join(d, f) for d, _, fs in os.walk(tmp_path) for f in fs if f == "metrics.json"]
    assert found == [str(tmp_path / "out" / "metrics.json")]                  # exists once
    lines = [json.loads(l) for l in open(found[0]).read().splitlines()]
    assert [l["iteration"] for l in lines] == list(range(steps))
    for it, line in enumerate(lines):
        a, b = r0["reads"][it], r1["reads"][it]
        assert a != b
        for k in ("hm_loss", "wh_loss", "off_loss"):
            assert line[k] == (a[k] + b[k]) / 2, (it, k)       # the f64 mean of two f32 values is exact
        assert line["total_loss"] == sum((a[k] + b[k]) / 2 for k in ("hm_loss", "wh_loss", "off_loss"))
