"""Host side of the trainer surface (no GPU): event storage and writers, TrainerBase and the hooks, the rank reduction of a
metric-ring flush on host arrays (also over two gloo ranks), the argument parser, resume arithmetic, verify_results, and the
new C-ABI symbol."""
import json
import logging
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from detectron2_centernet_amd.engine import hooks
from detectron2_centernet_amd.engine.metric_ring import (NO_BAD_ITERATION, RING_ROWS, ROW_FLOATS, MetricRing,
                                                         first_bad_iteration, put_records, records_from_rows)
from detectron2_centernet_amd.engine.train_loop import HookBase, TrainerBase
from detectron2_centernet_amd.utils.events import (CommonMetricPrinter, EventStorage, HistoryBuffer, JSONWriter,
                                                   get_event_storage)


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


# ---------------------------------------------------------------------------------------------- storage and history
def test_history_buffer_against_numpy():
    series = [3.0, -1.5, 8.25, 0.0, 2.0, 2.0, 7.5, -4.0, 1.0]
    h = HistoryBuffer()
    for i, v in enumerate(series):
        h.update(v, 10 + i)
    assert h.latest() == 1.0
    for w in (1, 2, 3, 4, 9, 20):
        assert h.median(w) == float(np.median(series[-w:])) and h.avg(w) == float(np.mean(series[-w:]))
    assert h.global_avg() == pytest.approx(float(np.mean(series)), rel=1e-15)
    assert h.values() == [(v, 10 + i) for i, v in enumerate(series)]
    short = HistoryBuffer(max_length=4)
    for v in series:
        short.update(v)
    assert [v for v, _ in short.values()] == series[-4:] and short.global_avg() == pytest.approx(float(np.mean(series)))


def test_event_storage_hints_scopes_and_put_at_iteration():
    with pytest.raises(AssertionError):
        get_event_storage()
    with EventStorage(5) as st:
        assert get_event_storage() is st and st.iter == 5
        st.put_scalar("a", 1)
        st.put_scalars(b=2.5, c=3, smoothing_hint=False)
        assert st.smoothing_hints() == {"a": True, "b": False, "c": False}
        with pytest.raises(AssertionError):
            st.put_scalar("a", 2, smoothing_hint=False)       # one hint per name
        st.step()
        with st.name_scope("eval"):
            st.put_scalar("AP", 40.0, smoothing_hint=False)
        st.put_scalar("a", 5)
        assert st.latest() == {"a": (5.0, 6), "b": (2.5, 5), "c": (3.0, 5), "eval/AP": (40.0, 6)}
        # the flush's entry point: a value filed under the iteration it belongs to, histories kept in iteration order
        st.step()
        st.step()
        for it, v in ((6, 10.0), (7, 30.0), (8, 20.0)):
            st._put_scalar_at("loss", v, it)
        assert st.history("loss").values() == [(10.0, 6), (30.0, 7), (20.0, 8)] and st.latest()["loss"] == (20.0, 8)
        assert st.latest_with_smoothing_hint(2)["loss"] == (25.0, 8) and st.latest_with_smoothing_hint(3)["loss"] == (20.0, 8)
        assert st.latest_with_smoothing_hint(3)["b"] == (2.5, 5)
        with pytest.raises(AssertionError):
            st._put_scalar_at("loss", 1.0, 7)                 # not behind a later entry
        with pytest.raises(KeyError):
            st.history("nothing")
        assert set(st.histories()) == {"a", "b", "c", "eval/AP", "loss"}
    with pytest.raises(AssertionError):
        get_event_storage()


def _scripted_run(writer, st, first, last):
    for it in range(first, last):
        st.put_scalar("total_loss", 100.0 - it)
        st.put_scalar("lr", 0.001 * (it + 1), smoothing_hint=False)
        if it in (9, 29):
            st.put_scalar("bbox/AP", float(it), smoothing_hint=False)
        if (it + 1) % 20 == 0 or it == 44:
            writer.write()
        st.step()


def test_json_writer_scripted_run_and_append(tmp_path):
    """45 iterations, written after 19, 39 and 44.  The reference's rule (events.py:103-122): of every scalar's LATEST
    value, those filed after the previous write, grouped by their iteration, in the order the storage first saw the scalars;
    smoothed scalars as the median of their last 20 values.  By hand: total_loss = 100 - it, so the median of iterations
    0..19 is (90 + 91) / 2, of 20..39 (70 + 71) / 2, of 25..44 (65 + 66) / 2; bbox/AP of iteration 9 goes out with the first
    write, that of 29 with the second, and the third has nothing new of it."""
    path = tmp_path / "metrics.json"
    want = [
        {"iteration": 19, "lr": 0.001 * 20, "total_loss": 90.5},
        {"bbox/AP": 9.0, "iteration": 9},
        {"iteration": 39, "lr": 0.001 * 40, "total_loss": 70.5},
        {"bbox/AP": 29.0, "iteration": 29},
        {"iteration": 44, "lr": 0.001 * 45, "total_loss": 65.5},
    ]
    w = JSONWriter(str(path))
    with EventStorage(0) as st:
        _scripted_run(w, st, 0, 45)
        w.write()                                       # nothing new: no line
    w.close()
    lines = path.read_text().splitlines()
    got = [json.loads(l) for l in lines]
    assert got == want
    assert all(list(json.loads(l)) == sorted(json.loads(l)) for l in lines)        # sorted keys
    # re-opening appends
    w = JSONWriter(str(path))
    with EventStorage(45) as st:
        st.put_scalar("total_loss", 1.0)
        w.write()
    w.close()
    again = [json.loads(l) for l in path.read_text().splitlines()]
    assert again[:5] == want and again[5] == {"iteration": 45, "total_loss": 1.0} and len(again) == 6


def test_common_metric_printer_line(caplog):
    p = CommonMetricPrinter(max_iter=100)
    with EventStorage(0) as st:
        for it in range(30):
            st.put_scalar("total_loss", 50.0 - it)
            st.put_scalar("hm_loss", 2.0)
            st.put_scalar("data_time", 0.01 * (it % 3))
            if it >= 2:
                st.put_scalar("time", 0.5 if it < 29 else 1.5)
            st.put_scalar("lr", 0.00025, smoothing_hint=False)
            st.put_scalar("bbox/AP", 12.0, smoothing_hint=False)
            if it < 29:
                st.step()
        p.logger.addHandler(caplog.handler)          # directly: the package logger may not propagate (setup_logger)
        try:
            with caplog.at_level(logging.INFO, logger=p.logger.name):
                p.write()
        finally:
            p.logger.removeHandler(caplog.handler)
        line = caplog.records[-1].getMessage()
        eta = 0.5 * (100 - 29)                                     # median(1000) of `time` times the iterations left
        assert st.latest()["eta_seconds"] == (eta, 29)
    times = [0.5] * 27 + [1.5]
    dts = [0.01 * (it % 3) for it in range(10, 30)]
    want = (" eta: 0:00:35  iter: 29  total_loss: {:.4g}  hm_loss: 2  time: {:.4f}  data_time: {:.4f}  lr: 0.00025  ".format(
        float(np.median([50.0 - it for it in range(10, 30)])), float(np.mean(times)), float(np.mean(dts))))
    assert line.startswith(want), (line, want)
    assert ("max_mem" in line) == torch.cuda.is_available() and "bbox" not in line and "eta_seconds" not in line


# ---------------------------------------------------------------------------------------------- trainer and hooks
class _Recorder(HookBase):
    def __init__(self, name, log):
        self.name, self.log = name, log

    def before_train(self):
        self.log.append((self.name, "before_train", self.trainer.iter))

    def after_train(self):
        self.log.append((self.name, "after_train", self.trainer.iter))

    def before_step(self):
        self.log.append((self.name, "before_step", self.trainer.iter))

    def after_step(self):
        assert self.trainer.storage.iter == self.trainer.iter
        self.log.append((self.name, "after_step", self.trainer.iter))


class _CountingTrainer(TrainerBase):
    def __init__(self, fail_at=None):
        super().__init__()
        self.steps, self.fail_at = [], fail_at

    def run_step(self):
        if self.iter == self.fail_at:
            raise ValueError("boom")
        self.steps.append(self.iter)


def test_trainer_base_call_order_and_after_train_on_error():
    log = []
    tr = _CountingTrainer()
    tr.register_hooks([_Recorder("a", log), None, _Recorder("b", log)])
    tr.train(2, 4)
    assert tr.steps == [2, 3] and tr.start_iter == 2 and tr.max_iter == 4 and tr.storage.iter == 4
    want = [("a", "before_train", 2), ("b", "before_train", 2)]
    for it in (2, 3):
        want += [("a", "before_step", it), ("b", "before_step", it), ("a", "after_step", it), ("b", "after_step", it)]
    want += [("a", "after_train", 3), ("b", "after_train", 3)]
    assert log == want
    with pytest.raises(ReferenceError):          # the hooks hold a weak proxy: they do not keep the trainer alive
        hook = tr._hooks[0]
        del tr
        hook.trainer.iter
    log = []
    tr = _CountingTrainer(fail_at=1)
    tr.register_hooks([_Recorder("a", log)])
    with pytest.raises(ValueError, match="boom"):
        tr.train(0, 5)
    assert tr.steps == [0] and log[-1] == ("a", "after_train", 1) and ("a", "after_step", 1) not in log
    with pytest.raises(AssertionError):
        tr.register_hooks([object()])


def test_periodic_checkpointer_files(tmp_path):
    from detectron2_centernet_amd.checkpoint import DetectionCheckpointer
    net = torch.nn.Linear(3, 2)
    ck = DetectionCheckpointer(net, str(tmp_path), save_to_disk=True)
    tr = _CountingTrainer()
    flushed = []
    tr.flush_metrics = lambda: flushed.append(tr.iter)
    tr.register_hooks([hooks.PeriodicCheckpointer(ck, 3)])
    tr.train(0, 7)
    files = sorted(f for f in os.listdir(tmp_path))
    assert files == ["last_checkpoint", "model_0000002.pth", "model_0000005.pth", "model_final.pth"]
    assert (tmp_path / "last_checkpoint").read_text() == "model_final.pth"
    assert torch.load(tmp_path / "model_final.pth", weights_only=False)["iteration"] == 6
    assert torch.load(tmp_path / "model_0000002.pth", weights_only=False)["iteration"] == 2
    assert flushed == [2, 5, 6]                  # the ring is flushed before every save, and only then


def test_periodic_checkpointer_writes_nothing_when_the_flush_raises(tmp_path):
    from detectron2_centernet_amd.checkpoint import DetectionCheckpointer
    ck = DetectionCheckpointer(torch.nn.Linear(3, 2), str(tmp_path), save_to_disk=True)
    tr = _CountingTrainer()

    def flush():
        raise FloatingPointError("Loss became infinite or NaN at iteration=1!")
    tr.flush_metrics = flush
    tr.register_hooks([hooks.PeriodicCheckpointer(ck, 3)])
    with pytest.raises(FloatingPointError):
        tr.train(0, 7)
    assert tr.steps == [0, 1, 2] and os.listdir(tmp_path) == []


def test_eval_hook_firing_and_non_float():
    fired = []
    tr = _CountingTrainer()
    flushed = []
    tr.flush_metrics = lambda: flushed.append(tr.iter)

    def ev():
        fired.append(tr.iter)
        return {"bbox": {"AP": 10.0 + tr.iter, "AP50": 20}}
    tr.register_hooks([hooks.EvalHook(3, ev)])
    tr.train(0, 7)
    assert fired == [2, 5, 6] and flushed == fired
    assert tr.storage.history("bbox/AP").values() == [(12.0, 2), (15.0, 5), (16.0, 6)]
    assert tr.storage.smoothing_hints()["bbox/AP50"] is False
    fired.clear()
    tr = _CountingTrainer()
    tr.register_hooks([hooks.EvalHook(0, ev)])             # period 0: only at the end
    tr.train(0, 4)
    assert fired == [3]
    tr = _CountingTrainer()
    tr.register_hooks([hooks.EvalHook(2, lambda: {"bbox": {"AP": "high"}})])
    with pytest.raises(ValueError, match="nested dict of float"):
        tr.train(0, 4)
    tr = _CountingTrainer()
    tr.register_hooks([hooks.EvalHook(2, lambda: None)])   # a rank without results
    tr.train(0, 4)
    assert "bbox/AP" not in tr.storage.histories()


def test_lr_scheduler_hook_records_and_never_steps():
    class Opt:
        lr = 0.5

    class Sched:
        calls = 0

        def step(self):
            Sched.calls += 1

    class Tr(_CountingTrainer):
        def run_step(self):
            super().run_step()
            opt.lr = opt.lr * 0.5          # what SimpleTrainer's own scheduler step does inside the step

    opt = Opt()
    tr = Tr()
    tr.register_hooks([hooks.LRScheduler(opt, Sched())])
    tr.train(0, 3)
    assert Sched.calls == 0
    assert tr.storage.history("lr").values() == [(0.5, 0), (0.25, 1), (0.125, 2)]     # the rate each step USED
    assert tr.storage.smoothing_hints()["lr"] is False


def test_iteration_timer_and_periodic_writer_and_callback():
    class W(hooks.EventWriter):
        def __init__(self):
            self.at, self.closed = [], False

        def write(self):
            self.at.append(get_event_storage().iter)

        def close(self):
            self.closed = True

    w = W()
    seen = []
    tr = _CountingTrainer()
    tr.time_from_iteration = None
    tr.register_hooks([hooks.IterationTimer(warmup_iter=3), hooks.PeriodicWriter([w], period=4),
                       hooks.CallbackHook(after_step=lambda t: seen.append(t.iter))])
    tr.train(10, 21)
    assert w.at == [11, 15, 19, 20] and w.closed and seen == list(range(10, 21))
    assert [it for _, it in tr.storage.history("time").values()] == list(range(12, 21))     # the warm-up iterations left out
    assert tr.time_from_iteration == 12
    with pytest.raises(AssertionError):
        hooks.PeriodicWriter([object()])


# ---------------------------------------------------------------------------------------------- the flush reduction
def _rows(world, iterations, names, seed=0):
    rng = np.random.default_rng(seed)
    rows = np.full((world, len(iterations), ROW_FLOATS), -7.0, dtype=np.float32)
    rows[:, :, 0] = np.asarray(iterations, dtype=np.int32).view(np.float32)[None]
    rows[:, :, 1:len(names) + 2] = rng.random((world, len(iterations), len(names) + 1), dtype=np.float32)
    return rows


def test_flush_reduction_world_one_is_the_identity():
    names = ("hm_loss", "wh_loss", "off_loss")
    its = [62, 63, 64, 65]
    rows = _rows(1, its, names)
    recs = records_from_rows(names, rows, its)
    assert [r["iteration"] for r in recs] == its
    for j, r in enumerate(recs):
        vals = [float(rows[0, j, 1 + i]) for i in range(3)]
        assert list(r["losses"]) == list(names) and list(r["losses"].values()) == vals
        assert r["total_loss"] == vals[0] + vals[1] + vals[2] == sum(vals)        # the Python sum, in dict order
        assert r["data_time"] == float(rows[0, j, 4])
    # dict order decides the order of the sum: three values whose f64 sum depends on it
    rows = np.zeros((1, 1, ROW_FLOATS), dtype=np.float32)
    rows[0, 0, 1:4] = [1e8, 1.0, -1e8]
    rows[0, 0, 0] = np.asarray([0], dtype=np.int32).view(np.float32)[0]
    a = records_from_rows(("a", "b", "c"), rows, [0])[0]["total_loss"]
    assert a == (1e8 + 1.0) + -1e8 == 1.0
    rows[0, 0, 1:4] = [2.0 ** 60, -(2.0 ** 60), 1.0]
    assert records_from_rows(("a", "b", "c"), rows, [0])[0]["total_loss"] == 1.0
    rows[0, 0, 1:4] = [2.0 ** 60, 1.0, -(2.0 ** 60)]
    assert records_from_rows(("a", "b", "c"), rows, [0])[0]["total_loss"] == 0.0     # 2^60 + 1 rounds away in f64
    assert records_from_rows(names, np.zeros((1, 0, ROW_FLOATS), np.float32), []) == []


def test_flush_reduction_mean_and_max_over_ranks():
    names = ("hm_loss", "wh_loss")
    its = [3, 4, 5]
    rows = _rows(3, its, names, seed=2)
    for j, r in enumerate(records_from_rows(names, rows, its)):
        for i, k in enumerate(names):
            assert r["losses"][k] == float(np.mean([float(rows[w, j, 1 + i]) for w in range(3)]))
        assert r["data_time"] == max(float(rows[w, j, 3]) for w in range(3))
        assert r["total_loss"] == r["losses"]["hm_loss"] + r["losses"]["wh_loss"]


def test_flush_reduction_checks_the_tags():
    names = ("hm_loss",)
    its = [10, 11, 12]
    ok = _rows(2, its, names)
    records_from_rows(names, ok, its)
    swapped = ok.copy()
    swapped[1, [0, 1]] = swapped[1, [1, 0]]                    # out of order on rank 1
    with pytest.raises(RuntimeError, match="rank 1 holds tag 11 where iteration 10"):
        records_from_rows(names, swapped, its)
    missing = ok.copy()
    missing[0, 2, 0] = np.asarray([-1], dtype=np.int32).view(np.float32)[0]        # never written
    with pytest.raises(RuntimeError, match="rank 0 holds tag -1 where iteration 12"):
        records_from_rows(names, missing, its)
    old = ok.copy()
    old[0, 1, 0] = np.asarray([11 - RING_ROWS], dtype=np.int32).view(np.float32)[0]   # a lap behind: not overwritten yet
    with pytest.raises(RuntimeError, match="iteration 11"):
        records_from_rows(names, old, its)
    with pytest.raises(ValueError):
        records_from_rows(names, ok[:, :2], its)
    assert first_bad_iteration([NO_BAD_ITERATION, NO_BAD_ITERATION]) is None
    assert first_bad_iteration([NO_BAD_ITERATION, 17, 40]) == 17


def test_put_records_files_each_row_at_its_iteration():
    names = ("hm_loss", "wh_loss", "off_loss")
    its = list(range(20, 26))
    recs = records_from_rows(names, _rows(1, its, names, seed=5), its)
    for r, t in zip(recs, (None, 0.5, 0.25, 0.125, 0.5, 0.5)):
        r["time"] = t
    with EventStorage(25) as st:
        put_records(st, recs, time_from_iteration=22)
        for k in names:
            assert st.history(k).values() == [(r["losses"][k], r["iteration"]) for r in recs]
        assert st.history("total_loss").values() == [(r["total_loss"], r["iteration"]) for r in recs]
        assert st.history("data_time").values() == [(r["data_time"], r["iteration"]) for r in recs]
        assert st.history("time").values() == [(0.25, 22), (0.125, 23), (0.5, 24), (0.5, 25)]
        assert list(st.histories())[:2] == ["data_time", "total_loss"]          # the reference's order of first puts
    with EventStorage(0) as st:      # a single loss is the total loss (train_loop.py:289)
        put_records(st, records_from_rows(("loss",), _rows(1, [0], ("loss",)), [0]))
        assert set(st.histories()) == {"data_time", "total_loss"}


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _fake_default_trainer(out_dir):
    from detectron2_centernet_amd.config import get_cfg
    from detectron2_centernet_amd.engine import DefaultTrainer

    class Opt:
        lr = 0.1

    cfg = get_cfg()
    cfg.OUTPUT_DIR = out_dir
    tr = DefaultTrainer.__new__(DefaultTrainer)
    TrainerBase.__init__(tr)
    tr.cfg, tr.optimizer, tr.scheduler, tr.checkpointer, tr.max_iter = cfg, Opt(), None, object(), 10
    return tr


def _gloo_worker(rank, world, port, out_dir, q):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        names = ("hm_loss", "wh_loss", "off_loss")
        its = [7, 8, 9]
        mine = torch.from_numpy(_rows(1, its, names, seed=100 + rank)[0])
        every = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)                                    # the one collective of a flush
        recs = records_from_rows(names, torch.stack(every).numpy(), its)
        both = [_rows(1, its, names, seed=100 + r)[0] for r in range(world)]
        for j, r in enumerate(recs):
            for i, k in enumerate(names):
                assert r["losses"][k] == (float(both[0][j, 1 + i]) + float(both[1][j, 1 + i])) / 2
            assert r["data_time"] == max(float(both[0][j, 4]), float(both[1][j, 4]))
            assert r["total_loss"] == sum(r["losses"].values())
        # the hooks are the same on every rank (a flush is a collective); the writers belong to rank 0 alone
        tr = _fake_default_trainer(out_dir)
        built = tr.build_hooks()
        assert [type(h).__name__ for h in built] == ["IterationTimer", "LRScheduler", "PeriodicCheckpointer", "EvalHook",
                                                      "PeriodicWriter"]
        writers = [type(w).__name__ for w in built[-1]._writers]
        assert writers[:2] == (["CommonMetricPrinter", "JSONWriter"] if rank == 0 else []) and (rank == 0 or not writers)
        dist.barrier()
        q.put((rank, "ok", os.path.exists(os.path.join(out_dir, "metrics.json"))))
    except Exception as e:  # noqa: BLE001
        q.put((rank, repr(e), None))
    finally:
        dist.destroy_process_group()


def test_flush_reduction_two_ranks_gloo(tmp_path):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, str(tmp_path), q)) for r in range(2)]
    for p in procs:
        p.start()
    results = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert sorted(results) == [(0, "ok", True), (1, "ok", True)], results
    assert sorted(os.listdir(tmp_path)) == ["metrics.json"]             # exists once


# ---------------------------------------------------------------------------------------------- defaults, testing, ABI
def test_default_argument_parser_defaults():
    from detectron2_centernet_amd.engine import default_argument_parser
    a = default_argument_parser().parse_args([])
    assert (a.config_file, a.resume, a.eval_only, a.num_gpus, a.num_machines, a.machine_rank, a.opts) == ("", False, False, 1, 1, 0, [])
    assert a.dist_url.startswith("tcp://127.0.0.1:") and 2 ** 15 + 2 ** 14 <= int(a.dist_url.rsplit(":", 1)[1]) < 2 ** 16
    a = default_argument_parser().parse_args(["--config-file", "x.yaml", "--resume", "--eval-only", "--num-gpus", "8",
                                              "SOLVER.MAX_ITER", "40", "TEST.EVAL_PERIOD", "20"])
    assert (a.config_file, a.resume, a.eval_only, a.num_gpus) == ("x.yaml", True, True, 8)
    assert a.opts == ["SOLVER.MAX_ITER", "40", "TEST.EVAL_PERIOD", "20"]


def test_resume_or_load_arithmetic(tmp_path):
    class Ck:
        def __init__(self, has, payload):
            self.has, self.payload, self.calls = has, payload, []

        def resume_or_load(self, path, *, resume=True):
            self.calls.append((path, resume))
            return self.payload

        def has_checkpoint(self):
            return self.has

    for has, payload, resume, want in ((True, {"iteration": 2}, True, 3), (True, {"iteration": 2}, False, 0),
                                       (False, {}, True, 0), (True, {}, True, 0)):
        tr = _fake_default_trainer(str(tmp_path))
        tr.cfg.MODEL.WEIGHTS = "w.pth"
        tr.start_iter, tr.checkpointer = 0, Ck(has, payload)
        tr.resume_or_load(resume=resume)
        assert tr.start_iter == want and tr.checkpointer.calls == [("w.pth", resume)]


def test_default_setup_writes_config_and_log(tmp_path, clean_logger):
    from detectron2_centernet_amd.config import get_cfg
    from detectron2_centernet_amd.engine import default_argument_parser, default_setup
    cfg = get_cfg()
    cfg.OUTPUT_DIR, cfg.SEED = str(tmp_path / "out"), 11
    default_setup(cfg, default_argument_parser().parse_args([]))
    a = torch.rand(3)
    again = get_cfg()
    again.merge_from_file(str(tmp_path / "out" / "config.yaml"))
    assert again.SEED == 11 and again.OUTPUT_DIR == cfg.OUTPUT_DIR
    log = (tmp_path / "out" / "log.txt").read_text()
    assert "Rank of current process: 0. World size: 1" in log and "Full config saved to" in log
    default_setup(cfg, default_argument_parser().parse_args([]))
    assert torch.equal(torch.rand(3), a)                        # the seed was set


def test_verify_results_and_flatten():
    from detectron2_centernet_amd.config import get_cfg
    from detectron2_centernet_amd.evaluation import flatten_results_dict, print_csv_format, verify_results
    res = {"bbox": {"AP": 31.2, "AP50": 50.0, "AP-class_0": 3.0}}
    assert flatten_results_dict({"a": {"b": {"c": 1}, "d": 2}, "e": 3}) == {"a/b/c": 1, "a/d": 2, "e": 3}
    cfg = get_cfg()
    assert verify_results(cfg, res) is True                     # nothing expected
    cfg.TEST.EXPECTED_RESULTS = [["bbox", "AP", 31.0, 0.5]]
    assert verify_results(cfg, res) is True
    for bad in ([["bbox", "AP", 30.0, 0.5]], [["bbox", "APx", 31.0, 0.5]], [["segm", "AP", 31.0, 0.5]]):
        cfg.TEST.EXPECTED_RESULTS = bad
        with pytest.raises(SystemExit):
            verify_results(cfg, res)
    cfg.TEST.EXPECTED_RESULTS = [["bbox", "AP", 31.0, 0.5]]
    with pytest.raises(SystemExit):
        verify_results(cfg, {"bbox": {"AP": float("nan")}})
    print_csv_format(res)


def test_train_net_refuses_unregistered_datasets_unless_asked(tmp_path, monkeypatch):
    """tools/train_net.py: a dataset name nothing registered is an error; only CTDET_SYNTHETIC_SET replaces it by the synthetic
    set.  register_synthetic_files does not replace a registration unasked."""
    import importlib.util
    from detectron2_centernet_amd.config import get_cfg
    from detectron2_centernet_amd.data.catalog import DatasetCatalog, register_synthetic_files
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = get_cfg()
    names = (f"trainer_host_train_{os.getpid()}", f"trainer_host_val_{os.getpid()}")
    cfg.DATASETS.TRAIN, cfg.DATASETS.TEST, cfg.OUTPUT_DIR = (names[0],), (names[1],), str(tmp_path)

    def load(env):
        if env is None:
            monkeypatch.delenv("CTDET_SYNTHETIC_SET", raising=False)
        else:
            monkeypatch.setenv("CTDET_SYNTHETIC_SET", env)
        spec = importlib.util.spec_from_file_location("train_net_under_test", os.path.join(root, "tools", "train_net.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod

    with pytest.raises(KeyError, match="not registered"):
        load(None).register_missing_datasets(cfg)
    assert names[0] not in DatasetCatalog and not os.path.exists(tmp_path / "synthetic")
    try:
        load("3,2,32").register_missing_datasets(cfg)
        train, val = DatasetCatalog.get(names[0]), DatasetCatalog.get(names[1])
        assert len(train) == 3 and len(val) == 2 and all(os.path.isfile(r["file_name"]) and r["annotations"] for r in train + val)
        assert (train[0]["height"], train[0]["width"]) == (32, 32)
        load(None).register_missing_datasets(cfg)              # nothing missing any more: nothing to do, no error
        with pytest.raises(ValueError, match="already registered"):
            register_synthetic_files(names[0], str(tmp_path / "synthetic"), length=1, size=32)
        assert len(register_synthetic_files(names[0], str(tmp_path / "synthetic"), length=1, size=32, replace=True)) == 1
    finally:
        for n in names:
            if n in DatasetCatalog:
                DatasetCatalog.remove(n)


def test_new_symbol_and_abi_version():
    """the push lives in libctdet_metrics.so, next to the hot-path library, whose ABI (version 8) it does not touch"""
    from detectron2_centernet_amd import _lib
    l = _lib.lib()
    assert l.ctdet_abi_version() == 8 and "ctdet_metric_push" not in _lib.SIGNATURES
    m = _lib.metrics_lib()
    assert "ctdet_metric_push" in _lib.METRICS_SIGNATURES and hasattr(m, "ctdet_metric_push")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ctdet_metrics.h")).read()
    assert "ctdet_metric_push(" in header and "CTDET_METRIC_MAX_SCALARS 8" in header
    assert m.ctdet_metric_push(None, 1, 0.0, None, 64, 10, None, 0, None) == -22 and b"null" in l.ctdet_last_error()


def test_metric_ring_refuses_cpu_tensors():
    from detectron2_centernet_amd import ops_train
    with pytest.raises(NotImplementedError):
        MetricRing(torch.device("cpu"))
    ring = torch.zeros(RING_ROWS, ROW_FLOATS)
    with pytest.raises(NotImplementedError):
        ops_train.metric_push([torch.zeros(())], 0.0, ring, torch.zeros(1, dtype=torch.int32), 0)


def test_exports():
    import detectron2_centernet_amd.engine as E
    import detectron2_centernet_amd.evaluation as V
    import detectron2_centernet_amd.utils as U
    for n in ("DefaultTrainer", "default_argument_parser", "default_setup", "HookBase", "TrainerBase", "SimpleTrainer", "hooks",
              "MetricRing", "EvalHook", "PeriodicCheckpointer", "PeriodicWriter", "LRScheduler", "IterationTimer", "CallbackHook"):
        assert n in E.__all__ and hasattr(E, n)
    for n in ("flatten_results_dict", "print_csv_format", "verify_results"):
        assert n in V.__all__ and hasattr(V, n)
    for n in ("EventStorage", "get_event_storage", "EventWriter", "JSONWriter", "CommonMetricPrinter", "HistoryBuffer",
              "setup_logger"):
        assert n in U.__all__ and hasattr(U, n)
    assert issubclass(E.SimpleTrainer, E.TrainerBase)
