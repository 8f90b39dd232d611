"""Data-parallel training step on the GPU: two ranks sharing the device, gloo collectives on the device tensors (the rehearsal
mode of `bench.py --gpus N`; the RCCL run needs as many GPUs as ranks).  Both ranks get the SAME batch, so the averaged
gradient equals the single-rank gradient and the parameters after the step must equal those of a single-process step --
through everything that differs in the data-parallel path: eager backward, gradients written straight into the flat buffer,
the per-bucket tap-major -> OIHW scatter launched from the reducer, the hooks that count a bucket's parameters (called by
autograd for some parameters and by the backward kernels' wrappers for the others), the bucketed all-reduce."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def _one_step(outfile):
    import bench
    from detectron2_centernet_amd.engine.bench_train import synthetic_batch
    from detectron2_centernet_amd.engine.train_loop import SimpleTrainer

    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    model, cfg = bench.build_model("f16", dev, seed=5, calibrate=False)
    model.train()
    cfg.SOLVER.IMS_PER_BATCH = 2
    tr = SimpleTrainer(model, None, cfg)
    if tr.reducer.world > 1:
        assert len(tr.reducer.buckets) >= 2      # the exchange really is bucketed
    batch = synthetic_batch(2, 128, 0, dev)       # rank argument fixed: identical data on every rank
    tr.run_step_tensors(*batch)
    torch.cuda.synchronize()
    names = {id(p): n for n, p in model.named_parameters()}
    layout = [(names[id(p)], off, n) for p, (off, n) in zip(tr.optimizer.params, tr.optimizer.offsets)]
    torch.save({"param": tr.optimizer.flat_param.cpu(), "grad": tr.optimizer.flat_grad.cpu(),
                "world": tr.reducer.world, "layout": layout, "calls": dict(tr.reducer.calls), "buckets": [tuple(b) for b in tr.reducer.buckets]}, outfile)


def _worker(outdir):
    from detectron2_centernet_amd.utils import comm

    _one_step(os.path.join(outdir, f"rank{comm.get_rank()}.pt"))


def test_two_rank_step_equals_single_rank_step(tmp_path):
    from detectron2_centernet_amd.engine import launch

    os.environ["CTDET_TRAIN_GRAPH"] = "hooks"      # the eager path: buckets launched from autograd hooks
    try:
        _one_step(str(tmp_path / "single.pt"))
        _one_step(str(tmp_path / "single2.pt"))     # the run-to-run noise of the step itself (order of the f32 atomics)
        launch(_worker, 2, num_machines=1, machine_rank=0, dist_url="auto", args=(str(tmp_path),), backend="gloo")
    finally:
        os.environ.pop("CTDET_TRAIN_GRAPH", None)
    ref = torch.load(tmp_path / "single.pt")
    r0, r1 = torch.load(tmp_path / "rank0.pt"), torch.load(tmp_path / "rank1.pt")
    assert ref["world"] == 1 and r0["world"] == 2 and r1["world"] == 2
    # DLA-34 has parameters that never receive a gradient (the `project` of the multi-level Trees: dla.py computes it and the
    # inner Tree ignores it); their bucket goes out in finish()
    missing = [r0["layout"][i][0] for i in range(len(r0["layout"])) if i not in r0["calls"]]
    assert all(".project." in n for n in missing), missing
    if not torch.equal(r0["grad"], r1["grad"]):                # one all-reduce result on both ranks
        d = (r0["grad"] - r1["grad"]).abs()
        bad = [(n, d[o:o + k].max().item(), r0["grad"][o:o + k].abs().max().item()) for n, o, k in r0["layout"]
               if d[o:o + k].max().item() > 0]
        raise AssertionError(f"ranks disagree after the exchange in {len(bad)} parameters, buckets {r0['buckets']}: {bad[:12]}")
    gs = ref["grad"].abs().max().item()
    assert gs > 0
    ref2 = torch.load(tmp_path / "single2.pt")
    noise = (ref2["grad"] - ref["grad"]).abs().max().item()
    # each rank's gradient is pre-divided by the world size and the two are summed: the single-rank gradient up to the
    # run-to-run noise of the step (f16 activations of a random-init net amplify the atomics' rounding order)
    assert (r0["grad"] - ref["grad"]).abs().max().item() <= 4 * noise + 5e-3 * gs, (noise, gs)
    cos = torch.nn.functional.cosine_similarity(r0["grad"].double(), ref["grad"].double(), dim=0).item()
    cos_noise = torch.nn.functional.cosine_similarity(ref2["grad"].double(), ref["grad"].double(), dim=0).item()
    assert cos > 0.9999 and 1 - cos <= 4 * (1 - cos_noise) + 2e-5, (cos, cos_noise)
    pnoise = (ref2["param"] - ref["param"]).abs().max().item()
    assert (r0["param"] - ref["param"]).abs().max().item() <= 4 * pnoise + 1e-5
    assert torch.equal(r0["param"], r1["param"])


def _graph_steps(outfile, nsteps=6, B=16, size=512, device_index=0):
    """nsteps training steps at BASELINE's per-GPU shape on the bench's own model; after every step the sums of the parameter
    and gradient buffers are recorded on the device (two tiny reductions on the launch stream: no host synchronisation that
    would change the step's timing)"""
    import bench
    from detectron2_centernet_amd.engine.bench_train import synthetic_batch
    from detectron2_centernet_amd.engine.train_loop import SimpleTrainer

    dev = torch.device("cuda", device_index)
    torch.cuda.set_device(device_index)
    model, cfg = bench.build_model(os.environ.get("CTDET_TEST_DP_PRECISION", "f16"), dev, seed=5)
    model.train()
    tr = SimpleTrainer(model, None, cfg)
    cfg.SOLVER.IMS_PER_BATCH = B * tr.reducer.world
    batch = synthetic_batch(B, size, 0, dev)       # rank argument fixed: identical data on every rank
    trace, losses, grads = [], [], []
    for _ in range(nsteps):
        l = tr.run_step_tensors(*batch)
        losses.append(torch.stack([v.float() for v in l.values()]).clone())
        trace.append(torch.stack([tr.optimizer.flat_param.double().sum(), tr.optimizer.flat_grad.double().abs().sum()]))
        grads.append(tr.optimizer.flat_grad.clone())          # the exchanged gradient this step's update used
    torch.cuda.synchronize()
    names = {id(p): n for n, p in model.named_parameters()}
    layout = [(names[id(p)], off, n) for p, (off, n) in zip(tr.optimizer.params, tr.optimizer.offsets)]
    torch.save({"param": tr.optimizer.flat_param.cpu(), "mom": tr.optimizer.flat_mom.cpu(), "world": tr.reducer.world,
                "trace": torch.stack(trace).cpu(), "losses": torch.stack(losses).cpu(), "graph_state": tr.graph_state,
                "grads": [g.cpu() for g in grads], "layout": layout, "buckets": [tuple(b) for b in tr.reducer.buckets]}, outfile)


def _graph_worker(outdir, own_gpu=False):
    from detectron2_centernet_amd.utils import comm

    _graph_steps(os.path.join(outdir, f"rank{comm.get_rank()}.pt"), device_index=comm.get_local_rank() if own_gpu else 0)


def test_two_rank_graph_steps_equal_single_rank_steps(tmp_path):
    """the data-parallel step as a replayed HIP graph (forward + backward captured; exchange, SGD launch and weight re-pack
    behind it): two ranks on the device, gloo, six steps of BASELINE's per-GPU shape (16 x 512^2) on identical batches.
    Both ranks must hold bit-identical parameters after every step (one all-reduce result, one update), and the trajectory
    must be the single-process one up to the run-to-run noise of the step (f32 atomics), which two single runs measure.
    Round 3 saw inf / drifting losses on this path in 3 of 6 runs of `bench.py --gpus 2`."""
    from detectron2_centernet_amd.engine import launch

    try:
        os.environ["CTDET_TRAIN_GRAPH"] = "0"
        _graph_steps(str(tmp_path / "eager.pt"))
        os.environ["CTDET_TRAIN_GRAPH"] = "ddp"
        _graph_steps(str(tmp_path / "single.pt"))
        _graph_steps(str(tmp_path / "single2.pt"))
        launch(_graph_worker, 2, num_machines=1, machine_rank=0, dist_url="auto", args=(str(tmp_path),), backend="gloo")
    finally:
        os.environ.pop("CTDET_TRAIN_GRAPH", None)
    ref, ref2 = torch.load(tmp_path / "single.pt"), torch.load(tmp_path / "single2.pt")
    eag = torch.load(tmp_path / "eager.pt")
    r0, r1 = torch.load(tmp_path / "rank0.pt"), torch.load(tmp_path / "rank1.pt")
    assert ref["world"] == 1 and r0["world"] == 2 and r1["world"] == 2
    assert ref["graph_state"] == r0["graph_state"] == r1["graph_state"] == "captured" and eag["graph_state"] == "eager"
    ms_ = eag["mom"].abs().max().item()
    print("momentum max |diff| / max: eager vs single graph", (eag["mom"] - ref["mom"]).abs().max().item() / ms_,
          "eager vs rank0", (eag["mom"] - r0["mom"]).abs().max().item() / ms_,
          "single graph vs rank0", (ref["mom"] - r0["mom"]).abs().max().item() / ms_)
    for st in range(len(ref["grads"])):
        d = (r0["grads"][st] - ref["grads"][st]).abs()
        nz = (ref2["grads"][st] - ref["grads"][st]).abs()
        bad = [(n, o, round(d[o:o + k].max().item() / max(1e-30, ref["grads"][st][o:o + k].abs().max().item()), 5))
               for n, o, k in r0["layout"] if d[o:o + k].max().item() > 8 * nz[o:o + k].max().item() + 1e-6 * ref["grads"][st][o:o + k].abs().max().item()]
        print(f"step {st}: {len(bad)} of {len(r0['layout'])} parameters off (relative max err), buckets {r0['buckets']}:", bad[:40])
    print("losses eager ", eag["losses"].sum(1).tolist())
    print("param sums eager", eag["trace"][:, 0].tolist())
    print("losses single", ref["losses"].sum(1).tolist(), "\nlosses rank0 ", r0["losses"].sum(1).tolist(),
          "\nlosses rank1 ", r1["losses"].sum(1).tolist())
    print("param sums single", ref["trace"][:, 0].tolist(), "\nrank0", r0["trace"][:, 0].tolist(), "\nrank1", r1["trace"][:, 0].tolist())
    assert torch.isfinite(r0["losses"]).all() and torch.isfinite(r1["losses"]).all()
    assert torch.equal(r0["trace"], r1["trace"]), (r0["trace"], r1["trace"])       # the same buffers after EVERY step
    assert torch.equal(r0["param"], r1["param"]) and torch.equal(r0["mom"], r1["mom"])
    # identical batches on both ranks: the first step's loss is the single-rank one; later steps up to the noise two single
    # runs show between themselves
    lnoise = (ref2["losses"] - ref["losses"]).abs().max().item()
    assert (r0["losses"] - ref["losses"]).abs().max().item() <= 4 * lnoise + 1e-5 * ref["losses"].abs().max().item(), lnoise
    pnoise = (ref2["param"] - ref["param"]).abs().max().item()
    assert (r0["param"] - ref["param"]).abs().max().item() <= 4 * pnoise + 1e-6, pnoise
    mnoise = (ref2["mom"] - ref["mom"]).abs().max().item()
    ms = ref["mom"].abs().max().item()
    assert (r0["mom"] - ref["mom"]).abs().max().item() <= 4 * mnoise + 1e-5 * ms, (mnoise, ms)
    # and the eager single-process trajectory: replaying the step as a graph changes nothing
    assert (eag["mom"] - ref["mom"]).abs().max().item() <= 4 * mnoise + 1e-5 * ms


def _compare_with_single(tmp_path, what):
    ref, ref2 = torch.load(tmp_path / "single.pt"), torch.load(tmp_path / "single2.pt")
    r0, r1 = torch.load(tmp_path / "rank0.pt"), torch.load(tmp_path / "rank1.pt")
    assert r0["world"] == 2 and r1["world"] == 2 and r0["graph_state"] == r1["graph_state"] == "captured", what
    assert torch.isfinite(r0["losses"]).all() and torch.equal(r0["trace"], r1["trace"]), what
    assert torch.equal(r0["param"], r1["param"]) and torch.equal(r0["mom"], r1["mom"]), what
    lnoise = (ref2["losses"] - ref["losses"]).abs().max().item()
    assert (r0["losses"] - ref["losses"]).abs().max().item() <= 4 * lnoise + 1e-5 * ref["losses"].abs().max().item(), what
    mnoise, ms = (ref2["mom"] - ref["mom"]).abs().max().item(), ref["mom"].abs().max().item()
    assert (r0["mom"] - ref["mom"]).abs().max().item() <= 4 * mnoise + 1e-5 * ms, (what, mnoise, ms)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs: one rank per GPU over RCCL")
@pytest.mark.parametrize("direct", [False, True])
def test_two_gpus_rccl_graph_steps_equal_single_rank_steps(tmp_path, direct):
    """the same check with the exchange that production uses: one rank per GPU, backend "nccl" (RCCL over xGMI) through
    torch.distributed, and once more with CTDET_RCCL_DIRECT=1 (the C ABI's ctdet_comm_* / ctdet_allreduce_bucket entry points).
    Skipped on one-GPU boxes; written in round 4 so that it runs the day two GPUs are visible."""
    from detectron2_centernet_amd.engine import launch

    os.environ["CTDET_TRAIN_GRAPH"] = "1"
    if direct:
        os.environ["CTDET_RCCL_DIRECT"] = "1"
    try:
        _graph_steps(str(tmp_path / "single.pt"))
        _graph_steps(str(tmp_path / "single2.pt"))
        launch(_graph_worker, 2, num_machines=1, machine_rank=0, dist_url="auto", args=(str(tmp_path), True), backend="nccl")
    finally:
        os.environ.pop("CTDET_TRAIN_GRAPH", None)
        os.environ.pop("CTDET_RCCL_DIRECT", None)
    _compare_with_single(tmp_path, f"RCCL, direct={direct}")


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs: one rank per GPU over RCCL")
def test_two_gpus_rccl_hooks_path(tmp_path):
    """the eager data-parallel path (buckets launched from autograd hooks, overlapping backward) over RCCL on two GPUs"""
    from detectron2_centernet_amd.engine import launch

    os.environ["CTDET_TRAIN_GRAPH"] = "hooks"
    try:
        _graph_steps(str(tmp_path / "single.pt"))
        _graph_steps(str(tmp_path / "single2.pt"))
        launch(_graph_worker, 2, num_machines=1, machine_rank=0, dist_url="auto", args=(str(tmp_path), True), backend="nccl")
    finally:
        os.environ.pop("CTDET_TRAIN_GRAPH", None)
    r0 = torch.load(tmp_path / "rank0.pt")
    r0["graph_state"] = "captured"          # (_compare_with_single checks the graph path's state; this path is eager by design)
    r1 = torch.load(tmp_path / "rank1.pt")
    assert r1["graph_state"] == "eager"
    r1["graph_state"] = "captured"
    torch.save(r0, tmp_path / "rank0.pt")
    torch.save(r1, tmp_path / "rank1.pt")
    _compare_with_single(tmp_path, "RCCL, hooks")


def test_two_rank_graph_steps_f16x3(tmp_path):
    """the parity-grade training mode through the data-parallel graph path: two ranks on the device over gloo, six steps of
    BASELINE's per-GPU shape, == the single-process trajectory"""
    from detectron2_centernet_amd.engine import launch

    os.environ["CTDET_TRAIN_GRAPH"] = "1"
    os.environ["CTDET_TEST_DP_PRECISION"] = "f16x3"
    try:
        _graph_steps(str(tmp_path / "single.pt"))
        _graph_steps(str(tmp_path / "single2.pt"))
        launch(_graph_worker, 2, num_machines=1, machine_rank=0, dist_url="auto", args=(str(tmp_path),), backend="gloo")
    finally:
        os.environ.pop("CTDET_TRAIN_GRAPH", None)
        os.environ.pop("CTDET_TEST_DP_PRECISION", None)
    _compare_with_single(tmp_path, "gloo, f16x3")


def test_bench_self_launches_its_ranks():
    """`python bench.py --gpus 2` with no launcher and no WORLD_SIZE starts two ranks itself (before touching the GPU) and
    rank 0 prints ONE line with n_gpus == 2; with fewer GPUs than ranks the ranks share the device and the line says so"""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "CTDET_BENCH_BACKEND")}
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
                          "--no-cpu-baseline", "--no-f32", "--no-f16", "--no-train", "--no-roofline"],
                         env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    lines = [ln for ln in out.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["dtype"] == "f16x3" and rec["value"] > 0
    assert rec["config"]["ranks_share_devices"] == (torch.cuda.device_count() < 2)


def test_two_rank_bench_training_graph_equals_hooks_path():
    """`python bench.py --gpus 2 --full` (the inference leg, then the f16x3 training leg): nothing between the training steps (the per-step recordings of the tests above put
    torch kernels between the eager SGD launch and the next replay, which is exactly what hid round 3's corruption -- the
    memset node of the captured step, profiles/r04_graph_memset_node.txt).  The captured data-parallel step must end where the
    eager hooks path ends: final losses of 14 steps equal to 1e-4 (a wrong run ended at hm_loss 99 ... inf against 93.72)."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "CTDET_BENCH_BACKEND",
                                                               "CTDET_TRAIN_GRAPH", "CTDET_TRAIN_CHECK")}
    finals = {}
    for mode in ("hooks", "1"):
        out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "20", "--warmup", "5",
                              "--full", "--no-cpu-baseline", "--no-f32", "--no-f16", "--no-roofline"],
                             env=dict(base, CTDET_TRAIN_GRAPH=mode), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert out.returncode == 0, out.stderr.decode()[-2000:]
        line = json.loads([ln for ln in out.stdout.decode().splitlines() if ln.startswith("{")][-1])
        rec = line["train"]
        assert line["n_gpus"] == 2 and rec["config"]["graph_state"] == ("captured" if mode == "1" else "eager"), rec["config"]
        finals[mode] = rec["config"]["final_losses"]
    for k, v in finals["hooks"].items():
        assert abs(finals["1"][k] - v) <= 1e-4 * abs(v), finals
