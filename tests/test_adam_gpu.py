"""SOLVER.OPTIMIZER ADAM / ADAMW on the GPU: the flat step against torch.optim.Adam / AdamW on the CPU (small net, DLA-34's
full size), its determinism, its capture into a HIP graph with the step count advancing inside the replays, the trainer's
single-GPU and two-rank steps, and the checkpoint round trip.

Oracle everywhere: torch.optim.Adam / AdamW (foreach=False: the single-tensor path) with one param group per parameter carrying
the learning rate the kernel read and the run's weight decay, preceded by clip_grad_norm_ / clip_grad_value_ called with ONE
parameter at a time.

Bounds.  Parameters and first moment against torch's f32 result: atol 1e-6 + rtol 1e-6, this kernel family's own
(test_hip_ops.test_sgd_matches_torch).  That bound is blind on the second moment (v ~ 1e-3 g^2 sits under the atol), so
exp_avg_sq / max_exp_avg_sq are judged relatively: with E(X) = max over parameters of max|X - X64| / max|X64| and X64 from
torch's f64 run, E(kernel) <= 4 E(torch f32) + 1.2e-7 -- the margin test_full_size_against_torch gives the norms, the floor two
f32 ulps."""
import math
import os

import pytest
import torch

from test_grad_clip_gpu import close, full_size_grads, hyper, set_clip, split, worst

pytestmark = pytest.mark.gpu

KINDS = {"adam": ("ADAM", False), "adamw": ("ADAMW", False), "adam_amsgrad": ("ADAM", True), "adamw_amsgrad": ("ADAMW", True)}


def set_adam(cfg, name, amsgrad=False, clip=None):
    cfg.SOLVER.OPTIMIZER = name
    cfg.SOLVER.ADAM.AMSGRAD = amsgrad
    if clip is not None:
        set_clip(cfg, clip[0], clip[1], clip[2] if len(clip) > 2 else 2.0)


def state_of(opt):
    """[exp_avg, exp_avg_sq(, max_exp_avg_sq)] per parameter, on the CPU"""
    flats = [opt.exp_avg, opt.exp_avg_sq] + ([opt.max_exp_avg_sq] if opt.amsgrad else [])
    return [split(f.cpu(), opt) for f in flats]


def torch_adam_step(params, state, grads, hyp, t, opt, clip, dtype=torch.float32):
    """step t + 1 of torch.optim.Adam / AdamW on the CPU in `dtype`, from (parameters, state, step count t) and the gradients:
    every parameter clipped on its own, then the optimizer.  Returns (parameters, state, norms or None) after the step."""
    ps = [torch.nn.Parameter(p.clone().to(dtype)) for p in params]
    cls = torch.optim.AdamW if opt.decoupled else torch.optim.Adam
    ref = cls([{"params": [p], "lr": lr, "weight_decay": wd} for p, (lr, wd) in zip(ps, hyp)], lr=1.0, betas=opt.betas,
              eps=opt.eps, amsgrad=opt.amsgrad, foreach=False)
    names = ["exp_avg", "exp_avg_sq"] + (["max_exp_avg_sq"] if opt.amsgrad else [])
    norms = []
    for i, (p, g) in enumerate(zip(ps, grads)):
        p.grad = g.clone().to(dtype)
        ref.state[p] = {"step": torch.tensor(float(t)), **{k: s[i].clone().to(dtype) for k, s in zip(names, state)}}
        if clip is not None and clip[0] == "norm":
            norms.append(torch.nn.utils.clip_grad_norm_(p, clip[1], clip[2]))
        elif clip is not None:
            torch.nn.utils.clip_grad_value_(p, clip[1])
    ref.step()
    assert all(int(ref.state[p]["step"]) == t + 1 for p in ps)
    return [p.detach() for p in ps], [[ref.state[p][k] for p in ps] for k in names], (torch.stack(norms) if norms else None)


def rel_err(got, want64):
    """E(X) = max over parameters of max|X - X64| / max|X64| (a parameter whose X64 is all zero must be all zero)"""
    e = 0.0
    for a, b in zip(got, want64):
        scale = b.abs().max().item() if b.numel() else 0.0
        if scale == 0.0:
            assert not a.numel() or a.abs().max().item() == 0.0
            continue
        e = max(e, (a.double() - b).abs().max().item() / scale)
    return e


def compare(opt, want32, state32, state64, what):
    """the bounds of the module docstring; prints the worst value of each comparison.  Returns them"""
    gotp, got = split(opt.flat_param.cpu(), opt), state_of(opt)
    wp, wm = worst(torch.cat(gotp), torch.cat(want32)), worst(torch.cat(got[0]), torch.cat(state32[0]))
    line = f"{what}: parameter / exp_avg error {wp:.3f} / {wm:.3f} of the bound"
    es = []
    for k in range(1, len(got)):
        ek, et = rel_err(got[k], state64[k]), rel_err(state32[k], state64[k])
        es.append((ek, et))
        line += f"; {'exp_avg_sq' if k == 1 else 'max_exp_avg_sq'} E kernel {ek:.3e}, torch f32 {et:.3e}"
    print(line)
    assert close(torch.cat(gotp), torch.cat(want32)) and close(torch.cat(got[0]), torch.cat(state32[0])), line
    for ek, et in es:
        assert ek <= 4 * et + 1.2e-7, line
    return wp, wm, es


# ------------------------------------------------------------------------------------------------------------------------
# 1. small net through build_optimizer
# ------------------------------------------------------------------------------------------------------------------------
SCALES = [3.0, 0.01, 0.3, 1.0, 0.05, 2.0]             # tests/golden/make_g21.py
SMALL_CLIPS = {"noclip": None, "value": ("value", 0.5), "norm2": ("norm", 1.0, 2.0), "norminf": ("norm", 0.3, math.inf)}


def small_net(dev, seed=21):
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3), torch.nn.BatchNorm2d(8), torch.nn.Conv2d(8, 5, 1))
    for p in net.parameters():
        p.data.copy_(torch.randn(p.shape) * 0.5)
    return net.to(dev)


def small_cfg(name, amsgrad, clip):
    from detectron2_centernet_amd.config import get_cfg

    cfg = get_cfg()
    cfg.SOLVER.BASE_LR, cfg.SOLVER.BIAS_LR_FACTOR, cfg.SOLVER.WEIGHT_DECAY_BIAS = 0.02, 2.0, 0.0
    set_adam(cfg, name, amsgrad, clip)
    return cfg


@pytest.mark.parametrize("clip", sorted(SMALL_CLIPS))
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_small_net_matches_torch(dev, kind, clip):
    """six steps, two learning rates, three weight decays; the torch chains (f32 and f64) run on their own results, the kernel
    on its own: what is compared is six steps of drift, not one"""
    from detectron2_centernet_amd.solver import FlatAdam, build_optimizer

    name, amsgrad = KINDS[kind]
    clip = SMALL_CLIPS[clip]
    net = small_net(dev)
    opt = build_optimizer(small_cfg(name, amsgrad, clip), net)
    assert isinstance(opt, FlatAdam) and opt.decoupled == (name == "ADAMW") and opt.amsgrad == amsgrad
    assert len(opt.runs) >= 3 and len(opt.lr_factors) == 2 and opt.flat_mom is opt.exp_avg
    assert (opt.max_exp_avg_sq is not None) == amsgrad and int(opt.step_count) == 0
    hyp = hyper(opt, opt._lr_table.cpu())
    scales = list(reversed(SCALES))                      # opt.params is the reversed module order
    p32, s32 = split(opt.flat_param.cpu(), opt), state_of(opt)
    p64, s64 = [p.double() for p in p32], [[x.double() for x in s] for s in s32]
    gen = torch.Generator().manual_seed(2100)
    all_grads = [[torch.randn(n, generator=gen) * s for (_, n), s in zip(opt.offsets, scales)] for _ in range(6)]
    clipped = kept = 0
    if clip is not None:                                 # the condition on the inputs, from torch's own norms
        norms = torch.stack([torch.linalg.vector_norm(g, clip[2] if clip[0] == "norm" else math.inf)
                             for grads in all_grads for g in grads])
        clipped, kept = int((norms > clip[1]).sum()), int((norms <= clip[1]).sum())
        assert clipped >= 3 and kept >= 3, (clipped, kept)
    worst_p = worst_m = 0.0
    for step, grads in enumerate(all_grads):
        opt.flat_grad.copy_(torch.cat(grads).to(dev))
        before = opt.flat_grad.clone()
        opt.step()
        assert torch.equal(opt.flat_grad, before)        # the clipped gradient is not written back
        p32, s32, _ = torch_adam_step(p32, s32, grads, hyp, step, opt, clip)
        p64, s64, _ = torch_adam_step(p64, s64, grads, hyp, step, opt, clip, torch.float64)
        wp, wm, _ = compare(opt, p32, s32, s64, f"{kind} {clip} step {step}")
        worst_p, worst_m = max(worst_p, wp), max(worst_m, wm)
        assert int(opt.step_count) == step + 1
    if clip is not None and clip[0] == "norm":
        assert (opt.clip_coefs < 1).any() and (opt.clip_coefs == 1).any()
    print(f"small net {kind} {clip}: worst parameter / exp_avg error {worst_p:.3f} / {worst_m:.3f} of the bound; "
          f"{clipped} parameter-steps clipped, {kept} not")


# ------------------------------------------------------------------------------------------------------------------------
# 2. + 3. full size
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dla34(dev):
    import bench

    model, cfg = bench.build_model("f16x3", dev, seed=3, calibrate=False)
    return model, cfg


FULL_CASES = {"adam": ("ADAM", False, None), "adamw_amsgrad": ("ADAMW", True, None), "adam_norm2": ("ADAM", False, ("norm", 1.0, 2.0)),
              "adamw_value": ("ADAMW", False, ("value", 0.01))}


def full_grads(opt, clip, step):
    return full_size_grads(opt, clip or ("value", 0.01), step, (clip or ("value", 0.01))[1])


@pytest.mark.parametrize("case", sorted(FULL_CASES))
def test_full_size_against_torch(dev, dla34, case):
    """DLA-34's real parameter list: three steps after set_lr_factor(0.37)"""
    from detectron2_centernet_amd.solver import build_optimizer

    name, amsgrad, clip = FULL_CASES[case]
    model, cfg = dla34
    cfg = cfg.clone()
    set_adam(cfg, name, amsgrad, clip)
    opt = build_optimizer(cfg, model)
    assert opt.flat_param.numel() > 18e6 and len(opt.runs) > 50 and max(n for _, n in opt.offsets) == 512 * 512 * 9
    opt.set_lr_factor(0.37)
    hyp = hyper(opt, opt._lr_table.cpu())
    p32, s32 = split(opt.flat_param.cpu(), opt), state_of(opt)
    p64, s64 = [p.double() for p in p32], [[x.double() for x in s] for s in s32]
    P = len(opt.params)
    for step in range(3):
        grads = full_grads(opt, clip, step)
        opt.flat_grad.copy_(torch.cat(grads).to(dev))
        opt.step()
        p32, s32, norms32 = torch_adam_step(p32, s32, grads, hyp, step, opt, clip)
        p64, s64, norms64 = torch_adam_step(p64, s64, grads, hyp, step, opt, clip, torch.float64)
        compare(opt, p32, s32, s64, f"full size {case} step {step}")
        if clip is not None and clip[0] == "norm":
            n_clipped = int((clip[1] / (norms64 + 1e-6) < 1).sum())
            assert abs(n_clipped - P / 2) <= 0.15 * P, (n_clipped, P)      # half the parameters clipped, half not
            assert torch.equal(opt.clip_coefs.cpu() < 1, torch.clamp(clip[1] / (norms64 + 1e-6), max=1.0) < 1)
            print(f"  {n_clipped} of {P} parameters clipped")
    assert int(opt.step_count) == 3


@pytest.mark.parametrize("case", ["adamw_amsgrad", "adam_norm2"])
def test_full_size_step_is_deterministic(dev, dla34, case):
    """the same state and gradients stepped twice: identical bits in every buffer, the step counter included"""
    from detectron2_centernet_amd.solver import build_optimizer

    name, amsgrad, clip = FULL_CASES[case]
    model, cfg = dla34
    cfg = cfg.clone()
    set_adam(cfg, name, amsgrad, clip)
    opt = build_optimizer(cfg, model)
    opt.flat_grad.copy_(torch.cat(full_grads(opt, clip, 0)).to(dev))
    opt.step()
    opt.flat_grad.copy_(torch.cat(full_grads(opt, clip, 1)).to(dev))
    buffers = [opt.flat_param, opt.exp_avg, opt.exp_avg_sq, opt.step_count] + ([opt.max_exp_avg_sq] if amsgrad else [])
    saved = [b.clone() for b in buffers]
    runs = []
    for _ in range(2):
        for b, s in zip(buffers, saved):
            b.copy_(s)
        opt._bias.fill_(-1.0)
        if opt.grad_norms is not None:
            opt.grad_norms.fill_(-1.0)
            opt.clip_coefs.fill_(-1.0)
        opt.step()
        runs.append([b.clone() for b in buffers] + [opt._bias.clone()] +
                    ([opt.grad_norms.clone(), opt.clip_coefs.clone()] if opt.grad_norms is not None else []))
    assert not torch.equal(runs[0][0], saved[0]) and int(runs[0][3]) == 2
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------------------
# 4. capture
# ------------------------------------------------------------------------------------------------------------------------
def _small_groups(dev):
    g = torch.Generator().manual_seed(44)
    lens = [1, 255, 256, 257, 3, 70001, 1, 1, 4096, 9, 300000]
    return [(torch.nn.Parameter(torch.randn(n, generator=g).to(dev)), 1.0 + (i % 2), 1e-4 * (i % 3)) for i, n in enumerate(lens)], g


@pytest.mark.parametrize("decoupled,amsgrad,clip,extra", [(False, False, None, 1), (True, True, ("value", 0.5), 1),
                                                          (False, True, ("norm", 20.0, 2.0), 3), (True, False, ("norm", 2.0, math.inf), 3)],
                         ids=lambda v: str(v).replace(" ", ""))
def test_step_captures_as_kernels_only_and_keeps_counting(dev, decoupled, amsgrad, clip, extra):
    """`step()` captured alone holds kernels only: plain SGD's captured step plus the advance (plus the two norm launches);
    THREE replays on three gradients == three eager steps, bit for bit -- a bias correction frozen at the capture differs at
    the second replay -- and the device step count has advanced by three"""
    from detectron2_centernet_amd.engine import graph_nodes
    from detectron2_centernet_amd.solver import FlatAdam, FlatSGD

    def capture(opt):
        graph = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(graph):
            opt.step()
        nodes = graph_nodes.node_types(graph.raw_cuda_graph())
        graph.instantiate()
        return graph, nodes

    groups, g = _small_groups(dev)
    plain = FlatSGD(groups, 0.05, 0.9)
    plain.flat_grad.copy_(torch.randn(plain.flat_grad.numel(), generator=g).to(dev))
    plain.step()
    torch.cuda.synchronize()
    _, plain_nodes = capture(plain)
    assert set(plain_nodes) <= {"kernel", "empty"}

    groups, g = _small_groups(dev)
    opt = FlatAdam(groups, 0.05, decoupled=decoupled, amsgrad=amsgrad, clip=clip)
    n = opt.flat_grad.numel()
    opt.flat_grad.copy_(torch.randn(n, generator=g).to(dev))
    opt.step()
    grads = [torch.randn(n, generator=g).to(dev) for _ in range(3)]
    buffers = [opt.flat_param, opt.exp_avg, opt.exp_avg_sq, opt.step_count] + ([opt.max_exp_avg_sq] if amsgrad else [])
    saved = [b.clone() for b in buffers]
    eager = []
    for gk in grads:
        opt.flat_grad.copy_(gk)
        opt.step()
        eager.append([b.clone() for b in buffers])
    assert int(opt.step_count) == 4
    for b, s in zip(buffers, saved):
        b.copy_(s)
    torch.cuda.synchronize()
    graph, nodes = capture(opt)
    assert set(nodes) <= {"kernel", "empty"}, nodes
    assert nodes["kernel"] == plain_nodes["kernel"] + extra, (nodes, plain_nodes)
    assert torch.equal(opt.flat_param, saved[0]) and int(opt.step_count) == 1      # the capture itself ran nothing
    for k, gk in enumerate(grads):
        opt.flat_grad.copy_(gk)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager[k], buffers):
            assert torch.equal(a, b), k
    assert int(opt.step_count) == int(saved[3]) + 3
    if clip is not None and clip[0] == "norm":
        assert (opt.clip_coefs < 1).any() and (opt.clip_coefs == 1).any()


# ------------------------------------------------------------------------------------------------------------------------
# 5. the trainer's captured single-GPU step
# ------------------------------------------------------------------------------------------------------------------------
def test_trainer_captured_step_matches_torch(dev, tmp_path):
    """SimpleTrainer with OPTIMIZER: ADAM, norm clipping at the median per-parameter norm of a first, unclipped backward, six
    steps with the warm-up schedule moving the learning rate, the last ones replayed as a HIP graph with the update (and the
    step count) inside it.  For every step the CPU torch update of (state before, flat_grad after, that step's learning
    rates, that step's t) must equal the state after"""
    from test_model_gpu import make_model
    from detectron2_centernet_amd.engine.bench_train import synthetic_batch
    from detectron2_centernet_amd.engine.train_loop import SimpleTrainer
    from detectron2_centernet_amd.solver import FlatAdam

    batch = synthetic_batch(2, 128, 0, dev)
    model, cfg = make_model(tmp_path, "f16x3", seed=12, calibrated=False)
    cfg.SOLVER.IMS_PER_BATCH = 2
    tr = SimpleTrainer(model, None, cfg)
    tr.use_hip_graph = False
    tr.run_step_tensors(*batch)
    norms = torch.stack([g.norm() for g in split(tr.optimizer.flat_grad.cpu(), tr.optimizer)])
    c = float(norms[norms > 0].median())
    assert c > 0

    model, cfg = make_model(tmp_path, "f16x3", seed=12, calibrated=False)
    cfg.SOLVER.IMS_PER_BATCH = 2
    clip = ("norm", c, 2.0)
    set_adam(cfg, "ADAM", False, clip)
    tr = SimpleTrainer(model, None, cfg)
    opt = tr.optimizer
    assert isinstance(opt, FlatAdam) and opt.grad_norms is not None
    some_clipped = some_kept = False
    lrs = []
    for step in range(6):
        lr_table = opt._lr_table.clone()
        lrs.append(float(lr_table[0]))
        t = int(opt.step_count)
        assert t == step
        p0, s0 = split(opt.flat_param.cpu(), opt), state_of(opt)
        tr.run_step_tensors(*batch)
        torch.cuda.synchronize()
        grads = split(opt.flat_grad.cpu(), opt)
        hyp = hyper(opt, lr_table.cpu())
        p32, s32, _ = torch_adam_step(p0, s0, grads, hyp, t, opt, clip)
        _, s64, _ = torch_adam_step([p.double() for p in p0], [[x.double() for x in s] for s in s0], grads, hyp, t, opt, clip,
                                    torch.float64)
        compare(opt, p32, s32, s64, f"trainer step {step} ({tr.graph_state}, {int((opt.clip_coefs < 1).sum())} of "
                                    f"{len(opt.params)} parameters clipped)")
        assert not torch.equal(opt.flat_param.cpu(), torch.cat(p0))
        some_clipped |= bool((opt.clip_coefs < 1).any())
        some_kept |= bool((opt.clip_coefs == 1).any())
    assert len(set(lrs)) == 6, lrs                                   # the warm-up moved the learning rate every step
    assert tr.graph_state == "captured" and int(opt.step_count) == 6
    nodes = next(g["nodes"] for g in tr._graphs.values() if g["graph"] is not None)
    assert set(nodes) <= {"kernel", "empty"}, nodes
    assert some_clipped and some_kept


# ------------------------------------------------------------------------------------------------------------------------
# 6. two ranks on one device
# ------------------------------------------------------------------------------------------------------------------------
def _dp_worker(outdir, nsteps=4):
    import bench
    from detectron2_centernet_amd.engine.bench_train import synthetic_batch
    from detectron2_centernet_amd.engine.train_loop import SimpleTrainer
    from detectron2_centernet_amd.utils import comm

    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    model, cfg = bench.build_model("f16x3", dev, seed=5, calibrate=False)
    model.train()
    set_adam(cfg, "ADAM", False, None)
    cfg.SOLVER.BASE_LR = 1.25e-4
    tr = SimpleTrainer(model, None, cfg)
    cfg.SOLVER.IMS_PER_BATCH = 2 * tr.reducer.world
    batch = synthetic_batch(2, 128, 0, dev)        # rank argument fixed: identical data on every rank
    opt, rec = tr.optimizer, []
    for _ in range(nsteps):
        tr.run_step_tensors(*batch)
        rec.append([opt.flat_param.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.step_count.clone()])
    torch.cuda.synchronize()
    torch.save({"world": tr.reducer.world, "graph_state": tr.graph_state, "kind": type(opt).__name__,
                "steps": [[t.cpu() for t in r] for r in rec]}, os.path.join(outdir, f"rank{comm.get_rank()}.pt"))


def test_two_ranks_step_identically(dev, tmp_path):
    """the data-parallel step (forward + backward replayed, exchange, then the eager Adam launches): one result on both ranks
    after every step"""
    from detectron2_centernet_amd.engine import launch

    os.environ["CTDET_TRAIN_GRAPH"] = "1"
    try:
        launch(_dp_worker, 2, num_machines=1, machine_rank=0, dist_url="auto", args=(str(tmp_path),), backend="gloo")
    finally:
        os.environ.pop("CTDET_TRAIN_GRAPH", None)
    r0, r1 = torch.load(tmp_path / "rank0.pt"), torch.load(tmp_path / "rank1.pt")
    assert r0["world"] == r1["world"] == 2 and r0["graph_state"] == r1["graph_state"] == "captured"
    assert r0["kind"] == r1["kind"] == "FlatAdam"
    prev = None
    for step, (a, b) in enumerate(zip(r0["steps"], r1["steps"])):
        for x, y in zip(a, b):
            assert torch.equal(x, y), step
        assert all(torch.isfinite(x).all() for x in a[:3]) and int(a[3]) == step + 1
        assert a[2].abs().sum() > 0 and (prev is None or not torch.equal(prev, a[0]))
        prev = a[0]


# ------------------------------------------------------------------------------------------------------------------------
# 7. checkpoint
# ------------------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip(dev, tmp_path):
    """three trainer steps, save, load into a freshly built model + FlatAdam: one step on a fixed gradient gives the same bits
    in both"""
    from test_model_gpu import make_model
    from detectron2_centernet_amd.checkpoint import DetectionCheckpointer
    from detectron2_centernet_amd.engine.bench_train import synthetic_batch
    from detectron2_centernet_amd.engine.train_loop import SimpleTrainer
    from detectron2_centernet_amd.solver import FlatAdam, build_optimizer

    batch = synthetic_batch(2, 128, 0, dev)
    model, cfg = make_model(tmp_path, "f16x3", seed=12, calibrated=False)
    cfg.SOLVER.IMS_PER_BATCH = 2
    set_adam(cfg, "ADAMW", True, None)
    tr = SimpleTrainer(model, None, cfg)
    for _ in range(3):
        tr.run_step_tensors(*batch)
    torch.cuda.synchronize()
    a = tr.optimizer
    path = DetectionCheckpointer(model, str(tmp_path / "ckpt"), save_to_disk=True, optimizer=a).save("model_0000002", iteration=2)
    saved = torch.load(path, map_location="cpu", weights_only=False)["optimizer"]
    assert set(saved) == {"exp_avg", "exp_avg_sq", "max_exp_avg_sq", "step"} and saved["step"] == 3

    model2, cfg2 = make_model(tmp_path, "f16x3", seed=99, calibrated=False)
    set_adam(cfg2, "ADAMW", True, None)
    b = build_optimizer(cfg2, model2)
    assert isinstance(b, FlatAdam) and not torch.equal(a.flat_param, b.flat_param)
    rest = DetectionCheckpointer(model2, str(tmp_path / "ckpt"), optimizer=b).load(path)
    assert rest["iteration"] == 2 and int(b.step_count) == 3
    assert torch.equal(a.flat_param, b.flat_param) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    b.set_lr_factor(a._sched_factor)
    grad = torch.randn(a.flat_grad.numel(), generator=torch.Generator().manual_seed(8)).to(dev) * 0.01
    for o in (a, b):
        o.flat_grad.copy_(grad)
        o.step()
    for x, y in ((a.flat_param, b.flat_param), (a.exp_avg, b.exp_avg), (a.exp_avg_sq, b.exp_avg_sq),
                 (a.max_exp_avg_sq, b.max_exp_avg_sq), (a.step_count, b.step_count)):
        assert torch.equal(x, y)
    assert int(a.step_count) == 4
    with pytest.raises(KeyError, match="momentum"):
        b.load_state_dict({"momentum": torch.zeros(1), "first": False})


@pytest.mark.parametrize("amsgrad", [False, True])
def test_torch_adamw_state_loads_and_continues(dev, amsgrad):
    """a torch.optim.AdamW state dict made on the CPU after two steps loads, and the third step matches torch's third step"""
    from detectron2_centernet_amd.solver import build_optimizer

    clip = ("norm", 1.0, 2.0)
    net = small_net(dev)
    opt = build_optimizer(small_cfg("ADAMW", amsgrad, clip), net)
    hyp = hyper(opt, opt._lr_table.cpu())
    mine = {id(p): i for i, p in enumerate(opt.params)}
    module_order = [mine[id(p)] for p in net.parameters()]              # module index -> index in opt.params
    gen = torch.Generator().manual_seed(2100)
    scales = list(reversed(SCALES))
    all_grads = [[torch.randn(n, generator=gen) * s for (_, n), s in zip(opt.offsets, scales)] for _ in range(3)]
    chains = {}
    for dtype in (torch.float32, torch.float64):
        ps = [torch.nn.Parameter(opt.params[i].detach().cpu().reshape(-1).to(dtype)) for i in module_order]
        ref = torch.optim.AdamW([{"params": [p], "lr": hyp[i][0], "weight_decay": hyp[i][1]} for p, i in zip(ps, module_order)],
                                lr=1.0, amsgrad=amsgrad, foreach=False)

        def ref_step(k, ps=ps, ref=ref, dtype=dtype):
            for p, i in zip(ps, module_order):
                p.grad = all_grads[k][i].clone().to(dtype)
                torch.nn.utils.clip_grad_norm_(p, clip[1], clip[2])
            ref.step()

        ref_step(0)
        ref_step(1)
        chains[dtype] = (ps, ref, ref_step)
    ps, ref, ref_step = chains[torch.float32]
    for p, i in zip(ps, module_order):
        opt.params[i].data.copy_(p.detach().view_as(opt.params[i]).to(dev))
    opt.load_state_dict(ref.state_dict())
    assert int(opt.step_count) == 2
    for p, i in zip(ps, module_order):
        off, n = opt.offsets[i]
        assert torch.equal(opt.exp_avg[off:off + n].cpu(), ref.state[p]["exp_avg"])
        assert torch.equal(opt.exp_avg_sq[off:off + n].cpu(), ref.state[p]["exp_avg_sq"])
    opt.flat_grad.copy_(torch.cat(all_grads[2]).to(dev))
    opt.step()
    names = ["exp_avg", "exp_avg_sq"] + (["max_exp_avg_sq"] if amsgrad else [])
    out = {}
    for dtype, (ps, ref, ref_step) in chains.items():
        ref_step(2)
        by_mine = {i: p for p, i in zip(ps, module_order)}
        order = [by_mine[i] for i in range(len(opt.params))]
        out[dtype] = ([p.detach() for p in order], [[ref.state[p][k] for p in order] for k in names])
    compare(opt, out[torch.float32][0], out[torch.float32][1], out[torch.float64][1], f"AdamW amsgrad={amsgrad} third step after loading")
    assert int(opt.step_count) == 3
