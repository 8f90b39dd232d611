"""SOLVER.CLIP_GRADIENTS / SOLVER.NESTEROV on the GPU: the flat step against the reference's own optimizer (G21), against torch
at DLA-34's full size, its determinism, its capture into a HIP graph, and the trainer's single-GPU and two-rank steps.

Tolerance of every parameter / momentum comparison: the project's own for this kernel, atol 1e-6 + rtol 1e-6
(test_hip_ops.test_sgd_matches_torch).  The per-parameter norms are reduced in another order than torch's (f32 partials of
4096 elements); a CPU restatement of that order, a 2.36 M-element parameter included, stayed below 0.08 of the bound over four
steps."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ATOL = RTOL = 1e-6

# tests/golden/make_g21.py: name -> (CLIP_TYPE or None, CLIP_VALUE, NORM_TYPE, NESTEROV)
G21_CASES = {"nesterov": (None, 0.0, 2.0, True)}
for _name, (_kind, _value, _norm) in {"value": ("value", 0.5, 2.0), "norm2": ("norm", 1.0, 2.0), "norm1": ("norm", 1.0, 1.0),
                                      "norminf": ("norm", 0.3, math.inf)}.items():
    G21_CASES[_name] = (_kind, _value, _norm, False)
    G21_CASES[_name + "_nesterov"] = (_kind, _value, _norm, True)


def close(a, b):
    return torch.allclose(a, b, atol=ATOL, rtol=RTOL)


def worst(a, b):
    """largest |a - b| in units of the bound atol + rtol * |b|"""
    return ((a - b).abs() / (ATOL + RTOL * b.abs())).max().item()


def set_clip(cfg, kind, value, norm=2.0, nesterov=False):
    cfg.SOLVER.NESTEROV = nesterov
    if kind is not None:
        cfg.SOLVER.CLIP_GRADIENTS.ENABLED = True
        cfg.SOLVER.CLIP_GRADIENTS.CLIP_TYPE, cfg.SOLVER.CLIP_GRADIENTS.CLIP_VALUE = kind, value
        cfg.SOLVER.CLIP_GRADIENTS.NORM_TYPE = norm


def hyper(opt, lr_table):
    """per parameter (in the order of opt.params): (learning rate as the kernel reads it, weight decay)"""
    out = []
    for off, _ in opt.offsets:
        run = next(r for r in opt.runs if r[0] <= off < r[1] or (r[0] == r[1] == off))
        out.append((float(lr_table[opt.lr_factors.index(run[2])]), run[3]))
    return out


def split(flat, opt):
    return [flat[off:off + n].clone() for off, n in opt.offsets]


def torch_step(params, moms, grads, hyp, momentum, nesterov, clip, first):
    """one step of the reference's optimizer on the CPU, from torch alone: every parameter clipped on its own
    (torch.nn.utils.clip_grad_norm_ / clip_grad_value_ called with ONE tensor), then torch.optim.SGD.
    Returns (parameters, momentum buffers, norms or None) after the step."""
    ps = [torch.nn.Parameter(p.clone()) for p in params]
    opt = torch.optim.SGD([{"params": [p], "lr": lr, "weight_decay": wd} for p, (lr, wd) in zip(ps, hyp)], lr=1.0,
                          momentum=momentum, nesterov=nesterov, foreach=False)
    norms = []
    for p, m, g in zip(ps, moms, grads):
        p.grad = g.clone()
        if not first:
            opt.state[p]["momentum_buffer"] = m.clone()
        if clip is not None and clip[0] == "norm":
            norms.append(torch.nn.utils.clip_grad_norm_(p, clip[1], clip[2]))
        elif clip is not None:
            torch.nn.utils.clip_grad_value_(p, clip[1])
    opt.step()
    return [p.detach() for p in ps], [opt.state[p]["momentum_buffer"] for p in ps], (torch.stack(norms) if norms else None)


# ------------------------------------------------------------------------------------------------------------------------
# 1. G21: the reference's own build_optimizer
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(G21_CASES))
def test_g21_reference_optimizer(dev, case):
    """`build_optimizer` from the config the reference got reproduces the reference's parameters and momentum buffers after
    each of its four steps (SGDWithGradientClip: per-parameter clipping, two learning rates, three weight decays)"""
    from detectron2_centernet_amd.config import get_cfg
    from detectron2_centernet_amd.solver import build_optimizer

    gold = np.load(os.path.join(HERE, "golden", "g21_clip_sgd.npz"))
    kind, value, norm, nesterov = G21_CASES[case]
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3), torch.nn.BatchNorm2d(8), torch.nn.Conv2d(8, 5, 1))
    params = list(net.parameters())
    numels = gold["numels"].tolist()
    assert [p.numel() for p in params] == numels
    bounds = np.concatenate([[0], np.cumsum(numels)])
    pieces = lambda flat: [torch.from_numpy(flat[a:b].copy()) for a, b in zip(bounds[:-1], bounds[1:])]   # noqa: E731
    for p, v in zip(params, pieces(gold["init"])):
        p.data.copy_(v.view_as(p))
    net.to(dev)
    cfg = get_cfg()
    cfg.SOLVER.BASE_LR, cfg.SOLVER.BIAS_LR_FACTOR, cfg.SOLVER.WEIGHT_DECAY_BIAS = 0.02, 2.0, 0.0
    set_clip(cfg, kind, value, norm, nesterov)
    opt = build_optimizer(cfg, net)
    assert len(opt.runs) >= 3 and len(opt.lr_factors) == 2
    where = {id(p): opt.offsets[i] for i, p in enumerate(opt.params)}
    wp = wm = 0.0
    for step in range(gold["grads"].shape[0]):
        opt.zero_grad()
        for p, g in zip(params, pieces(gold["grads"][step])):
            p.grad.copy_(g.view_as(p).to(dev))
        before = opt.flat_grad.clone()
        opt.step()
        assert torch.equal(opt.flat_grad, before)            # the clipped gradient is not written back
        for p, wantp, wantm in zip(params, pieces(gold[case + "_params"][step]), pieces(gold[case + "_mom"][step])):
            off, n = where[id(p)]
            gotp, gotm = p.detach().reshape(-1).cpu(), opt.flat_mom[off:off + n].cpu()
            wp, wm = max(wp, worst(gotp, wantp)), max(wm, worst(gotm, wantm))
            assert close(gotp, wantp) and close(gotm, wantm), (case, step, worst(gotp, wantp), worst(gotm, wantm))
        if kind == "norm":       # the recorded coefficients clip exactly the parameter-steps the reference's norms clip
            got = [bool(opt.clip_coefs[[id(q) for q in opt.params].index(id(p))] < 1) for p in params]
            assert got == gold[case + "_clipped"][step].tolist()
    print(f"G21 {case}: worst parameter / momentum error {wp:.3f} / {wm:.3f} of the bound")


# ------------------------------------------------------------------------------------------------------------------------
# 2. + 3. full size
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dla34(dev):
    import bench

    model, cfg = bench.build_model("f16x3", dev, seed=3, calibrate=False)
    return model, cfg


def full_size_grads(opt, clip, step, c):
    """randn * s_i, u_i alternating 0.25 and 4: parameter i's norm (value mode: its typical |g|) is about u_i * c"""
    g = torch.Generator().manual_seed(2200 + step)
    out = []
    for i, (_, n) in enumerate(opt.offsets):
        u = 0.25 if i % 2 == 0 else 4.0
        if clip[0] == "value":
            s = u * c
        elif clip[2] == 2:
            s = u * c / math.sqrt(n)
        elif clip[2] == 1:
            s = u * c / (n * math.sqrt(2 / math.pi))                       # E|x| of a normal
        else:
            s = u * c / max(1.0, math.sqrt(2 * math.log(n)))               # about the largest of n normals
        out.append(torch.randn(n, generator=g) * s)
    return out


FULL_CASES = [(("norm", 1.0, 2.0), False), (("norm", 1.0, 2.0), True), (("norm", 2.0, 1.0), False),
              (("norm", 0.5, math.inf), True), (("value", 0.01), False), (("value", 0.01), True)]


@pytest.mark.parametrize("clip,nesterov", FULL_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_full_size_against_torch(dev, dla34, clip, nesterov):
    """DLA-34's real parameter list (about 18.6 M elements, about 109 runs): three steps against per-parameter
    clip_grad_norm_ / clip_grad_value_ + torch.optim.SGD on the CPU; `grad_norms` against f64 norms, within four times the
    distance of torch's own f32 norms from them (plus 1e-6, relative)"""
    from detectron2_centernet_amd.solver import build_optimizer

    model, cfg = dla34
    cfg = cfg.clone()
    set_clip(cfg, clip[0], clip[1], clip[2] if len(clip) > 2 else 2.0, nesterov)
    opt = build_optimizer(cfg, model)
    total = opt.flat_param.numel()
    assert total > 18e6 and len(opt.runs) > 50 and max(n for _, n in opt.offsets) == 512 * 512 * 9
    opt.set_lr_factor(0.37)
    hyp = hyper(opt, opt._lr_table.cpu())
    params, moms = split(opt.flat_param.cpu(), opt), split(opt.flat_mom.cpu(), opt)
    P = len(opt.params)
    for step in range(3):
        grads = full_size_grads(opt, clip, step, clip[1])
        opt.flat_grad.copy_(torch.cat(grads).to(dev))
        opt.step()
        params, moms, norms32 = torch_step(params, moms, grads, hyp, opt.momentum, nesterov, clip, step == 0)
        gotp, gotm = opt.flat_param.cpu(), opt.flat_mom.cpu()
        wantp, wantm = torch.cat(params), torch.cat(moms)
        print(f"{clip} nesterov={nesterov} step {step}: parameter / momentum error {worst(gotp, wantp):.3f} / "
              f"{worst(gotm, wantm):.3f} of the bound")
        assert close(gotp, wantp) and close(gotm, wantm)
        if clip[0] == "norm":
            norms64 = torch.stack([torch.linalg.vector_norm(g.double(), clip[2]) for g in grads])
            clipped = int((clip[1] / (norms64 + 1e-6) < 1).sum())
            assert abs(clipped - P / 2) <= 0.15 * P, (clipped, P)          # half the parameters clipped, half not
            torch_rel = ((norms32.double() - norms64).abs() / norms64).max().item()
            got_rel = ((opt.grad_norms.cpu().double() - norms64).abs() / norms64).max().item()
            print(f"  norms: relative distance from f64 {got_rel:.3e}, torch's f32 norms {torch_rel:.3e}; {clipped} of {P} clipped")
            assert got_rel <= 4 * torch_rel + 1e-6, (got_rel, torch_rel)
            want_coef = torch.clamp(clip[1] / (norms64 + 1e-6), max=1.0)
            assert torch.equal(opt.clip_coefs.cpu() < 1, want_coef < 1)
            assert torch.allclose(opt.clip_coefs.cpu().double(), want_coef, rtol=4 * torch_rel + 1e-6, atol=0)
        else:
            frac = (torch.cat(grads).abs() > clip[1]).float().mean().item()
            assert 0.2 < frac < 0.8, frac
            assert opt.grad_norms is None and opt.clip_coefs is None


@pytest.mark.parametrize("clip,nesterov", [(("norm", 1.0, 2.0), True), (("norm", 2.0, 1.0), False), (("norm", 0.5, math.inf), False),
                                           (("value", 0.01), True)], ids=lambda v: str(v).replace(" ", ""))
def test_full_size_step_is_deterministic(dev, dla34, clip, nesterov):
    """the same state and gradients stepped twice: identical bits in parameters, momentum, norms and coefficients (no float
    atomics anywhere in the reduction)"""
    from detectron2_centernet_amd.solver import build_optimizer

    model, cfg = dla34
    cfg = cfg.clone()
    set_clip(cfg, clip[0], clip[1], clip[2] if len(clip) > 2 else 2.0, nesterov)
    opt = build_optimizer(cfg, model)
    opt.flat_grad.copy_(torch.cat(full_size_grads(opt, clip, 0, clip[1])).to(dev))
    opt.step()                                                    # past the first step: the momentum buffer is read
    opt.flat_grad.copy_(torch.cat(full_size_grads(opt, clip, 1, clip[1])).to(dev))
    p0, m0 = opt.flat_param.clone(), opt.flat_mom.clone()
    runs = []
    for _ in range(2):
        opt.flat_param.copy_(p0)
        opt.flat_mom.copy_(m0)
        if opt.grad_norms is not None:
            opt.grad_norms.fill_(-1.0)
            opt.clip_coefs.fill_(-1.0)
        opt.step()
        runs.append([opt.flat_param.clone(), opt.flat_mom.clone()] +
                    ([opt.grad_norms.clone(), opt.clip_coefs.clone()] if opt.grad_norms is not None else []))
    assert not torch.equal(runs[0][0], p0)
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    if opt.grad_norms is not None:
        assert (runs[0][2] > 0).all() and (runs[0][3] > 0).all() and (runs[0][3] <= 1).all()


# ------------------------------------------------------------------------------------------------------------------------
# 4. capture
# ------------------------------------------------------------------------------------------------------------------------
def _small_optimizer(dev, clip, nesterov):
    from detectron2_centernet_amd.solver.build import FlatSGD

    g = torch.Generator().manual_seed(44)
    lens = [1, 255, 256, 257, 3, 70001, 1, 1, 4096, 9, 300000]
    groups = [(torch.nn.Parameter(torch.randn(n, generator=g).to(dev)), 1.0 + (i % 2), 1e-4 * (i % 3)) for i, n in enumerate(lens)]
    opt = FlatSGD(groups, 0.05, 0.9, nesterov=nesterov, clip=clip)
    return opt, g


@pytest.mark.parametrize("clip,nesterov,extra", [(None, True, 0), (("value", 0.5), False, 0), (("value", 0.5), True, 0),
                                                 (("norm", 20.0, 2.0), False, 2), (("norm", 300.0, 1.0), True, 2),
                                                 (("norm", 2.0, math.inf), False, 2)], ids=lambda v: str(v).replace(" ", ""))
def test_step_captures_as_kernels_only(dev, clip, nesterov, extra):
    """`optimizer.step()` captured alone and replayed == the eager call, bit for bit; the graph holds kernels only, as many as
    the plain step's plus two in norm mode and plus none otherwise"""
    from detectron2_centernet_amd.engine import graph_nodes

    def capture(opt):
        graph = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(graph):
            opt.step()
        nodes = graph_nodes.node_types(graph.raw_cuda_graph())
        graph.instantiate()
        return graph, nodes

    plain, g = _small_optimizer(dev, None, False)
    plain.flat_grad.copy_(torch.randn(plain.flat_grad.numel(), generator=g).to(dev))
    plain.step()
    torch.cuda.synchronize()
    _, plain_nodes = capture(plain)
    assert set(plain_nodes) <= {"kernel", "empty"}

    opt, g = _small_optimizer(dev, clip, nesterov)
    opt.flat_grad.copy_(torch.randn(opt.flat_grad.numel(), generator=g).to(dev))
    opt.step()                                                    # the first step: the graph below bakes first_step = 0
    opt.flat_grad.copy_(torch.randn(opt.flat_grad.numel(), generator=g).to(dev))
    p0, m0 = opt.flat_param.clone(), opt.flat_mom.clone()
    opt.step()
    eager = [opt.flat_param.clone(), opt.flat_mom.clone()] + ([opt.grad_norms.clone(), opt.clip_coefs.clone()] if extra else [])
    opt.flat_param.copy_(p0)
    opt.flat_mom.copy_(m0)
    if extra:
        opt.grad_norms.zero_()
        opt.clip_coefs.zero_()
    torch.cuda.synchronize()
    graph, nodes = capture(opt)
    assert set(nodes) <= {"kernel", "empty"}, nodes
    assert nodes["kernel"] == plain_nodes["kernel"] + extra, (nodes, plain_nodes)
    assert torch.equal(opt.flat_param, p0)                        # the capture itself ran nothing
    graph.replay()
    torch.cuda.synchronize()
    replayed = [opt.flat_param, opt.flat_mom] + ([opt.grad_norms, opt.clip_coefs] if extra else [])
    for a, b in zip(eager, replayed):
        assert torch.equal(a, b)
    assert not torch.equal(opt.flat_param, p0)
    if extra:
        assert (opt.clip_coefs < 1).any() and (opt.clip_coefs == 1).any()


# ------------------------------------------------------------------------------------------------------------------------
# 5. the trainer's captured single-GPU step
# ------------------------------------------------------------------------------------------------------------------------
def test_trainer_captured_step_clips_like_torch(dev, tmp_path):
    """SimpleTrainer on the small DLA model, norm clipping at the median per-parameter norm of a first, unclipped backward (so
    about half the parameters clip), Nesterov on: six steps, the last ones replayed as a HIP graph with the update inside it.
    For every step the CPU torch update of (parameters and momentum before, flat_grad after, the step's learning rates) must
    equal the parameters after -- independent of backward's run-to-run noise."""
    from test_model_gpu import make_model
    from detectron2_centernet_amd.engine.bench_train import synthetic_batch
    from detectron2_centernet_amd.engine.train_loop import SimpleTrainer

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
    set_clip(cfg, *clip, nesterov=True)
    tr = SimpleTrainer(model, None, cfg)
    opt = tr.optimizer
    assert opt.nesterov and opt.grad_norms is not None
    some_clipped = some_kept = False
    for step in range(6):
        lr_table = opt._lr_table.clone()
        p0, m0 = opt.flat_param.clone(), opt.flat_mom.clone()
        tr.run_step_tensors(*batch)
        torch.cuda.synchronize()
        grads = split(opt.flat_grad.cpu(), opt)
        wantp, wantm, _ = torch_step(split(p0.cpu(), opt), split(m0.cpu(), opt), grads, hyper(opt, lr_table.cpu()), opt.momentum,
                                     True, clip, step == 0)
        gotp, gotm = opt.flat_param.cpu(), opt.flat_mom.cpu()
        wantp, wantm = torch.cat(wantp), torch.cat(wantm)
        print(f"step {step} ({tr.graph_state}): parameter / momentum error {worst(gotp, wantp):.3f} / {worst(gotm, wantm):.3f} "
              f"of the bound; {int((opt.clip_coefs < 1).sum())} of {len(opt.params)} parameters clipped")
        assert close(gotp, wantp) and close(gotm, wantm), step
        assert not torch.equal(gotp, p0.cpu())
        some_clipped |= bool((opt.clip_coefs < 1).any())
        some_kept |= bool((opt.clip_coefs == 1).any())
    assert tr.graph_state == "captured"
    nodes = next(g["nodes"] for g in tr._graphs.values() if g["graph"] is not None)
    assert set(nodes) <= {"kernel", "empty"}, nodes
    assert some_clipped and some_kept


# ------------------------------------------------------------------------------------------------------------------------
# 6. two ranks on one device
# ------------------------------------------------------------------------------------------------------------------------
def _dp_steps(outfile, nsteps=4):
    import bench
    from detectron2_centernet_amd.engine.bench_train import synthetic_batch
    from detectron2_centernet_amd.engine.train_loop import SimpleTrainer

    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    model, cfg = bench.build_model("f16x3", dev, seed=5, calibrate=False)
    model.train()
    set_clip(cfg, "norm", float(os.environ["CTDET_TEST_CLIP_VALUE"]), 2.0, nesterov=False)
    tr = SimpleTrainer(model, None, cfg)
    cfg.SOLVER.IMS_PER_BATCH = 2 * tr.reducer.world
    batch = synthetic_batch(2, 128, 0, dev)        # rank argument fixed: identical data on every rank
    opt, rec = tr.optimizer, []
    for _ in range(nsteps):
        tr.run_step_tensors(*batch)
        rec.append([opt.flat_param.clone(), opt.flat_mom.clone(), opt.grad_norms.clone(), opt.clip_coefs.clone()])
    torch.cuda.synchronize()
    torch.save({"world": tr.reducer.world, "graph_state": tr.graph_state, "steps": [[t.cpu() for t in r] for r in rec]}, outfile)


def _dp_worker(outdir):
    from detectron2_centernet_amd.utils import comm

    _dp_steps(os.path.join(outdir, f"rank{comm.get_rank()}.pt"))


def test_two_ranks_clip_the_averaged_gradient_identically(dev, tmp_path):
    """the data-parallel step (forward + backward replayed, exchange, then the update): clipping sees the averaged gradient,
    one result on both ranks after every step; some parameters clip and others do not on the recorded steps"""
    import bench
    from detectron2_centernet_amd.engine import launch
    from detectron2_centernet_amd.engine.bench_train import synthetic_batch
    from detectron2_centernet_amd.engine.train_loop import SimpleTrainer

    # the clip value: the median per-parameter norm of one unclipped backward of the same model and batch
    model, cfg = bench.build_model("f16x3", dev, seed=5, calibrate=False)
    model.train()
    cfg.SOLVER.IMS_PER_BATCH = 2
    tr = SimpleTrainer(model, None, cfg)
    tr.use_hip_graph = False
    tr.run_step_tensors(*synthetic_batch(2, 128, 0, dev))
    norms = torch.stack([g.norm() for g in split(tr.optimizer.flat_grad.cpu(), tr.optimizer)])
    del tr, model
    os.environ["CTDET_TEST_CLIP_VALUE"] = repr(float(norms[norms > 0].median()))
    os.environ["CTDET_TRAIN_GRAPH"] = "1"
    try:
        launch(_dp_worker, 2, num_machines=1, machine_rank=0, dist_url="auto", args=(str(tmp_path),), backend="gloo")
    finally:
        os.environ.pop("CTDET_TRAIN_GRAPH", None)
        os.environ.pop("CTDET_TEST_CLIP_VALUE", None)
    r0, r1 = torch.load(tmp_path / "rank0.pt"), torch.load(tmp_path / "rank1.pt")
    assert r0["world"] == r1["world"] == 2 and r0["graph_state"] == r1["graph_state"] == "captured"
    for step, (a, b) in enumerate(zip(r0["steps"], r1["steps"])):
        for x, y in zip(a, b):
            assert torch.equal(x, y), step
        coefs = a[3]
        assert (coefs < 1).any() and (coefs == 1).any(), step
        assert torch.isfinite(a[0]).all()
