"""SyncBatchNorm on the GPU: the split BatchNorm kernels (ctdet_bn_local_stats / _sync_fwd / _local_grad_sums / _sync_bwd),
ops_train.SyncBNActFn over a real process group, and the training step of a ctdet_res_18_bot_1x-shaped model (trainable
SyncBN in res3 / res4) -- two ranks share the device over gloo, as tests/test_dp_gpu.py does -- against float64 references
whose BatchNorm statistics span both ranks' tensors."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from oracle import ctdet_oracle as O
from oracle import model_ref as MR

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ot():
    assert torch.cuda.is_available()
    import detectron2_centernet_amd.ops_train as m
    return m


def rel_err(got, ref):
    err = (got.double() - ref).abs().max().item()
    return err / max(1e-30, ref.abs().max().item())


def _bn_ref(ys, gamma, beta, res, relu, dzs, eps=1e-5, zk=None):
    """f64 BatchNorm over the union of the ranks' rows ([M_r, C] each): outputs, input gradients (dy, dres = g), the
    rank-local (sum g, sum g*xhat), running-stat targets.  zk: the kernels' outputs, whose ReLU mask the backward uses (as
    the kernels do: an output within rounding of 0 may sit on either side)"""
    y = torch.cat([t.double() for t in ys])
    M = y.shape[0]
    mean = y.mean(0)
    var = (y - mean).square().mean(0)
    invstd = 1.0 / torch.sqrt(var + eps)
    out = {"mean": mean, "var": var, "invstd": invstd, "M": M, "z": [], "g": [], "local": []}
    for r, yr in enumerate(ys):
        xh = (yr.double() - mean) * invstd
        z = xh * gamma.double() + beta.double()
        if res is not None:
            z = z + res[r].double()
        if relu:
            z = z.clamp(min=0.0)
        out["z"].append(z)
    gs = []
    for r, dz in enumerate(dzs):
        g = dz.double() * ((out["z"][r] if zk is None else zk[r]) > 0) if relu else dz.double()
        xh = (ys[r].double() - mean) * invstd
        gs.append(g)
        out["local"].append((g.sum(0), (g * xh).sum(0)))
    s0 = sum(l[0] for l in out["local"])
    s1 = sum(l[1] for l in out["local"])
    out["dy"] = [(gamma.double() * invstd) * (g - s0 / M - (ys[r].double() - mean) * invstd * (s1 / M)) for r, g in enumerate(gs)]
    out["g"] = gs
    return out


def _case_tensors(Ms, C, dt, dev, seed, shifted, res):
    g = torch.Generator(device=dev).manual_seed(seed)
    if shifted:
        mu, sd = torch.linspace(0.0, 10.0, C, device=dev), torch.linspace(1.0, 0.1, C, device=dev)
    else:
        mu, sd = torch.full((C,), 0.5, device=dev), torch.full((C,), 2.0, device=dev)
    # the second rank's rows have other statistics (what makes per-rank BatchNorm differ from SyncBN)
    ys = [(torch.randn(M, C, generator=g, device=dev) * sd * (1 + r) + mu + 0.7 * r).to(dt).view(1, 1, M, C)
          for r, M in enumerate(Ms)]
    rs = [torch.randn(M, C, generator=g, device=dev).to(dt).view(1, 1, M, C) for M in Ms] if res else None
    dzs = [torch.randn(M, C, generator=g, device=dev).to(dt).view(1, 1, M, C) for M in Ms]
    gamma = torch.rand(C, generator=g, device=dev) + 0.5
    beta = torch.randn(C, generator=g, device=dev)
    return ys, rs, dzs, gamma, beta


# (rank row counts, channels, residual, relu, shifted means); 1024 partial blocks need M >= 1024 * 8 * rows per pass
CASES = {"unequal_64": ((3000, 1200), 64, True, True, False),
         "one_row_rank": ((777, 1), 128, False, True, False),
         "partial_blocks_1024": ((300000, 70000), 16, False, False, False),
         "non_pow2_vectors_96": ((513, 2049), 96, True, False, False),
         "non_pow2_vectors_24": ((100, 37), 24, False, True, False),
         "shifted_mean": ((200000, 50000), 16, False, False, True)}


@pytest.mark.parametrize("dt", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("name", list(CASES))
def test_split_kernels_two_simulated_ranks(ot, name, dt):
    """local stats of each rank into its slot, the slot buffers summed (the all-reduce), then the per-rank sync forward /
    backward: z, dy, dres and the running stats against f64 BatchNorm over cat(y0, y1); dgamma / dbeta against the LOCAL
    sums; both ranks' running stats bit-identical"""
    dev = torch.device("cuda:0")
    Ms, C, res, relu, shifted = CASES[name]
    if dt == torch.float16 and shifted:
        pytest.skip("f16 tensors keep the fused kernels' plain sums; the shifted-mean bound is an f32 property")
    ys, rs, dzs, gamma, beta = _case_tensors(Ms, C, dt, dev, sum(Ms) + C, shifted, res)
    W = len(Ms)
    stats = sum(ot.bn_local_stats(y, r, W) for r, y in enumerate(ys))
    for r in range(W):     # the slots of the other ranks are written with zeros, not left alone
        one = ot.bn_local_stats(ys[r], r, W)
        assert torch.count_nonzero(torch.cat([one[q] for q in range(W) if q != r])).item() == 0
        assert one[r, 0].eq(Ms[r]).all()
    outs = []
    for r in range(W):
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        z, mean, invstd, scale = ot.bn_sync_fwd(ys[r], stats, gamma, beta, rm, rv, 1e-5, 0.1,
                                                res=rs[r] if res else None, relu=relu)
        sums, dgamma, dbeta = ot.bn_local_grad_sums(dzs[r], z, ys[r], mean, invstd, r, W, relu=relu, grad_mult=1.0)
        outs.append(dict(z=z, mean=mean, invstd=invstd, scale=scale, rm=rm, rv=rv, sums=sums, dgamma=dgamma, dbeta=dbeta))
    gsum = sum(o["sums"] for o in outs)
    for r in range(W):
        o = outs[r]
        o["dy"], o["dres"] = ot.bn_sync_bwd(dzs[r], o["z"], ys[r], o["mean"], o["invstd"], o["scale"], stats, gsum, relu=relu,
                                            want_dres=res)
    ref = _bn_ref([y.view(-1, C) for y in ys], gamma, beta, [t.view(-1, C) for t in rs] if res else None, relu,
                  [d.view(-1, C) for d in dzs], zk=[o["z"].view(-1, C) for o in outs])
    f32 = dt == torch.float32
    tf, tb = (2e-6, 2e-5) if f32 else (4e-3, 2e-2)
    M = ref["M"]
    for r in range(W):
        o = outs[r]
        assert torch.equal(o["rm"], outs[0]["rm"]) and torch.equal(o["rv"], outs[0]["rv"]) and torch.equal(o["mean"], outs[0]["mean"])
        errs = {"invstd": (rel_err(o["invstd"], ref["invstd"]), 2e-6),
                "z": (rel_err(o["z"].view(-1, C), ref["z"][r]), tf),
                "running_mean": (rel_err(o["rm"], 0.1 * ref["mean"]), 1e-5),
                "running_var": (rel_err(o["rv"], 0.9 + 0.1 * ref["var"] * M / (M - 1)), 1e-5),
                "dbeta_local": (rel_err(o["dbeta"], ref["local"][r][0]), tb),
                "dgamma_local": (rel_err(o["dgamma"], ref["local"][r][1]), tb),
                "dy": (rel_err(o["dy"].view(-1, C), ref["dy"][r]), tb)}
        for k, (e, tol) in errs.items():
            print(f"{name} {dt} rank {r} {k}: rel err {e:.2e} (bound {tol:.0e})")
        bad = {k: f"{e:.2e} > {tol:.0e}" for k, (e, tol) in errs.items() if not e <= tol}
        assert not bad, (r, bad)
        if res:
            assert torch.equal(o["dres"].view(-1, C).double(), ref["g"][r].to(dt).double())


@pytest.mark.parametrize("dt", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("C", [64, 96, 256])
def test_one_slot_equals_fused_kernels(ot, dt, C):
    """world 1: the split kernels give the fused ctdet_bn_train_fwd / _bwd results bit for bit -- the same statistics
    (the single slot is taken as it stands), the same apply expressions -- except dy, bounded here instead: on f16 tensors
    the two kernels' f32 arithmetic before the f16 rounding of dy is not evaluated identically by the compiler (measured:
    differences of f16 rounding size, f32 tensors bit-identical).  The f32 bound at channel-vector counts that are not powers
    of two dates from when the fused generic apply kernel multiplied xhat * sum * (1/M); all three apply kernels now share
    bn_bwd_elem's xhat * (sum/M), and tests/test_bn_gpu.py::test_world_one_equals_fused asserts f32 dy bit for bit."""
    dev = torch.device("cuda:0")
    ys, rs, dzs, gamma, beta = _case_tensors((5000,), C, dt, dev, C, False, True)
    y, r0, dz = ys[0], rs[0], dzs[0]
    rm1, rv1, rm2, rv2 = torch.zeros(C, device=dev), torch.ones(C, device=dev), torch.zeros(C, device=dev), torch.ones(C, device=dev)
    zf, mf, isf, scf = ot.bn_train_fwd(y, gamma, beta, rm1, rv1, 1e-5, 0.1, res=r0, relu=True)
    stats = ot.bn_local_stats(y, 0, 1)
    zs, ms, iss, scs = ot.bn_sync_fwd(y, stats, gamma, beta, rm2, rv2, 1e-5, 0.1, res=r0, relu=True)
    for a, b in ((zf, zs), (mf, ms), (isf, iss), (scf, scs), (rm1, rm2), (rv1, rv2)):
        assert torch.equal(a, b)
    dyf, dresf, dgf, dbf = ot.bn_train_bwd(dz, zf, y, mf, isf, scf, relu=True, want_dres=True, grad_mult=0.25)
    sums, dgs, dbs = ot.bn_local_grad_sums(dz, zs, y, ms, iss, 0, 1, relu=True, grad_mult=0.25)
    dys, dress = ot.bn_sync_bwd(dz, zs, y, ms, iss, scs, stats, sums, relu=True, want_dres=True)
    assert torch.equal(dgf, dgs) and torch.equal(dbf, dbs) and torch.equal(dresf, dress)
    cv = C // (4 if dt == torch.float32 else 8)
    if cv & (cv - 1) == 0 and dt == torch.float32:
        assert torch.equal(dyf, dys)
    else:
        assert rel_err(dys.view(-1, C), dyf.view(-1, C).double()) <= (1e-6 if dt == torch.float32 else 2e-3)


def test_empty_rank_batch_is_rejected(ot):
    dev = torch.device("cuda:0")
    y = torch.zeros(0, 1, 1, 64, device=dev)
    with pytest.raises(RuntimeError, match="empty batch"):
        ot.bn_local_stats(y, 1, 2)


# ------------------------------------------------------------------------------------------ SyncBNActFn, two ranks
_FN_M = (2900, 700)
_FN_C = 64


def _fn_worker(outdir, dt_name):
    import torch.distributed as dist
    import detectron2_centernet_amd.ops_train as ot

    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    rank = dist.get_rank()
    dt = getattr(torch, dt_name)
    ot.PARAM_GRAD_MULT = 1.0
    ys, rs, dzs, gamma, beta = _case_tensors(_FN_M, _FN_C, dt, dev, 11, False, True)
    y = ys[rank].clone().requires_grad_(True)
    res = rs[rank].clone().requires_grad_(True)
    gm, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rm, rv = torch.zeros(_FN_C, device=dev), torch.ones(_FN_C, device=dev)
    z = ot.SyncBNActFn.apply(y, gm, bt, res, rm, rv, 1e-5, 0.1, True)
    z.backward(dzs[rank])
    torch.cuda.synchronize()
    torch.save({k: v.detach().cpu() for k, v in dict(z=z, dy=y.grad, dres=res.grad, dgamma=gm.grad, dbeta=bt.grad, rm=rm,
                                                       rv=rv).items()}, os.path.join(outdir, f"fn{rank}.pt"))


@pytest.mark.parametrize("dt_name", ["float32", "float16"])
def test_sync_bn_act_fn_two_ranks(tmp_path, dt_name):
    from detectron2_centernet_amd.engine import launch

    launch(_fn_worker, 2, num_machines=1, machine_rank=0, dist_url="auto", args=(str(tmp_path), dt_name), backend="gloo")
    dev = torch.device("cuda:0")
    dt = getattr(torch, dt_name)
    ys, rs, dzs, gamma, beta = _case_tensors(_FN_M, _FN_C, dt, dev, 11, False, True)
    C = _FN_C
    out = [torch.load(tmp_path / f"fn{r}.pt") for r in range(2)]
    ref = _bn_ref([y.view(-1, C).cpu() for y in ys], gamma.cpu(), beta.cpu(), [t.view(-1, C).cpu() for t in rs], True,
                  [d.view(-1, C).cpu() for d in dzs], zk=[o["z"].view(-1, C) for o in out])
    assert torch.equal(out[0]["rm"], out[1]["rm"]) and torch.equal(out[0]["rv"], out[1]["rv"])
    tf, tb = (2e-6, 2e-5) if dt == torch.float32 else (4e-3, 2e-2)
    M = ref["M"]
    for r in range(2):
        o = out[r]
        assert rel_err(o["z"].view(-1, C), ref["z"][r]) <= tf
        assert rel_err(o["dy"].view(-1, C), ref["dy"][r]) <= tb
        assert torch.equal(o["dres"].view(-1, C).double(), ref["g"][r].to(dt).double())
        assert rel_err(o["dgamma"], ref["local"][r][1]) <= tb and rel_err(o["dbeta"], ref["local"][r][0]) <= tb
        assert rel_err(o["rm"], 0.1 * ref["mean"]) <= 1e-5
        assert rel_err(o["rv"], 0.9 + 0.1 * ref["var"] * M / (M - 1)) <= 1e-5


# ------------------------------------------------------------------------------------------ training steps (res_18_bot)
def _bot_model(tmpdir, precision, seed=21):
    import shutil
    from detectron2_centernet_amd.config import get_cfg
    from detectron2_centernet_amd.data.catalog import register_synthetic
    from detectron2_centernet_amd.modeling import build_model
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from weights import fill_state_dict

    shutil.copy(os.path.join(HERE, "golden", "g16_configs", "Base-CenterNet.yaml"), os.path.join(tmpdir, "Base-CenterNet.yaml"))
    shutil.copy(os.path.join(HERE, "golden", "g17_configs", "ctdet_res_18_bot_1x.yaml"), os.path.join(tmpdir, "bot.yaml"))
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(tmpdir, "bot.yaml"))
    cfg.MODEL.CENTERNET.HIP_PRECISION = precision
    register_synthetic(cfg.DATASETS.TRAIN[0], num_classes=1)
    model = build_model(cfg)
    sd = fill_state_dict({k: v.cpu() for k, v in model.state_dict().items()}, seed=seed)
    model.load_state_dict({k: v.to(model.device) for k, v in sd.items()})
    return model.train(), cfg, sd


# per rank: (images, size); rank 1's images are darker and of lower contrast -- other BatchNorm statistics
RANK_BATCH = {0: (2, 128), 1: (2, 96)}


def _rank_batch(rank, dev):
    from detectron2_centernet_amd.engine.bench_train import synthetic_batch
    B, size = RANK_BATCH[rank]
    imgs, boxes, classes, counts = synthetic_batch(B, size, rank, dev, num_classes=1, max_boxes=8)
    if rank == 1:
        imgs = (imgs.float() * 0.35 + 20).to(torch.uint8)
    return imgs, boxes, classes, counts


def _step_worker(outdir, precision):
    import torch.distributed as dist
    from detectron2_centernet_amd.engine.train_loop import SimpleTrainer

    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    rank = dist.get_rank() if dist.is_initialized() else 0
    model, cfg, sd = _bot_model(outdir, precision)
    tr = SimpleTrainer(model, None, cfg)
    batch = _rank_batch(rank, dev)
    losses = tr.run_step_tensors(*batch)
    torch.cuda.synchronize()
    names = {id(p): n for n, p in model.named_parameters()}
    rec = {"losses": {k: float(v) for k, v in losses.items()}, "grad": tr.optimizer.flat_grad.cpu().clone(),
           "layout": [(names[id(p)], off, n) for p, (off, n) in zip(tr.optimizer.params, tr.optimizer.offsets)],
           "graph_ddp": tr.graph_ddp, "world": tr.reducer.world}
    tr.run_step_tensors(*batch)
    tr.run_step_tensors(*batch)
    torch.cuda.synchronize()
    rec.update(param=tr.optimizer.flat_param.cpu().clone(), buffers={k: v.cpu().clone() for k, v in model.named_buffers()},
               graph_state=tr.graph_state, graphs=len(tr._graphs))
    if rank == 0:
        torch.save(sd, os.path.join(outdir, "sd0.pt"))
    torch.save(rec, os.path.join(outdir, f"step{rank}.pt"))


def _ref_step(sd0, cfg_mean, cfg_std, batches, trainable, sync=True):
    """CPU f64 autograd of the res_18_bot model: frozen stem / res2 (FrozenBN), res3 / res4 conv + BatchNorm whose
    statistics span every rank's tensors (sync) or only the rank's own (the negative control), per-GPU BatchNorm in the
    deconv layers, heads and losses per rank; total (L_0 + ... ) / world.  Returns (per-rank losses, {name: grad})."""
    sd = {k: (v.double().clone().requires_grad_(k in trainable) if v.dtype.is_floating_point else v) for k, v in sd0.items()}

    def bn(xs, p):
        if not sync:
            return [F.batch_norm(x, None, None, sd[p + ".weight"], sd[p + ".bias"], True, 0.1, 1e-5) for x in xs]
        flat = torch.cat([x.permute(1, 0, 2, 3).reshape(x.shape[1], -1) for x in xs], dim=1)
        mean = flat.mean(1)
        var = (flat - mean[:, None]).square().mean(1)
        sc = sd[p + ".weight"] / torch.sqrt(var + 1e-5)
        sh = sd[p + ".bias"] - mean * sc
        return [x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1) for x in xs]

    def conv(xs, p, stride, pad):
        return [F.conv2d(x, sd[p + ".weight"], None, stride, pad) for x in xs]

    feats = []
    for imgs, _, _, _ in batches:
        x, _ = O.preprocess(list(imgs.cpu()), cfg_mean, cfg_std, 32)
        x = x.double()
        x = F.relu(MR._conv_norm(sd, "backbone.stem.conv1", x, 2, 3))
        x = F.max_pool2d(x, kernel_size=3, stride=2, padding=1)
        for bi in range(2):
            x = MR.basic_res_block(sd, f"backbone.res2.{bi}", x, 1)
        feats.append(x)
    for st in (3, 4):
        for bi in range(2):
            p = f"backbone.res{st}.{bi}"
            stride = 2 if bi == 0 else 1
            out = [F.relu(t) for t in bn(conv(feats, p + ".conv1", stride, 1), p + ".conv1.norm")]
            out = bn(conv(out, p + ".conv2", 1, 1), p + ".conv2.norm")
            sc = bn(conv(feats, p + ".shortcut", stride, 0), p + ".shortcut.norm") if (p + ".shortcut.weight") in sd else feats
            feats = [F.relu(o + s) for o, s in zip(out, sc)]
    losses, total = [], 0.0
    for (imgs, boxes, classes, counts), f in zip(batches, feats):
        y = MR.deconv_layers(sd, "deconv_layers", f, training=True)
        z = MR.centernet_heads(MR.Net(sd), y)
        H, W = imgs.shape[2] // 4, imgs.shape[3] // 4
        targets = [O.gen_heatmap(boxes[b, :int(counts[b])].cpu(), classes[b, :int(counts[b])].cpu(), H, W, 1)
                   for b in range(imgs.shape[0])]
        l = MR.centernet_losses(z, targets, [1.0])
        losses.append({k: v.item() for k, v in l.items()})
        total = total + sum(l.values())
    (total / len(batches)).backward()
    return losses, {k: sd[k].grad for k in trainable}


def _grad_checks(rec, grads, cos_min, ratio_tol, only=None):
    """[(name, cos, norm ratio)] of the parameters whose check fails"""
    bad = []
    for name, off, n in rec["layout"]:
        if only is not None and not only(name):
            continue
        gref = grads[name]
        if gref is None or gref.abs().max() == 0:
            continue
        got = rec["grad"][off:off + n].double()
        cos = F.cosine_similarity(got, gref.flatten(), dim=0).item()
        ratio = (got.norm() / gref.norm()).item()
        if not (cos >= cos_min and abs(ratio - 1) <= ratio_tol):
            bad.append((name, round(cos, 5), round(ratio, 4)))
    return bad


BOUNDS = {"f32": (1e-3, 0.999, 0.01), "f16x3": (1e-3, 0.999, 0.01), "f16": (1e-2, 0.98, 0.10)}


@pytest.mark.parametrize("precision", ["f32", "f16x3", "f16"])
def test_two_rank_bot_training_step_matches_f64_sync_reference(tmp_path, precision):
    """two ranks, different images of different sizes and statistics: each rank's losses and the exchanged gradient against
    CPU f64 autograd with BatchNorm statistics over both ranks; after three steps (all eager: trainable SyncBN at world 2
    never captures) parameters and every buffer (running stats, num_batches_tracked) are bit-identical on both ranks.
    f32: the same reference with per-rank statistics fails on the res3 / res4 norm gradients (negative control)."""
    from detectron2_centernet_amd.engine import launch

    launch(_step_worker, 2, num_machines=1, machine_rank=0, dist_url="auto", args=(str(tmp_path), precision), backend="gloo")
    recs = [torch.load(tmp_path / f"step{r}.pt") for r in range(2)]
    sd0 = torch.load(tmp_path / "sd0.pt")
    for r in recs:
        assert r["world"] == 2 and not r["graph_ddp"] and r["graph_state"] == "eager" and r["graphs"] == 0
    assert torch.equal(recs[0]["grad"], recs[1]["grad"]) and torch.equal(recs[0]["param"], recs[1]["param"])
    # the backbone's buffers (SyncBN running stats and counters, FrozenBN) agree bit for bit; the deconv layers' BatchNorms
    # are per-GPU (centernet.py:_make_deconv_layer), their running statistics follow each rank's own images
    for k, v in recs[0]["buffers"].items():
        if k.startswith("backbone."):
            assert torch.equal(v, recs[1]["buffers"][k]), k
    assert not torch.equal(recs[0]["buffers"]["deconv_layers.1.running_mean"], recs[1]["buffers"]["deconv_layers.1.running_mean"])
    assert int(recs[0]["buffers"]["backbone.res3.0.conv1.norm.num_batches_tracked"]) == 3
    trainable = {n for n, _, _ in recs[0]["layout"]}
    assert any(".norm." in n and n.startswith("backbone.res3") for n in trainable)
    batches = [_rank_batch(r, torch.device("cpu")) for r in range(2)]
    mean, std = [0.408, 0.447, 0.470], [0.289, 0.274, 0.278]
    losses, grads = _ref_step(sd0, mean, std, batches, trainable, sync=True)
    ltol, cmin, rtol = BOUNDS[precision]
    for r in range(2):
        for k, want in losses[r].items():
            got = recs[r]["losses"][k]
            print(precision, r, k, got, want)
            assert abs(got - want) <= ltol * max(1.0, abs(want)), (r, k, got, want)
    bad = _grad_checks(recs[0], grads, cmin, rtol)
    assert not bad, bad
    if precision == "f32":
        _, grads_local = _ref_step(sd0, mean, std, batches, trainable, sync=False)
        bn_param = lambda n: n.startswith(("backbone.res3", "backbone.res4")) and ".norm." in n
        wrong = _grad_checks(recs[0], grads_local, cmin, rtol, only=bn_param)
        print("per-rank statistics reference fails on", len(wrong), wrong[:6])
        assert wrong, "the test cannot tell SyncBN from per-GPU BatchNorm"


@pytest.mark.parametrize("precision", ["f32", "f16x3", "f16"])
def test_single_gpu_bot_step_matches_f64_and_captures(tmp_path, precision):
    """world 1: trainable res3 / res4 BatchNorm on the fused kernels; the first (eager) step against the f64 reference; from
    the third call on the step is one captured graph of kernel nodes only, whose losses follow an eager trainer's"""
    from detectron2_centernet_amd.engine.train_loop import SimpleTrainer

    dev = torch.device("cuda:0")
    d1, d2 = tmp_path / "a", tmp_path / "b"
    d1.mkdir(), d2.mkdir()
    model, cfg, sd0 = _bot_model(str(d1), precision)
    tr = SimpleTrainer(model, None, cfg)
    assert tr.sync_bn and tr.reducer.world == 1 and tr.graph_ddp
    batch = _rank_batch(0, dev)
    losses = {k: float(v) for k, v in tr.run_step_tensors(*batch).items()}
    torch.cuda.synchronize()
    names = {id(p): n for n, p in model.named_parameters()}
    rec = {"grad": tr.optimizer.flat_grad.cpu().clone(),
           "layout": [(names[id(p)], off, n) for p, (off, n) in zip(tr.optimizer.params, tr.optimizer.offsets)]}
    ref_losses, grads = _ref_step(sd0, [0.408, 0.447, 0.470], [0.289, 0.274, 0.278], [_rank_batch(0, torch.device("cpu"))],
                                  {n for n, _, _ in rec["layout"]})
    ltol, cmin, rtol = BOUNDS[precision]
    for k, want in ref_losses[0].items():
        assert abs(losses[k] - want) <= ltol * max(1.0, abs(want)), (k, losses[k], want)
    bad = _grad_checks(rec, grads, cmin, rtol)
    assert not bad, bad
    os.environ["CTDET_TRAIN_GRAPH"] = "0"
    try:
        model_e, cfg_e, _ = _bot_model(str(d2), precision)
        tr_e = SimpleTrainer(model_e, None, cfg_e)
    finally:
        os.environ.pop("CTDET_TRAIN_GRAPH", None)
    tr_e.run_step_tensors(*batch)
    for _ in range(3):
        got = tr.run_step_tensors(*batch)
        want = tr_e.run_step_tensors(*batch)
    torch.cuda.synchronize()
    assert tr.graph_state == "captured" and tr_e.graph_state == "eager"
    for g in tr._graphs.values():
        if g["graph"] is not None:
            assert g["nodes"].get("kernel", 0) > 0 and set(g["nodes"]) <= {"kernel", "empty"}, g["nodes"]
    tol = 1e-3 if precision == "f16" else 1e-4
    for k in got:
        a, b = float(got[k]), float(want[k])
        assert abs(a - b) <= tol * max(1.0, abs(b)), (k, a, b)
    assert int(model.backbone.res3[0].conv1.norm.num_batches_tracked) == 4
