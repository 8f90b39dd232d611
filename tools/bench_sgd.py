#!/usr/bin/env python
"""Dev tool: time the flat SGD update on DLA-34's parameter layout (about 18.6 M elements, 109 runs, ~300 parameters) for
{plain, nesterov, value, norm-2, norm-1, norm-inf} and the flat Adam step (advance + update) for {adam, adamw, adam-amsgrad,
adam norm-2} -- 200 warm launches, 1000 timed, device events -- and print microseconds,
achieved GB/s from the bytes a variant must move (the SGD update: 3 reads + 2 writes of 4 B per element; Adam: 4 + 3, with
AMSGrad 5 + 4; the norm pass: one more read) and the share of the HBM bound.  The variants alternate over --rounds, so that a
drift of the machine shows as spread inside a variant; every line also gives the variant's GB/s over the plain SGD case's of
the same round.  Not part of the product or of the tests.

  --lib PATH     an additional "plain" case through another build of libctdet_hip.so (the plain case calls
                 ctdet_sgd_momentum_runs alone, which every build of ABI 8 has): A/B of the plain path against a parent build
  --train-step   instead: the f16x3 DLA-34 training step (16 x 512^2, engine/bench_train.py's step), a fresh trainer per leg,
                 legs alternating: SGD with norm clipping off / on, or with --adam SGD / ADAM (no clipping), or with --ema SGD
                 with SOLVER.EMA off / on
  --ema          instead: the EMA update alone (advance + the lerp over the flat parameters + the lerp over the BatchNorm
                 statistics) next to the plain SGD launch, on the same layout; 12 B per parameter (e and p read, e written)"""
import argparse
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from detectron2_centernet_amd import _lib, ops  # noqa: E402
from detectron2_centernet_amd.solver.build import FlatAdam, FlatSGD, param_groups  # noqa: E402

HBM_PEAK = 8.0e12      # bytes / s (MI355X)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=1000)
ap.add_argument("--warm", type=int, default=200)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--lib", default=None)
ap.add_argument("--train-step", action="store_true")
ap.add_argument("--adam", action="store_true", help="--train-step: the legs are SGD / ADAM instead of norm clipping off / on")
ap.add_argument("--ema", action="store_true", help="the EMA update alone; with --train-step: the legs are SOLVER.EMA off / on")
ap.add_argument("--steps", type=int, default=40, help="--train-step: timed steps per leg")
a = ap.parse_args()
dev = torch.device("cuda:0")


def timed(f, warm, reps):
    for _ in range(warm):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3      # us


def train_step_legs():
    from detectron2_centernet_amd.engine.bench_train import synthetic_batch
    from detectron2_centernet_amd.engine.train_loop import SimpleTrainer

    batch = synthetic_batch(16, 512, 0, dev)
    for leg in range(2 * a.rounds):
        on = leg % 2 == 1
        model, cfg = bench.build_model("f16x3", dev, seed=1)
        model.train()
        cfg.SOLVER.IMS_PER_BATCH = 16
        if a.ema:
            cfg.SOLVER.EMA.ENABLED = on
        elif on and a.adam:
            cfg.SOLVER.OPTIMIZER = "ADAM"
            cfg.SOLVER.BASE_LR = 1.25e-4 * 16 / 32
        elif on:
            cfg.SOLVER.CLIP_GRADIENTS.ENABLED = True
            cfg.SOLVER.CLIP_GRADIENTS.CLIP_TYPE, cfg.SOLVER.CLIP_GRADIENTS.CLIP_VALUE = "norm", 1.0
        tr = SimpleTrainer(model, None, cfg)
        ms = timed(lambda: tr.run_step_tensors(*batch), 8, a.steps) / 1e3
        if a.ema:
            print(f"train step f16x3 16x512^2, SOLVER.EMA {'on ' if on else 'off'}: {ms:.3f} ms / step  ({tr.graph_state}"
                  f"{f', {int(tr.ema.updates)} updates' if on else ''})", flush=True)
            del tr, model
            continue
        if a.adam:
            print(f"train step f16x3 16x512^2, {type(tr.optimizer).__name__:8s}: {ms:.3f} ms / step  ({tr.graph_state}"
                  f"{f', step count {int(tr.optimizer.step_count)}' if on else ''})", flush=True)
            del tr, model
            continue
        clipped = int((tr.optimizer.clip_coefs < 1).sum()) if on else 0
        print(f"train step f16x3 16x512^2, norm clipping {'on ' if on else 'off'}: {ms:.3f} ms / step  ({tr.graph_state}"
              f"{f', {clipped} parameters clipped in the last step' if on else ''})", flush=True)
        del tr, model


def ema_cases():
    """the EMA update on DLA-34's layout, alternating with the plain SGD launch as the yardstick of the same round"""
    from detectron2_centernet_amd.solver.ema import ModelEMA

    model, cfg = bench.build_model("f16x3", dev, calibrate=False)
    model.train()
    opt = FlatSGD(param_groups(cfg, model), 0.01, 0.9)
    ema = ModelEMA(model, opt)
    n, ns = opt.flat_param.numel(), sum(k for _, _, k, _ in ema.table.buffers)
    grad = torch.randn(n, generator=torch.Generator().manual_seed(0)).to(dev) * 1e-3

    def plain():
        ops.sgd_momentum_runs_(opt.flat_param, grad, opt.flat_mom, opt._run_end, opt._run_lr_index, opt._run_wd, opt._lr_table,
                               0.9, False)

    def params_only():
        ops.ema_lerp_segments_(ema._param_ptrs, ema.ema_param, ema._param_start, n, ema.weight)

    def stats_only():
        ops.ema_lerp_segments_(ema._stat_ptrs, ema.ema_stats, ema._stat_start, ema._stat_max, ema.weight)

    cases = [("plain SGD launch", plain, 20 * n), ("EMA update (3 launches)", ema.update, 12 * (n + ns)),
             ("EMA lerp, parameters alone", params_only, 12 * n), ("EMA lerp, statistics alone", stats_only, 12 * ns)]
    print(f"{n} parameters in one segment, {ns} statistics in {ema._stat_ptrs.numel()} segments; {a.warm} warm + {a.reps} timed "
          "launches per case and round")
    for r in range(a.rounds):
        for name, f, by in cases:
            us = timed(f, a.warm, a.reps)
            print(f"round {r}  {name:28s} {us:8.2f} us  {by / us / 1e3:8.1f} GB/s  {by / HBM_PEAK * 1e6 / us * 100:5.1f} % of the "
                  f"HBM bound ({by / 1e6:.1f} MB)", flush=True)


def main():
    if a.train_step:
        return train_step_legs()
    if a.ema:
        return ema_cases()
    model, cfg = bench.build_model("f16x3", dev, calibrate=False)
    groups = param_groups(cfg, model)
    variants = {"plain": (False, None), "nesterov": (True, None), "value": (False, ("value", 0.01)),
                "norm-2": (False, ("norm", 1.0, 2.0)), "norm-1": (False, ("norm", 1.0, 1.0)),
                "norm-inf": (False, ("norm", 1.0, float("inf")))}
    opts = {k: FlatSGD(groups, 0.01, 0.9, nesterov=n, clip=c) for k, (n, c) in variants.items()}
    # name: (decoupled, amsgrad, clip, bytes per element)
    adam_variants = {"adam": (False, False, None, 28), "adamw": (True, False, None, 28), "adam-amsgrad": (False, True, None, 36),
                     "adam norm-2": (False, False, ("norm", 1.0, 2.0), 32)}
    adams = {k: FlatAdam(groups, 1e-4, decoupled=d, amsgrad=m, clip=c) for k, (d, m, c, _) in adam_variants.items()}
    n = opts["plain"].flat_param.numel()
    g = torch.Generator().manual_seed(0)
    # per-parameter scale alternating around the L2 clip value, so that about half the parameters clip
    grad = torch.cat([torch.randn(k, generator=g) * ((0.25 if i % 2 else 4.0) / k ** 0.5)
                      for i, (_, k) in enumerate(opts["plain"].offsets)]).to(dev)

    def raw_plain(path):
        h = ctypes.CDLL(path)
        fn = h.ctdet_sgd_momentum_runs
        fn.restype, fn.argtypes = _lib.SIGNATURES["ctdet_sgd_momentum_runs"]
        o = opts["plain"]
        args = [ctypes.c_void_p(t.data_ptr()) for t in (o.flat_param, grad, o.flat_mom)] + [n] + \
               [ctypes.c_void_p(t.data_ptr()) for t in (o._run_end, o._run_lr_index, o._run_wd, o._lr_table)] + \
               [o._run_end.numel(), 0.9, 0]

        def f():
            rc = fn(*args, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0, rc
        return f

    def variant(o):
        norm = o._clip_type == _lib.CLIP_NORM

        def f():
            if norm:
                ops.grad_chunk_norms_(grad, o._chunk_start, o._chunk_len, o._norm_type, o._partials)
                ops.grad_clip_coefs_(o._partials, o._param_chunk_end, o._norm_type, o._clip_value, o.grad_norms, o.clip_coefs)
            ops.sgd_momentum_runs_clip_(o.flat_param, grad, o.flat_mom, o._run_end, o._run_lr_index, o._run_wd, o._lr_table,
                                        0.9, False, o.nesterov, o._clip_type, o._clip_value, o.clip_coefs)
        return f

    def adam_variant(o):
        def f():
            ops.adam_advance_(o.step_count, o._bias, *o.betas)
            if o._clip_type == _lib.CLIP_NORM:
                ops.grad_chunk_norms_(grad, o._chunk_start, o._chunk_len, o._norm_type, o._partials)
                ops.grad_clip_coefs_(o._partials, o._param_chunk_end, o._norm_type, o._clip_value, o.grad_norms, o.clip_coefs)
            ops.adam_runs_(o.flat_param, grad, o.exp_avg, o.exp_avg_sq, o.max_exp_avg_sq, o._run_end, o._run_lr_index, o._run_wd,
                           o._lr_table, o._bias, o.betas[0], o.betas[1], o.eps, o.decoupled, o.amsgrad, o._clip_type,
                           o._clip_value, o.clip_coefs)
        return f

    def norm_pass(o):
        def f():
            ops.grad_chunk_norms_(grad, o._chunk_start, o._chunk_len, o._norm_type, o._partials)
            ops.grad_clip_coefs_(o._partials, o._param_chunk_end, o._norm_type, o._clip_value, o.grad_norms, o.clip_coefs)
        return f

    cases = [("plain", raw_plain(_lib.LIB_PATH), 20)]
    if a.lib:
        cases.append((f"plain [{os.path.basename(os.path.dirname(a.lib)) or a.lib}]", raw_plain(a.lib), 20))
    cases += [(k, variant(opts[k]), 24 if k.startswith("norm") else 20) for k in list(variants)[1:]]
    cases.append(("norm-2 pass alone", norm_pass(opts["norm-2"]), 4))
    cases += [(k, adam_variant(adams[k]), adam_variants[k][3]) for k in adam_variants]
    print(f"{n} elements, {len(opts['plain'].runs)} runs, {len(groups)} parameters, {opts['norm-2']._chunk_start.numel()} chunks; "
          f"{a.warm} warm + {a.reps} timed launches per case and round")
    for r in range(a.rounds):
        plain_rate = None
        for name, f, bpe in cases:
            us = timed(f, a.warm, a.reps)
            by = bpe * n
            plain_rate = plain_rate or by / us           # the first case is plain SGD
            print(f"round {r}  {name:28s} {us:8.2f} us  {by / us / 1e3:8.1f} GB/s  {by / HBM_PEAK * 1e6 / us * 100:5.1f} % of the "
                  f"HBM bound ({by / 1e6:.0f} MB)  {by / us / plain_rate:5.3f} of plain's GB/s", flush=True)


main()
