"""Host-side wrappers over the C ABI: torch tensors are used only as device-memory handles
(data_ptr + shape); every computation below happens in libctdet_hip.so on the current HIP stream.

Activation convention: NHWC tensors ``[B, H, W, C]`` that may be channel-slices of a wider NHWC
buffer (that is how Root's ``torch.cat`` (reference dla.py:88) is made free: producers write straight
into their slice of the concat buffer).
"""
import ctypes as C
import os
import math

import numpy as np
import torch

from . import _lib
from ._lib import (ACT_NONE, ACT_RELU, ACT_SIGMOID_CLAMP, DCN_MASK_LOGIT, DCN_MASK_NONE, DCN_MASK_PROB, F16, F16X3, F32, U8,
                   ConvDesc, HeadDesc)

_TORCH_DT = {F16: torch.float16, F32: torch.float32}

# bench.py's roofline leg: when PROFILE_ON, every conv-shaped launch is bracketed by HIP events on the
# launch stream and (kernel label as the launcher gave it, algorithmic FLOPs, start, end, algorithmic bytes, info, repetitions) is
# appended to PROFILE.
PROFILE_ON = False
PROFILE = []
PROFILE_REP = 5   # each profiled launch is issued this many times back to back between one event pair


class _Prof:
    def __init__(self, p, M, deform, out_dt, nsrc=1, flops=None):
        self.on = PROFILE_ON
        if self.on:
            _lib.lib().ctdet_set_label_mode(1)      # the launcher names the kernel instantiation it launches: done() reads it
            self.flops = flops if flops is not None else 2.0 * M * p.Cout * p.R * p.S * p.Cin_real
            osz = 2 if out_dt == F16 else 4
            if p is not None:   # algorithmic bytes: input once + output once (+ offsets/masks for the deformable conv)
                isz = 2 if p.compute == F16 else 4
                in_px = M * (p.stride * p.stride if not deform else 1)
                self.bytes = in_px * p.Cin_real * isz + M * p.Cout * osz + (M * 27 * 4 if deform else 0) + p.Cout_pad * p.Kpad * isz
                self.info = f"M={M} {p.Cin_real}->{p.Cout} k{p.R} s{p.stride}" + (" dcn" if deform else "") + (f" cat{nsrc}" if nsrc > 1 else "")
            else:
                self.bytes, self.info = 0.0, f"M={M}"
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def reps(self):
        return PROFILE_REP if self.on else 1

    def done(self):
        if self.on:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            name = _lib.lib().ctdet_last_kernel_label().decode()
            _lib.lib().ctdet_set_label_mode(0)
            PROFILE.append((name, self.flops, self.e0, e1, self.bytes, self.info, PROFILE_REP))


class prof_region:
    """`with prof_region(name, flops=, nbytes=):` brackets the launches inside with HIP events on the launch stream when
    PROFILE_ON (bench.py's live per-kernel timing of the decode and of the training step); free otherwise."""

    def __init__(self, name, flops=0.0, nbytes=0.0, info=""):
        self.rec = (name, flops, nbytes, info) if PROFILE_ON else None

    def __enter__(self):
        if self.rec is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if self.rec is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            name, flops, nbytes, info = self.rec
            PROFILE.append((name, flops, self.e0, e1, nbytes, info, 1))
        return False


# CTDET_RANGE_CHECK=1 (debug): after every f16x3 / f16 contraction the output's largest magnitude is read back and a value the
# NEXT layer cannot carry raises.  f16x3 holds an activation as hi + lo with hi = f16(x): beyond 65504 hi is inf, the layer's
# sums become inf / NaN -- and the ReLU of the epilogue (fmaxf) turns NaN into 0, so the network's outputs stay finite and
# wrong.  The check costs a host synchronisation per layer, so the eval engines run eagerly (no graph) while it is on.
RANGE_CHECK = os.environ.get("CTDET_RANGE_CHECK", "0") == "1"
F16_MAX = 65504.0


def _range_check(out, p, what):
    if RANGE_CHECK and p.compute in (F16, F16X3):
        amax = out.detach().float().abs().amax().item()
        if not (amax <= F16_MAX):
            raise FloatingPointError(f"{what}: output magnitude {amax:.4g} leaves the range the {'f16x3' if p.compute == F16X3 else 'f16'} "
                                     f"mode can carry into the next layer (|x| <= {F16_MAX:.0f}; Cin={p.Cin_real}, Cout={p.Cout}, k={p.R})")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _require_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            # same contract as the reference's native op (deform_conv.py:203-204): no CPU implementation
            raise NotImplementedError("the CenterNet HIP path has no CPU implementation; tensors must be on a ROCm device")


def _nhwc_stride(t):
    """pixel stride (elements) of an NHWC tensor or channel-slice view; validates the layout."""
    assert t.dim() == 4, f"expected NHWC 4-D tensor, got {tuple(t.shape)}"
    B, H, W, Cc = t.shape
    s = t.stride()
    ps = s[2] if W > 1 else (s[1] if H > 1 else (s[0] if B > 1 else Cc))
    if Cc > 1:
        assert s[3] == 1, "channel dim must be contiguous"
    assert ps >= Cc
    if W > 1 and H > 1:
        assert s[1] == W * ps, "rows must be dense"
    if B > 1 and H > 1:
        assert s[0] == H * W * ps, "images must be dense"
    return ps


def dt_of(t):
    if t.dtype == torch.float16:
        return F16
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.uint8:
        return U8
    raise TypeError(f"unsupported dtype {t.dtype}")


def round_up(a, b):
    return (a + b - 1) // b * b


def flip_taps(w):
    """w.flip(2, 3) of an OIHW weight; a 1x1 weight is returned as it is (torch's flip of size-1 dimensions is a plain copy, a
    hipMemcpyAsync: see kpad)"""
    return w if w.shape[2] * w.shape[3] == 1 else w.flip(2, 3)


def kpad(t, pad, value=0.0):
    """torch.nn.functional.pad(t, pad, value=value) for padding after the END of dimensions (pad = (0, n_last, 0, n_before_last,
    ...)), made of kernels only.  F.pad is fill + narrow().copy_(), and a contiguous narrow (a 1-D vector, dimension 0 of a
    weight) is copied by hipMemcpyAsync: a memcpy node in a captured step, which must hold kernels only (engine/graph_nodes.py)"""
    for i in range(0, len(pad), 2):
        assert pad[i] == 0, "kpad pads after the end of a dimension only"
        n, dim = int(pad[i + 1]), t.dim() - 1 - i // 2
        if n:
            shape = list(t.shape)
            shape[dim] = n
            t = torch.cat([t, t.new_full(shape, value)], dim)
    return t


class PackPlan:
    """The packed operands of every conv weight a training step packs (forward and input-gradient forms; f16 images and the
    split f16x3 images with their row scales), kept in persistent buffers and refreshed by ONE kernel per kind after the
    optimizer update (`run()`, called by solver.FlatSGD.step) instead of one pack launch per layer, direction and step.  An entry
    is valid while the weight's version counter still has the value `run()` (or the recording pack) saw; a stale or unknown
    weight is packed on the spot as before and (re)recorded."""

    def __init__(self, flat_param):
        """flat_param: the optimizer's parameter buffer -- only weights that live inside it are planned (their address is
        stable and their version counter is the parameter's; a temporary could reuse an address with a fresh counter).

        A captured training step holds raw pointers to every entry's packed buffer (its conv kernels) and to the descriptor
        table (its pack launch), so neither may ever be freed or moved while the plan lives: a stale entry is re-packed INTO
        its buffer (`repack`), a table that the entry set outgrew is retired, not dropped."""
        self.lo = flat_param.data_ptr()
        self.hi = self.lo + flat_param.numel() * flat_param.element_size()
        self.entries = {}        # key -> [weight, packed, args, version, scale buffer (f16x3 entries) or None]
        self.table = {0: None, 1: None}     # device descriptor tables (f16 / f16x3), rebuilt when the set of entries changes
        self.blocks = {0: 0, 1: 0}
        self._retired = []       # earlier tables: a captured graph may still launch the pack kernel on them

    def covers(self, weight):
        return self.lo <= weight.data_ptr() < self.hi

    def lookup(self, key, weight):
        e = self.entries.get(key)
        if e is not None and e[3] == weight._version:
            return e[1] if e[4] is None else (e[1], e[4])
        return None

    def stale_buffer(self, key):
        """the packed buffer (f16x3: the (buffer, scale) pair) of a known entry whose weight has changed since it was packed
        (None: unknown key)"""
        e = self.entries.get(key)
        if e is None:
            return None
        return e[1] if e[4] is None else (e[1], e[4])

    def record(self, key, weight, packed, args, scale=None):
        e = self.entries.get(key)
        if e is not None:                      # re-packed in place: same buffer, same table
            assert e[1].data_ptr() == packed.data_ptr()
            e[0], e[3] = weight, weight._version
            return
        self.entries[key] = [weight, packed, args, weight._version, scale]
        kind = 0 if scale is None else 1
        if self.table[kind] is not None:
            self._retired.append(self.table[kind])
        self.table[kind] = None

    def _build(self, kind, es):
        if kind == 0:
            arr = (_lib.PackDesc * len(es))()
            blk = 0
            for d, (w, wp, a, _, _) in zip(arr, es):
                d.w, d.packed = w.data_ptr(), wp.data_ptr()
                d.O, d.I, d.R, d.S, d.chans_pad, d.rows_pad, d.Kpad, d.korder, d.transposed = a
                d.blk0 = blk
                blk += (d.rows_pad * d.Kpad + 255) // 256
        else:
            arr = (_lib.Pack3Desc * len(es))()
            blk = 0
            for d, (w, wp, a, _, sc) in zip(arr, es):
                d.w, d.packed, d.scale_out = w.data_ptr(), wp.data_ptr(), sc.data_ptr()
                d.O, d.I, d.R, d.S, d.chans_pad, d.rows_pad, d.Kpad, d.layout, d.transposed, d.scale_n = a
                d.blk0 = blk
                blk += d.rows_pad
        raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
        self.table[kind], self.blocks[kind] = raw.to(es[0][1].device), blk

    def run(self):
        for kind in (0, 1):
            es = [e for e in self.entries.values() if (e[4] is None) == (kind == 0)]
            if not es:
                continue
            if self.table[kind] is None:
                self._build(kind, es)
            fn = _lib.lib().ctdet_pack_weights_batch if kind == 0 else _lib.lib().ctdet_pack_weights_x3_batch
            _lib.check(fn(_ptr(self.table[kind]), len(es), self.blocks[kind], _stream()), "ctdet_pack_weights_batch")
            for e in es:
                e[3] = e[0]._version


PACK_PLAN = None    # set by solver.FlatSGD on a GPU; None: every PackedConv packs for itself


def pack_x3(weight, args):
    """(packed f32-viewed image [rows_pad, Kpad], row scale [scale_n]) of ctdet_pack_weights_x3 for the f32 contiguous parameter
    `weight`; args = (O, I, R, S, chans_pad, rows_pad, Kpad, layout, transposed, scale_n).  Planned (persistent buffers, refreshed
    by the batched pack after every optimizer step) when the weight lives in the optimizer's flat buffer."""
    rows_pad, Kpad, scale_n = args[5], args[6], args[9]
    key = ("x3",) + tuple(args) + (weight.data_ptr(),)
    plan = PACK_PLAN if (PACK_PLAN is not None and PACK_PLAN.covers(weight)) else None
    bufs = plan.lookup(key, weight) if plan is not None else None
    if bufs is None:
        bufs = plan.stale_buffer(key) if plan is not None else None
        if bufs is None:
            bufs = (torch.empty(rows_pad, Kpad, dtype=torch.float32, device=weight.device),
                    torch.empty(scale_n, dtype=torch.float32, device=weight.device))
        rc = _lib.lib().ctdet_pack_weights_x3(_ptr(weight), _ptr(bufs[0]), _ptr(bufs[1]), *args, _stream())
        _lib.check(rc, "ctdet_pack_weights_x3")
        if plan is not None:
            plan.record(key, weight, bufs[0], tuple(args), scale=bufs[1])
    return bufs


class PackedConv:
    """Weights of one conv-shaped contraction, packed for the kernels, plus its folded epilogue.

    weight: [Cout, Cin, R, S] (PyTorch OIHW, the reference's parameter layout).
    scale/bias: per-output-channel f32 epilogue (folded BatchNorm and/or conv bias) or None.
    compute: F16 (f16 tensors, f16 MFMA), F32 (f32 tensors, f32 MFMA: the reference's arithmetic) or F16X3 (f32 tensors,
    every product as three f16 products on the f16 matrix pipe: ctdet_conv_desc in include/ctdet_hip.h).
    """

    def __init__(self, weight, scale=None, bias=None, stride=1, pad=0, dil=1, compute=F16, cin_pad=None,
                 tap_major=False, transposed=False, cout_align=None):
        """transposed: pack the input-gradient operand of `weight` (rows = its input channels, taps flipped) -- the
        conv that maps dY to dX; f16 / f16x3.  cout_align: pad the packed rows to a multiple of this (the DCNv2 window kernel
        works on 64-cout tiles whatever Cout is)."""
        _require_cuda(weight)
        # transposed = "dcn_cols" / "dcn_cols_chunked": the operand of DCNv2's d(columns) contraction for a [O, I, 3, 3] weight,
        # a 1x1 conv from dY's O channels to 9*I column channels (ctdet_pack_weights transposed = 2 / 3)
        dcn_mode = {"dcn_cols": 2, "dcn_cols_chunked": 3}[transposed] if isinstance(transposed, str) else 0
        if dcn_mode:
            assert compute in (F16, F16X3) and scale is None and bias is None and weight.dtype == torch.float32 and weight.is_contiguous()
            assert tuple(weight.shape[2:]) == (3, 3) and not tap_major
            Cin, Cout, R, S = weight.shape[0], 9 * weight.shape[1], 1, 1
        elif transposed:
            assert compute in (F16, F16X3) and scale is None and bias is None
            assert compute == F16 or (weight.dtype == torch.float32 and weight.is_contiguous())
            Cin, Cout, R, S = weight.shape
        else:
            Cout, Cin, R, S = weight.shape
        self.Cout, self.R, self.S = Cout, R, S
        self.Cin = cin_pad if cin_pad is not None else Cin
        self.Cin_real = Cin
        assert self.Cin >= Cin
        self.stride, self.pad, self.dil, self.compute = stride, pad, dil, compute
        self.in_dil = 1  # >1: input read as zero-stuffed (input gradient of a strided conv); set by the caller
        self.Cout_eff = round_up(Cout, 4)
        K = R * S * self.Cin
        self.K = K
        dev = weight.device
        self.korder = 1 if (compute == F16 and not tap_major and self.Cin % 32 == 0 and R * S > 1) else 0
        if compute == F16 and weight.dtype == torch.float32 and weight.is_contiguous():
            # one packing kernel instead of the torch chain below
            if self.Cin % 8:
                raise ValueError(f"f16 path needs Cin % 8 == 0 (got {self.Cin}); pass cin_pad")
            tile = max(_lib.lib().ctdet_conv_cout_tile(self.Cout_eff), cout_align or 1)
            self.Kpad = round_up(K, 32)
            self.Cout_pad = round_up(self.Cout_eff, tile)
            O, I = weight.shape[0], weight.shape[1]
            args = (O, I, weight.shape[2], weight.shape[3], self.Cin, self.Cout_pad, self.Kpad, self.korder,
                    dcn_mode if dcn_mode else int(bool(transposed)))
            plan = PACK_PLAN if (PACK_PLAN is not None and PACK_PLAN.covers(weight)) else None
            wp = plan.lookup(args + (weight.data_ptr(),), weight) if plan is not None else None
            if wp is None:
                # a stale planned entry is re-packed into its own buffer: a captured step reads that address
                wp = plan.stale_buffer(args + (weight.data_ptr(),)) if plan is not None else None
                if wp is None:
                    wp = torch.empty(self.Cout_pad, self.Kpad, dtype=torch.float16, device=dev)
                rc = _lib.lib().ctdet_pack_weights(_ptr(weight.detach()), _ptr(wp), *args, _stream())
                _lib.check(rc, "ctdet_pack_weights")
                if plan is not None:
                    plan.record(args + (weight.data_ptr(),), weight, wp, args)
            self.w = wp
            self.scale = self._pad_vec(scale, 1.0, dev)
            self.bias = self._pad_vec(bias, 0.0, dev)
            return
        if compute == F16X3 and weight.dtype == torch.float32 and weight.is_contiguous():
            # the split operands come from ctdet_pack_weights_x3, one launch per layout, built when a kernel first asks for
            # one (`w` / `scale`: the tap-major split image; `w_pair` / `scale_pair`: the tap-pair image of the 3x3 halo kernels)
            tile = max(_lib.lib().ctdet_conv_cout_tile(self.Cout_eff), cout_align or 1)
            self.Kpad = round_up(K, 16)
            self.Cout_pad = round_up(self.Cout_eff, tile)
            self._x3_src = (weight.detach(), dcn_mode if dcn_mode else int(bool(transposed)))
            self._x3 = {}
            self._user_scale = self._pad_vec(scale, 1.0, dev)
            self._pair_capable = (R, S, stride, pad, dil) == (3, 3, 1, 1, 1) and self.Cin % 16 == 0 and not dcn_mode
            self.bias = self._pad_vec(bias, 0.0, dev)
            return
        if transposed:
            weight = flip_taps(weight.detach()).permute(1, 0, 2, 3).contiguous()
        w = weight.detach().to(torch.float32).permute(0, 2, 3, 1)  # [Cout,R,S,Cin]
        if self.Cin != Cin:
            w = kpad(w, (0, self.Cin - Cin))
        # k ordering (ctdet_conv_desc.korder): chunk-major keeps the R*S taps of one 32-channel chunk adjacent
        if self.korder == 1:
            w = w.reshape(Cout, R * S, self.Cin // 32, 32).permute(0, 2, 1, 3)
        w = w.reshape(Cout, K)
        if compute == F16:
            if self.Cin % 8:
                raise ValueError(f"f16 path needs Cin % 8 == 0 (got {self.Cin}); pass cin_pad")
            tile = max(_lib.lib().ctdet_conv_cout_tile(self.Cout_eff), cout_align or 1)
            self.Kpad = round_up(K, 32)
            self.Cout_pad = round_up(self.Cout_eff, tile)
            wp = kpad(w.to(torch.float16), (0, self.Kpad - K, 0, self.Cout_pad - Cout))    # kernels only: see kpad
        else:
            # f32 MFMA path: the same [row = cout][k] image as the f16 operand, 16 k per LDS row
            tile = max(_lib.lib().ctdet_conv_cout_tile(self.Cout_eff), cout_align or 1)
            self.Kpad = round_up(K, 16)
            self.Cout_pad = round_up(self.Cout_eff, tile)
            wp = kpad(w.to(torch.float32), (0, self.Kpad - K, 0, self.Cout_pad - Cout))
            if wp.data_ptr() == weight.data_ptr():    # nothing to pad or reorder (1x1): the image is still a snapshot of the weight,
                wp = torch.mul(wp, 1.0)               # made by a kernel (clone() of a contiguous tensor is a hipMemcpyAsync)
            if compute == F16X3:   # same image, every group of 4 k as {w_hi[4], w_lo[4]} f16
                # rows are first scaled by a power of two (exact) so that their largest weight lies in [1024, 2048): the lo
                # halves of a row's significant weights then stay f16 normals (2^-22 of the row maximum instead of the 3e-8
                # absolute floor of the f16 subnormals, which is 1e-6 of a typical 0.02 weight); the epilogue scale undoes it
                amax = wp.abs().amax(dim=1)
                e = torch.floor(torch.log2(amax.clamp_min(1e-30)))
                pw = torch.where(amax > 0, torch.exp2(10.0 - e), torch.ones_like(amax))
                wp = wp * pw[:, None]
                inv = (1.0 / pw)[:self.Cout_eff]
                scale = inv if scale is None else self._pad_vec(scale, 1.0, dev) * inv
                if (R, S, stride, pad, dil) == (3, 3, 1, 1, 1) and self.Cin % 16 == 0 and not transposed:
                    self._wp_scaled = wp          # kept until the first plain-conv use builds the pair image from it
                ws = torch.empty_like(wp)
                _lib.check(_lib.lib().ctdet_split_weights(_ptr(wp), _ptr(ws), wp.numel(), _stream()), "ctdet_split_weights")
                wp = ws
        self.w = wp.contiguous()

        self.scale = self._pad_vec(scale, 1.0, dev)
        self.bias = self._pad_vec(bias, 0.0, dev)

    pair_korder = 2
    w_pair = None      # F16X3, 3x3 / s1 / p1: the tap-pair image of the halo-resident kernels (ctdet_conv_desc.korder 2 / 3),
    scale_pair = None  # its epilogue scale (the kernel-packed path; the torch path shares `scale`)
    _wp_scaled = None  # built on the first conv2d() that can use it (a DCNv2 weight never does)
    _x3_src = None     # (f32 OIHW parameter, transposed mode) when the f16x3 operands come from ctdet_pack_weights_x3
    _pair_capable = False
    _w = _scale = None

    @property
    def w(self):
        return self._w if self._x3_src is None else self._x3_operand(0)[0]

    @w.setter
    def w(self, v):
        self._w = v

    @property
    def scale(self):
        return self._scale if self._x3_src is None else self._x3_operand(0)[1]

    @scale.setter
    def scale(self, v):
        self._scale = v

    def _x3_operand(self, layout):
        """(packed image viewed as f32 [rows_pad, Kpad], epilogue scale) of one layout of ctdet_pack_weights_x3; planned
        (persistent buffers refreshed in one launch after the optimizer step) when the weight lives in the optimizer's buffer"""
        e = self._x3.get(layout)
        if e is not None:
            return e
        weight, tmode = self._x3_src
        nch = self.Cin // 16
        if layout == 0:
            rows_pad, Kpad = self.Cout_pad, self.Kpad
        else:
            rows_pad, Kpad = round_up(self.Cout_pad, 32), (nch // 2 * 288 if layout == 3 else nch * 160)
        O, I = weight.shape[0], weight.shape[1]
        R, S = (1, 1) if tmode >= 2 else (weight.shape[2], weight.shape[3])
        bufs = pack_x3(weight, (O, I, R, S, self.Cin, rows_pad, Kpad, layout, tmode, self.Cout_eff))
        sc = bufs[1] if self._user_scale is None else bufs[1] * self._user_scale
        e = self._x3[layout] = (bufs[0], sc)
        return e

    def _pack_pairs(self, wp):
        """wp: the scaled tap-major f32 image [Cout_pad, 9*Cin] -> pair image viewed as f32, rows padded to a multiple of 32 (the
        narrowest tile of the kernel).  A 128-byte step {X, Y} multiplies two (tap, 16-channel chunk) operands a, b:
        X = for q in 0..3 {w_hi[a][4q..4q+3], w_hi[b][4q..4q+3]}, Y likewise from w_lo.
        Cin % 32 == 0 (korder 3, [rows, Cin/32*288]): per chunk PAIR (A, B) nine steps -- taps (2s, 2s+1) of A, s = 0..3; tap 8
        of A with tap 8 of B; taps (2s, 2s+1) of B.  Otherwise (korder 2, [rows, Cin/16*160]): per chunk five steps, taps
        (2s, 2s+1), the tenth tap zero.  Returns (image, korder)."""
        rows = round_up(self.Cout_pad, 32)
        nch = self.Cin // 16
        w = torch.zeros(rows, 10, self.Cin, dtype=torch.float32, device=wp.device)
        w[:wp.shape[0], :9] = wp.reshape(wp.shape[0], 9, self.Cin)
        hi = w.to(torch.float16)
        lo = (w - hi.float()).to(torch.float16)
        if nch % 2 == 0:
            hl = torch.stack([hi, lo], 0).reshape(2, rows, 10, nch // 2, 2, 4, 4)   # [X/Y, row, tap, chunk pair, A/B, q, j]
            steps = ([((2 * s, 0), (2 * s + 1, 0)) for s in range(4)] + [((8, 0), (8, 1))]
                     + [((2 * s, 1), (2 * s + 1, 1)) for s in range(4)])
            tap = torch.tensor([[a[0], b[0]] for a, b in steps], device=wp.device)    # [9, 2]
            ab = torch.tensor([[a[1], b[1]] for a, b in steps], device=wp.device)
            g = hl[:, :, tap, :, ab]                # [9, 2, X/Y, row, chunk pair, q, j] (advanced indices first)
            img = g.permute(3, 4, 0, 2, 5, 1, 6).contiguous()                       # [row, chunk pair, step, X/Y, q, operand, j]
            return img.reshape(rows, nch // 2 * 576).view(torch.float32), 3
        hl = torch.stack([hi, lo], 0).reshape(2, rows, 5, 2, nch, 4, 4)     # [X/Y, row, pair, tap of pair, chunk, q, j]
        img = hl.permute(1, 4, 2, 0, 5, 3, 6).contiguous()                  # [row, chunk, pair, X/Y, q, tap of pair, j]
        return img.reshape(rows, nch * 320).view(torch.float32), 2

    def pair_ok(self, x):
        """may the halo pair kernel take this input?"""
        B, H, W, _ = x.shape
        out = torch.empty(0, *self.out_hw(H, W), self.Cout_eff, dtype=torch.float32, device=x.device)
        d = self.desc(x[:0], out, ACT_NONE, None)
        d.B = B
        return self._pair_image(d, x)

    def _pair_image(self, d, x):
        """does the conv d of x run on a pair-packed image?  Which convs do is the library's rule (ctdet_conv_pair_supported:
        tiles, alignment, the layers left to the LDS-window kernel, tuning flags); here only whether such an image exists or can
        be made, and its packing on first use."""
        if self.w_pair is None and self._wp_scaled is None and not self._pair_capable:
            return False
        korder = _lib.lib().ctdet_conv_pair_supported(C.byref(d), _ptr(x))
        if korder and self.w_pair is None:
            self.pair_korder = korder
            if self._x3_src is not None:
                self.w_pair, self.scale_pair = self._x3_operand(korder)
            else:
                (self.w_pair, packed), self._wp_scaled = self._pack_pairs(self._wp_scaled), None
                assert packed == korder, (packed, korder)
        return bool(korder)

    def _pad_vec(self, v, fill, dev):
        if v is None:
            return None
        v = v.detach().to(torch.float32)
        if v.shape[0] == self.Cout_eff:
            return v.contiguous()
        return kpad(v.contiguous(), (0, self.Cout_eff - v.shape[0]), value=float(fill))   # not a slice assignment: see kpad

    @property
    def act_dt(self):
        """dtype enum of the activations this contraction takes"""
        return F16 if self.compute == F16 else F32

    def out_hw(self, H, W):
        Ho = (H + 2 * self.pad - (self.dil * (self.R - 1) + 1)) // self.stride + 1
        Wo = (W + 2 * self.pad - (self.dil * (self.S - 1) + 1)) // self.stride + 1
        return Ho, Wo

    def desc(self, x, out, act, residual, clamp=(0.0, 1.0), allow_pair=False):
        B, H, W, Cx = x.shape
        assert Cx == self.Cin, f"conv expects {self.Cin} input channels, got {Cx}"
        if self.in_dil > 1:
            Ho, Wo = out.shape[1], out.shape[2]
        else:
            Ho, Wo = self.out_hw(H, W)
        assert tuple(out.shape[:3]) == (B, Ho, Wo) and out.shape[3] >= self.Cout_eff, (out.shape, (B, Ho, Wo, self.Cout_eff))
        d = ConvDesc()
        d.B, d.H, d.W, d.Cin, d.in_stride = B, H, W, self.Cin, _nhwc_stride(x)
        d.Cout, d.Ho, d.Wo, d.out_stride = self.Cout_eff, Ho, Wo, _nhwc_stride(out)
        d.R, d.S, d.stride, d.pad, d.dil = self.R, self.S, self.stride, self.pad, self.dil
        d.Kpad, d.Cout_pad = self.Kpad, self.Cout_pad
        d.compute_dtype, d.out_dtype, d.act = self.compute, dt_of(out), act
        d.res_stride = _nhwc_stride(residual) if residual is not None else 0
        d.clamp_lo, d.clamp_hi = clamp
        d.korder = self.korder
        d.in_dil = self.in_dil
        if allow_pair and self._pair_image(d, x):
            d.korder, d.Kpad, d.Cout_pad = self.pair_korder, self.w_pair.shape[1], self.w_pair.shape[0]
        return d


def _alloc_out(x, p, out, out_dtype):
    B, H, W, _ = x.shape
    Ho, Wo = p.out_hw(H, W)
    assert out is not None or p.in_dil == 1, "input-dilated convs need an explicit output buffer"
    if out is None:
        dt = out_dtype if out_dtype is not None else (torch.float16 if p.compute == F16 else torch.float32)
        out = torch.empty(B, Ho, Wo, p.Cout_eff, dtype=dt, device=x.device)
    return out


def conv2d(x, p, out=None, act=ACT_NONE, residual=None, out_dtype=None, clamp=(0.0, 1.0)):
    """y = act(conv(x) * scale + bias + residual); x NHWC. Returns the NHWC output buffer."""
    _require_cuda(x, residual, out)
    assert dt_of(x) == p.act_dt, "input dtype must match the packed compute dtype"
    out = _alloc_out(x, p, out, out_dtype)
    if residual is not None:
        assert residual.dtype == out.dtype and residual.shape[:3] == out.shape[:3]
    d = p.desc(x, out, act, residual, clamp, allow_pair=True)
    prof = _Prof(p, d.B * d.Ho * d.Wo, False, d.out_dtype)
    if d.korder >= 2:
        w, sc = p.w_pair, (p.scale_pair if p.scale_pair is not None else p.scale)
    else:
        w, sc = p.w, p.scale
    for _ in range(prof.reps()):
        rc = _lib.lib().ctdet_conv2d_fwd(C.byref(d), _ptr(x), _ptr(w), _ptr(sc), _ptr(p.bias), _ptr(residual),
                                         _ptr(out), _stream())
    _lib.check(rc, "ctdet_conv2d_fwd")
    prof.done()
    _range_check(out, p, "conv2d")
    return out


def conv1x1_cat(xs, p, out=None, act=ACT_NONE, residual=None, out_dtype=None):
    """1x1 conv over the channel-concatenation of the NHWC tensors `xs` (<= 4) without building the concat."""
    _require_cuda(*xs)
    assert 1 <= len(xs) <= 4 and p.R == 1 and p.S == 1 and p.stride == 1 and p.pad == 0
    B, H, W, _ = xs[0].shape
    for t in xs:
        assert tuple(t.shape[:3]) == (B, H, W) and dt_of(t) == p.act_dt
    cins = [t.shape[3] for t in xs]
    assert sum(cins) == p.Cin, (cins, p.Cin)
    if out is None:
        dt = out_dtype if out_dtype is not None else (torch.float16 if p.compute == F16 else torch.float32)
        out = torch.empty(B, H, W, p.Cout_eff, dtype=dt, device=xs[0].device)
    d = ConvDesc()
    d.B, d.H, d.W, d.Cin, d.in_stride = B, H, W, p.Cin, p.Cin
    d.Cout, d.Ho, d.Wo, d.out_stride = p.Cout_eff, H, W, _nhwc_stride(out)
    d.R = d.S = d.stride = d.dil = 1
    d.pad = 0
    d.Kpad, d.Cout_pad = p.Kpad, p.Cout_pad
    d.compute_dtype, d.out_dtype, d.act = p.compute, dt_of(out), act
    d.res_stride = _nhwc_stride(residual) if residual is not None else 0
    d.clamp_lo, d.clamp_hi = 0.0, 1.0
    d.korder = 0
    d.in_dil = 1
    n = len(xs)
    ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in xs])
    cin_a = (C.c_int32 * n)(*cins)
    str_a = (C.c_int32 * n)(*[_nhwc_stride(t) for t in xs])
    prof = _Prof(p, B * H * W, False, d.out_dtype, len(xs))
    for _ in range(prof.reps()):
        rc = _lib.lib().ctdet_conv1x1_cat_fwd(C.byref(d), ptrs, cin_a, str_a, n, _ptr(p.w), _ptr(p.scale),
                                              _ptr(p.bias), _ptr(residual), _ptr(out), _stream())
    _lib.check(rc, "ctdet_conv1x1_cat_fwd")
    prof.done()
    _range_check(out, p, "conv1x1_cat")
    return out


HEADS_FUSED = os.environ.get("CTDET_NO_FUSED_HEADS", "0") != "1"


def dcnv2(x, offset_mask, p, out=None, act=ACT_NONE, out_dtype=None, mask_is_prob=False, want_cols=False):
    """Deformable conv: offset_mask is the raw f32 NHWC output of conv_offset_mask (>= 27 ch);
    mask_is_prob is the mask mode: False / DCN_MASK_LOGIT = mask logits (sigmoid in the kernel), True / DCN_MASK_PROB = the 9
    mask channels already went through sigmoid, DCN_MASK_NONE = DCNv1, offset_mask holds the 18 offsets only (>= 18 ch; no
    channel beyond them is read, the kernels' mask-free variants run).
    want_cols (f16x3, training): returns (y, cols) where cols f32 [B,H,W,9*Cin] are the sampled columns written by the same
    kernel, or (y, None) when the layer is not served by the LDS-window kernel."""
    _require_cuda(x, offset_mask, out)
    assert dt_of(x) == p.act_dt and offset_mask.dtype == torch.float32
    mask_is_prob = int(mask_is_prob)
    if mask_is_prob not in (DCN_MASK_LOGIT, DCN_MASK_PROB, DCN_MASK_NONE):
        raise ValueError(f"dcnv2: mask mode {mask_is_prob}")
    if p.compute == F16 and p.Cout_pad % 64:
        raise ValueError(f"dcnv2 (f16) works on 64-cout tiles: pack the weights with PackedConv(..., cout_align=64) "
                         f"(Cout={p.Cout}, packed rows {p.Cout_pad})")
    if out is None and p.compute == F16 and p.Cout_eff % 8:
        # the window kernel stores 16 bytes at a time: give the buffer a pixel stride that is a multiple of 8 channels and
        # hand back the view of the real ones
        B, H, W, _ = x.shape
        dt = out_dtype if out_dtype is not None else torch.float16
        out = torch.empty(B, H, W, round_up(p.Cout_eff, 8), dtype=dt, device=x.device)[..., :p.Cout_eff]
    out = _alloc_out(x, p, out, out_dtype)
    assert tuple(offset_mask.shape[:3]) == tuple(out.shape[:3])
    p._wp_scaled = None          # a deformable conv's weights: no pair image will be needed
    d = p.desc(x, out, act, None)
    cols = None
    if want_cols and p.compute == F16X3 and _lib.lib().ctdet_dcnv2_cols_supported(C.byref(d), _ptr(x), _ptr(out)):
        cols = torch.empty(x.shape[0], x.shape[1], x.shape[2], 9 * p.Cin, dtype=torch.float32, device=x.device)
    prof = _Prof(p, d.B * d.Ho * d.Wo, True, d.out_dtype)     # (after the allocation: a 600 MB hipMalloc is not kernel time)
    if prof.on and cols is not None:
        prof.bytes += cols.numel() * 4
    for _ in range(prof.reps()):
        if cols is not None:
            rc = _lib.lib().ctdet_dcnv2_fwd_cols(C.byref(d), _ptr(x), _ptr(offset_mask), _nhwc_stride(offset_mask), int(mask_is_prob),
                                                 _ptr(p.w), _ptr(p.scale), _ptr(p.bias), _ptr(out), _ptr(cols), _stream())
        else:
            rc = _lib.lib().ctdet_dcnv2_fwd(C.byref(d), _ptr(x), _ptr(offset_mask), _nhwc_stride(offset_mask),
                                            int(mask_is_prob), _ptr(p.w), _ptr(p.scale), _ptr(p.bias), _ptr(out), _stream())
    _lib.check(rc, "ctdet_dcnv2_fwd")
    prof.done()
    _range_check(out, p, "dcnv2")
    return (out, cols) if want_cols else out


# CTDET_NO_FUSED_DCN_X3=1: the f16x3 DCNv2 layers keep their offset / mask conv as a launch of its own (the A/B switch of the
# fused form; CTDET_RANGE_CHECK=1 does the same, it has to see that conv's output)
DCN_X3_FUSED = os.environ.get("CTDET_NO_FUSED_DCN_X3", "0") != "1"


def _off_operands_x3(p_off):
    """(korder-3 pair image, [32 biases, 32 inverse row scales]) of a packed f16x3 offset / mask conv for ctdet_dcnv2_offset_fwd,
    or None when it has no such image: the same image, bias and scale conv2d() hands the pair kernel"""
    if p_off.w_pair is None or p_off.pair_korder != 3:
        if p_off._x3_src is not None and p_off._pair_capable and p_off.Cin % 32 == 0:
            p_off.pair_korder = 3
            p_off.w_pair, p_off.scale_pair = p_off._x3_operand(3)
        elif p_off._wp_scaled is not None and p_off.w_pair is None and p_off.Cin % 32 == 0:
            (p_off.w_pair, p_off.pair_korder), p_off._wp_scaled = p_off._pack_pairs(p_off._wp_scaled), None
        else:
            return None
    sc = p_off.scale_pair if p_off.scale_pair is not None else p_off.scale
    hit = p_off.__dict__.get("_off_bs")
    if hit is None or hit[0] is not sc or hit[1] is not p_off.bias:
        bs = torch.zeros(64, dtype=torch.float32, device=p_off.w_pair.device)
        bs[:p_off.bias.shape[0]] = p_off.bias
        bs[32:32 + sc.shape[0]] = sc
        hit = p_off._off_bs = (sc, p_off.bias, bs)
    return p_off.w_pair, hit[2]


def dcnv2_offset_supported(x, p_off, p):
    """may `dcnv2_offset` serve this layer?  Both convs 3x3/s1/p1 on a map divisible by the 8x16 tile, Cin % 32 == 0, at most 64
    couts packed to 64 rows, 27 offset / mask channels in 32 packed rows -- f16: chunk-major; f16x3: the korder-3 pair image
    (f32 x of 16-byte aligned pixels).  The batch size plays no part."""
    if p.compute not in (F16, F16X3) or p_off.compute != p.compute or p.Cout_pad != 64 or p_off.Cout != 27:
        return False
    if (p_off.R, p_off.S, p_off.stride, p_off.pad, p_off.dil) != (3, 3, 1, 1, 1) or p_off.bias is None:
        return False
    B, H, W, _ = x.shape
    if p.compute == F16X3:
        if dt_of(x) != F32 or x.data_ptr() % 16 or p.Cin % 32 or p_off.Cin != p.Cin or _off_operands_x3(p_off) is None:
            return False
        out = torch.empty(0, H, W, p.Cout_eff, dtype=torch.float32, device=x.device)
    else:
        if p_off.Cout_pad != 32 or (p_off.korder, p_off.Kpad) != (1, p.Kpad):
            return False
        out = torch.empty(0, H, W, round_up(p.Cout_eff, 8), dtype=torch.float16, device=x.device)
    d = p.desc(x[:0], out, ACT_NONE, None)
    d.B = B
    return bool(_lib.lib().ctdet_dcnv2_offset_supported(C.byref(d)))


def dcnv2_offset(x, p_off, p, out=None, act=ACT_NONE, out_dtype=None, om_out=None, finite_flag=None):
    """act(dcn(x, conv_offset_mask(x))) in one kernel (ctdet_dcnv2_offset_fwd): p_off = the packed 3x3 offset / mask conv with
    its bias, p = the packed deformable conv.  om_out (f16 mode only; f32 [B,H,W,>=28]) receives the offsets / mask logits if given.
    finite_flag (f16x3 only): an int32 [1] device tensor holding 1; the kernel's epilogue stores 0 into it when a value it writes
    is inf or NaN -- what `finite_flag(out, flag=finite_flag)` would find, without the pass over `out`."""
    _require_cuda(x, out, om_out, finite_flag)
    assert dt_of(x) == p.act_dt and p.compute in (F16, F16X3) and p_off.compute == p.compute and p_off.bias is not None
    assert finite_flag is None or (p.compute == F16X3 and finite_flag.dtype == torch.int32 and finite_flag.numel() == 1)
    if p.compute == F16X3:
        assert om_out is None, "dcnv2_offset (f16x3) keeps no offsets: the inference form"
        ops_off = _off_operands_x3(p_off)
        if ops_off is None:
            raise ValueError("dcnv2_offset (f16x3): the offset conv has no korder-3 pair image (3x3/s1/p1, Cin % 32 == 0)")
        w_off, b_off = ops_off
        p._wp_scaled = None          # a deformable conv's weights: no pair image will be needed
    else:
        assert p_off.scale is None
        w_off, b_off = p_off.w, p_off.bias
    if out is None and p.compute == F16 and p.Cout_eff % 8:
        B, H, W, _ = x.shape
        dt = out_dtype if out_dtype is not None else torch.float16
        out = torch.empty(B, H, W, round_up(p.Cout_eff, 8), dtype=dt, device=x.device)[..., :p.Cout_eff]
    out = _alloc_out(x, p, out, out_dtype)
    assert p_off.bias.shape[0] >= 28                     # Cout_eff floats: the kernel reads channels 0..27
    d = p.desc(x, out, act, None)
    prof = _Prof(p, d.B * d.Ho * d.Wo, True, d.out_dtype, flops=2.0 * d.B * d.Ho * d.Wo * p.K * (p.Cout + 27))
    if prof.on:
        prof.bytes -= d.B * d.Ho * d.Wo * 27 * 4      # no offset tensor is read
    for _ in range(prof.reps()):
        rc = _lib.lib().ctdet_dcnv2_offset_finite_fwd(C.byref(d), _ptr(x), _ptr(w_off), _ptr(b_off), _ptr(om_out),
                                                      _nhwc_stride(om_out) if om_out is not None else 0, _ptr(p.w), _ptr(p.scale),
                                                      _ptr(p.bias), _ptr(out), _ptr(finite_flag), _stream())
    _lib.check(rc, "ctdet_dcnv2_offset_finite_fwd")
    prof.done()
    if p.compute == F16X3:
        _range_check(out, p, "dcnv2_offset")
    return out


def _mirror_from(mirror, B):
    """(output images, mirror_from) of the flip-test forms: False = plain, True = every image mirrored, "both" = 2B output
    images, the plain B first, then their mirrors"""
    assert mirror in (False, True, "both"), mirror
    return (2 * B, B) if mirror == "both" else (B, 0 if mirror else None)


def preprocess(images, mean, std, Hp, Wp, out_dtype=torch.float16, out=None, partial=False, border=0, mirror=False):
    """images: [B,3,H,W] uint8/float32 CHW on device -> normalised NHWC [B,Hp,Wp,8] (3 channels used).
    `out` may be a batch-slice of a larger padded buffer (ragged batches: one call per image).
    border > 0: `out` is a caller-owned [B,Hp+2b,Wp+2b,8] buffer whose zero frame was cleared once.
    mirror (flip test): True = the horizontal mirror of the NETWORK INPUT -- the normalised tensor after right/bottom zero
    padding: column x holds source column Wp-1-x, zero where that is >= W, so the padding sits on the left; "both" = 2B
    output images, the plain ones then their mirrors, from the same B images."""
    _require_cuda(images)
    B, Cc, H, W = images.shape
    assert Cc == 3 and images.stride(3) == 1 and images.stride(2) == W and images.stride(1) == H * W
    B, mfrom = _mirror_from(mirror, B)
    if out is None:
        if border:
            out = torch.zeros(B, Hp + 2 * border, Wp + 2 * border, 8, dtype=out_dtype, device=images.device)
        else:
            out = torch.empty(B, Hp, Wp, 8, dtype=out_dtype, device=images.device)
    assert out.shape[3] % 8 == 0 or (out.shape[3] == 4 and out.dtype == torch.float32)
    assert tuple(out.shape[1:3]) == (Hp + 2 * border, Wp + 2 * border)
    m = (C.c_float * 3)(*[float(v) for v in mean])
    s = (C.c_float * 3)(*[float(v) for v in std])
    assert out.shape[0] == B
    if mfrom is None:
        rc = _lib.lib().ctdet_preprocess(_ptr(images), dt_of(images), _ptr(out), dt_of(out), B, H, W, Hp, Wp,
                                         images.stride(0), m, s, _nhwc_stride(out), int(border), _stream())
    else:
        rc = _lib.lib().ctdet_preprocess_mirror(_ptr(images), dt_of(images), _ptr(out), dt_of(out), B, H, W, Hp, Wp,
                                                images.stride(0), m, s, _nhwc_stride(out), int(border), mfrom, _stream())
    _lib.check(rc, "ctdet_preprocess")
    return out


# ---------------------------------------------------------------------------------- uint8 bilinear resize (csrc/resize.hip)
RESIZE_TW, RESIZE_RB = 64, 8      # output columns / rows of one block (csrc/resize.hip)
# ctdet_resize_desc as a numpy record: the descriptors of a batch are one array, uploaded as it is
RESIZE_DESC_DTYPE = np.dtype([("src", "<u8"), ("dst", "<u8")]
                             + [(n, "<i8") for n in ("src_row", "src_pix", "src_chan", "dst_row", "dst_pix", "dst_chan")]
                             + [(n, "<i4") for n in ("H", "W", "new_h", "new_w", "hb", "hc", "vb", "vc", "kh", "kv", "blk0", "pad_")])
assert RESIZE_DESC_DTYPE.itemsize == C.sizeof(_lib.ResizeDesc)


class _ResizeArena:
    """pinned host buffer a resize call assembles its one upload in (descriptors, tables, host images); re-used by the next
    call once the copy out of it has finished"""

    def __init__(self):
        self.host, self.event = None, None

    def take(self, nbytes):
        if self.event is not None:
            self.event.synchronize()      # waits for the previous upload only, not for the kernels behind it
        if self.host is None or self.host.numel() < nbytes:
            self.host = torch.empty(max(round_up(nbytes, 1 << 20), 1 << 20), dtype=torch.uint8, pin_memory=True)
        return self.host

    def uploaded(self):
        if self.event is None:
            self.event = torch.cuda.Event()
        self.event.record()


_RESIZE_ARENA = _ResizeArena()


def _u8_view(img):
    """an image given as a logical [3, H, W] uint8 view -> (device pointer or None, host block or None, offset of element
    [0,0,0] in that block, H, W, (row, pixel, channel) byte strides).  Host images (numpy arrays -- strides of either sign --
    or CPU tensors) come back with the dense block of memory they live in, in its own order: an HWC image stays HWC."""
    if isinstance(img, torch.Tensor):
        assert img.dtype == torch.uint8 and img.dim() == 3 and img.shape[0] == 3, (img.dtype, tuple(img.shape))
        if img.is_cuda:
            st = img.stride()
            return img.data_ptr(), None, 0, img.shape[1], img.shape[2], (st[1], st[2], st[0])
        img = img.numpy()
    assert isinstance(img, np.ndarray) and img.dtype == np.uint8 and img.ndim == 3 and img.shape[0] == 3, (
        "resize_u8 takes logical [3, H, W] uint8 views (an HWC array a: a.transpose(2, 0, 1))")
    lo = sum((n - 1) * st for n, st in zip(img.shape, img.strides) if st < 0)
    hi = sum((n - 1) * st for n, st in zip(img.shape, img.strides) if st > 0)
    if hi - lo + 1 != img.size:      # a crop or a strided view: its own dense copy
        img = np.ascontiguousarray(img)
        lo = 0
    block = np.frombuffer((C.c_uint8 * img.size).from_address(img.ctypes.data + lo), dtype=np.uint8)
    st = img.strides
    return None, (block, img), -lo, img.shape[1], img.shape[2], (st[1], st[2], st[0])


class ResizeLaunch:
    """one prepared resize of a list of images (resize_u8_prepare): the uploaded descriptors, tables and host images, and the
    destinations.  launch() may be repeated: it reads the same sources and writes the same destinations again."""

    def __init__(self, dev, desc, tab_at, blocks, outs):
        self.dev, self.desc, self.tab_at, self.blocks, self.outs = dev, desc, tab_at, blocks, outs

    def launch(self):
        n, tab = len(self.desc), C.c_void_p(self.dev.data_ptr() + self.tab_at)
        with torch.cuda.device(self.dev.device):
            if n == 1:      # the one-image entry point: the descriptor travels as a kernel argument
                one = _lib.ResizeDesc.from_buffer_copy(self.desc[0].tobytes())
                rc = _lib.lib().ctdet_resize_bilinear_u8(C.byref(one), tab, _stream())
            else:
                rc = _lib.lib().ctdet_resize_bilinear_u8_batch(C.c_void_p(self.dev.data_ptr()), n, self.blocks, tab, _stream())
        _lib.check(rc, "ctdet_resize_bilinear_u8")
        return self.outs


def resize_u8(images, sizes, outs=None, device=None):
    """Pillow's 8-bit bilinear resize (what data.transforms.ResizeTransform.apply_image computes on the host) of a list of
    3-channel images on the device, bit for bit, in ONE launch whatever their sizes.

    images: logical [3, H, W] uint8 views with any strides -- a device or CPU tensor, or a numpy array; an HWC image is
      `a.transpose(2, 0, 1)` / `t.permute(2, 0, 1)`, a reversed channel order `a[::-1]` of a numpy view (stride -1).  Host images
      travel to the device inside this call's single upload, in their own memory order.
    sizes: (new_h, new_w) per image.  outs: device uint8 views [3, new_h, new_w] with any strides (a window of a staging
      batch); None: fresh CHW tensors.  Returns outs.
    One host-to-device copy per call carries the descriptors, the coefficient tables (data.resample.bilinear_tables, cached
    per (in, out) pair and shared by the images of the call) and the host images."""
    if len(images) == 0:
        return []
    return resize_u8_prepare(images, sizes, outs, device).launch()


def resize_u8_prepare(images, sizes, outs=None, device=None):
    """everything of resize_u8 but the launch: a ResizeLaunch"""
    from .data import resample
    n = len(images)
    assert n >= 1 and n == len(sizes) and (outs is None or len(outs) == n)
    views = [_u8_view(im) for im in images]
    if device is None:
        device = outs[0].device if outs is not None else next((im.device for im in images if isinstance(im, torch.Tensor) and im.is_cuda),
                                                                torch.device("cuda", torch.cuda.current_device()))
    if outs is None:
        outs = [torch.empty(3, int(nh), int(nw), dtype=torch.uint8, device=device) for nh, nw in sizes]
    desc = np.zeros(n, dtype=RESIZE_DESC_DTYPE)
    tables, placed, words = [], {}, 0

    def place(in_size, out_size):
        """(bounds offset, coeffs offset, entries per coefficient row) of the axis' tables in this call's buffer"""
        nonlocal words
        hit = placed.get((in_size, out_size))
        if hit is None:
            bounds, coeffs = resample.bilinear_tables(in_size, out_size)
            hit = placed[(in_size, out_size)] = (words, words + bounds.size, coeffs.shape[1])
            tables.extend((bounds.reshape(-1), coeffs.reshape(-1)))
            words += bounds.size + coeffs.size
        return hit

    blocks = 0
    for i, ((ptr, host, org, H, W, st), (nh, nw), out) in enumerate(zip(views, sizes, outs)):
        nh, nw = int(nh), int(nw)
        assert nh >= 1 and nw >= 1 and H >= 1 and W >= 1, (H, W, nh, nw)
        assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (3, nh, nw), (
            f"image {i}: the destination must be a device uint8 view [3, {nh}, {nw}], got {tuple(out.shape)} {out.dtype} on {out.device}")
        d = desc[i]
        d["dst"] = out.data_ptr()
        d["dst_row"], d["dst_pix"], d["dst_chan"] = out.stride(1), out.stride(2), out.stride(0)
        d["src_row"], d["src_pix"], d["src_chan"] = st
        d["H"], d["W"], d["new_h"], d["new_w"] = H, W, nh, nw
        if W != nw:
            d["hb"], d["hc"], d["kh"] = place(W, nw)
        if H != nh:
            d["vb"], d["vc"], d["kv"] = place(H, nh)
        d["blk0"] = blocks
        blocks += -(-nw // RESIZE_TW) * -(-nh // RESIZE_RB)
    assert blocks < 2 ** 31 and words < 2 ** 31
    dev, tab_at = _u8_upload(desc, tables, words, views, device)
    return ResizeLaunch(dev, desc, tab_at, blocks, outs)


def _u8_upload(desc, tables, words, views, device, first=None):
    """the one upload of a resize / warp call: [descriptors][int32 tables][host images], each part 16-byte aligned, through
    the pinned arena.  Fills desc["src"] (device images: their pointer; host images: where they land), plus first[i] bytes
    where given (a source read from another element than [0, 0, 0]).  Returns the device buffer and the byte offset of the
    tables in it."""
    tab_at = round_up(desc.nbytes, 16)
    total = round_up(tab_at + 4 * max(words, 1), 16)
    host_at = []
    for ptr, host, org, H, W, st in views:
        host_at.append(total)
        if host is not None:
            total = round_up(total + host[0].size, 16)
    arena = _RESIZE_ARENA.take(total)
    dev = torch.empty(total, dtype=torch.uint8, device=device)
    staged = arena.numpy()
    for i, (ptr, host, org, H, W, st) in enumerate(views):
        if host is not None:
            staged[host_at[i]:host_at[i] + host[0].size] = host[0]
            ptr = dev.data_ptr() + host_at[i] + org
        desc["src"][i] = ptr + (first[i] if first is not None else 0)
    if tables:
        staged[tab_at:tab_at + 4 * words] = np.concatenate(tables).view(np.uint8)
    staged[:desc.nbytes] = desc.view(np.uint8)
    with torch.cuda.device(device):
        dev.copy_(arena[:total], non_blocking=True)
        _RESIZE_ARENA.uploaded()
    return dev, tab_at


# ---------------------------------------------------------------------------------- uint8 affine warp (csrc/warp.hip)
WARP_TW, WARP_RB = 64, 8      # output columns / rows of one block (csrc/warp.hip)
# ctdet_warp_desc as a numpy record
WARP_DESC_DTYPE = np.dtype([("src", "<u8"), ("dst", "<u8")]
                           + [(n, "<i8") for n in ("src_row", "src_pix", "src_chan", "dst_row", "dst_pix", "dst_chan")]
                           + [(n, "<i4") for n in ("H", "W", "out_h", "out_w", "ax", "bx", "x0", "y0", "blk0", "pad_")])
assert WARP_DESC_DTYPE.itemsize == C.sizeof(_lib.WarpDesc)


class WarpLaunch:
    """one prepared warp of a list of images (warp_affine_u8_prepare): the uploaded descriptors, tables and host images, and
    the destinations.  launch() may be repeated: it reads the same sources and writes the same destinations again."""

    def __init__(self, dev, desc, tab_at, blocks, outs):
        self.dev, self.desc, self.tab_at, self.blocks, self.outs = dev, desc, tab_at, blocks, outs

    def launch(self):
        with torch.cuda.device(self.dev.device):
            rc = _lib.lib().ctdet_warp_affine_u8_batch(C.c_void_p(self.dev.data_ptr()), len(self.desc), self.blocks,
                                                       C.c_void_p(self.dev.data_ptr() + self.tab_at), _stream())
        _lib.check(rc, "ctdet_warp_affine_u8_batch")
        return self.outs


def warp_affine_u8(images, warps, out_hw, outs=None, device=None):
    """The 8-bit bilinear affine warp of data.warp.warp_affine_u8_reference (what data.transforms.AffineTransform.apply_image
    computes on the host) of a list of 3-channel images on the device, byte for byte, in ONE launch whatever their sizes.

    images: logical [3, H, W] uint8 views with any strides, as ops.resize_u8 takes them; host images travel inside this
      call's single upload.  Sources above data.warp.MAX_SOURCE_SIDE per side are refused.
    warps: per image a float64 [2, 4] array / tensor (data.warp.pack_warp: the inverse matrix, destination to source pixel
      index, and the flip flag) or an (M [2, 3], flip) pair.  A flipped image is read mirrored: no copy is made.
    out_hw: (out_h, out_w) of every destination.  outs: device uint8 views [3, out_h, out_w] with any strides; None: fresh
      CHW tensors.  Returns outs.
    One host-to-device copy per call carries the descriptors, the four int32 tables of every image (data.warp.warp_tables;
      a table entry outside int32 is refused) and the host images."""
    if len(images) == 0:
        return []
    return warp_affine_u8_prepare(images, warps, out_hw, outs, device).launch()


def warp_affine_u8_prepare(images, warps, out_hw, outs=None, device=None):
    """everything of warp_affine_u8 but the launch: a WarpLaunch"""
    from .data import warp as W
    n = len(images)
    assert n >= 1 and n == len(warps) and (outs is None or len(outs) == n)
    if device is None:
        device = outs[0].device if outs is not None else next((im.device for im in images if isinstance(im, torch.Tensor) and im.is_cuda), None)
    if (device is None and not torch.cuda.is_available()) or (device is not None and torch.device(device).type != "cuda"):
        raise NotImplementedError("warp_affine_u8 has no CPU implementation: the host form is data.warp.warp_affine_u8_reference")
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    out_h, out_w = int(out_hw[0]), int(out_hw[1])
    assert out_h >= 1 and out_w >= 1, out_hw
    views = [_u8_view(im) for im in images]
    if outs is None:
        outs = [torch.empty(3, out_h, out_w, dtype=torch.uint8, device=device) for _ in range(n)]
    desc = np.zeros(n, dtype=WARP_DESC_DTYPE)
    tables, first, words, blocks = [], [], 0, 0
    for i, ((ptr, host, org, H, Wd, st), warp, out) in enumerate(zip(views, warps, outs)):
        if not (H <= W.MAX_SOURCE_SIDE and Wd <= W.MAX_SOURCE_SIDE):
            raise ValueError(f"image {i}: warp_affine_u8 takes sources of at most {W.MAX_SOURCE_SIDE} pixels per side, got {H}x{Wd}")
        assert H >= 1 and Wd >= 1, (H, Wd)
        assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (3, out_h, out_w), (
            f"image {i}: the destination must be a device uint8 view [3, {out_h}, {out_w}], got {tuple(out.shape)} {out.dtype} on {out.device}")
        M, flip = W.unpack_warp(warp.cpu() if isinstance(warp, torch.Tensor) else warp)
        d = desc[i]
        d["dst"] = out.data_ptr()
        d["dst_row"], d["dst_pix"], d["dst_chan"] = out.stride(1), out.stride(2), out.stride(0)
        # a mirrored source is read from its last column backwards
        d["src_row"], d["src_pix"], d["src_chan"] = st[0], (-st[1] if flip else st[1]), st[2]
        first.append((Wd - 1) * st[1] if flip else 0)
        d["H"], d["W"], d["out_h"], d["out_w"] = H, Wd, out_h, out_w
        d["ax"], d["bx"], d["x0"], d["y0"] = words, words + out_w, words + 2 * out_w, words + 2 * out_w + out_h
        tables.extend(W.warp_tables(M, out_h, out_w))      # ax, bx, x0, y0: refuses an entry outside int32
        words += 2 * (out_w + out_h)
        d["blk0"] = blocks
        blocks += -(-out_w // WARP_TW) * -(-out_h // WARP_RB)
    assert blocks < 2 ** 31 and words < 2 ** 31
    dev, tab_at = _u8_upload(desc, tables, words, views, device, first)
    return WarpLaunch(dev, desc, tab_at, blocks, outs)


# ---------------------------------------------------------------------------------- uint8 colour jitter (csrc/jitter.hip)
JITTER_TW, JITTER_TH = 64, 4      # pixel columns / rows of one block (csrc/jitter.hip)
# ctdet_jitter_desc as a numpy record
JITTER_DESC_DTYPE = np.dtype([("img", "<u8"), ("row", "<i8"), ("pix", "<i8"), ("chan", "<i8"), ("h", "<i4"), ("w", "<i4"),
                              ("blk0", "<i4"), ("sum_slot", "<i4"), ("on", "<i4", (4,)), ("contrast", "<f8", (2,)),
                              ("brightness", "<f8", (2,)), ("saturation", "<f8", (2,)), ("lighting", "<f8", (3,))])
assert JITTER_DESC_DTYPE.itemsize == C.sizeof(_lib.JitterDesc)


class JitterLaunch:
    """one prepared colour jitter of a list of images (colour_jitter_u8_prepare): the uploaded descriptors and the sum slots.
    n = 0 (nothing drawn): launch() launches nothing."""

    def __init__(self, dev, n, blocks, sums, images):
        self.dev, self.n, self.blocks, self.sums, self.images = dev, n, blocks, sums, images

    def launch_sum(self):
        """the byte sums of the images whose contrast was drawn (none: no launch)"""
        if self.n and self.sums.numel():
            with torch.cuda.device(self.sums.device):
                rc = _lib.lib().ctdet_byte_sum_u8_batch(C.c_void_p(self.dev.data_ptr()), self.n, _ptr(self.sums), self.sums.numel(),
                                                        _stream())
            _lib.check(rc, "ctdet_byte_sum_u8_batch")

    def launch_jitter(self):
        if self.n:
            with torch.cuda.device(self.sums.device):
                rc = _lib.lib().ctdet_colour_jitter_u8_batch(C.c_void_p(self.dev.data_ptr()), self.n, self.blocks, _ptr(self.sums),
                                                             self.sums.numel(), _stream())
            _lib.check(rc, "ctdet_colour_jitter_u8_batch")

    def launch(self):
        self.launch_sum()
        self.launch_jitter()
        return self.images


def _jitter_table(images, specs, all_sums=False):
    """descriptors (numpy records) of the images that drew a transform, their block count and the number of sum slots.
    all_sums: every image gets a descriptor and a slot (byte_sum_u8)."""
    from .data.jitter import spec_array
    desc = np.zeros(len(images), dtype=JITTER_DESC_DTYPE)
    n = blocks = slots = 0
    for i, (im, spec) in enumerate(zip(images, specs)):
        assert isinstance(im, torch.Tensor) and im.is_cuda and im.dtype == torch.uint8 and im.dim() == 3 and im.shape[0] == 3, (
            f"image {i}: colour_jitter_u8 takes device uint8 views [3, h, w]")
        spec = spec_array(spec)
        if not (all_sums or spec[:, 0].any()):
            continue
        d = desc[n]
        n += 1
        h, w = int(im.shape[1]), int(im.shape[2])
        assert h >= 1 and w >= 1 and 3 * h * w < 2 ** 53, (h, w)
        d["img"], d["row"], d["pix"], d["chan"], d["h"], d["w"], d["blk0"] = im.data_ptr(), im.stride(1), im.stride(2), im.stride(0), h, w, blocks
        blocks += -(-w // JITTER_TW) * -(-h // JITTER_TH)
        d["on"] = spec[:, 0] != 0
        d["contrast"], d["brightness"], d["saturation"], d["lighting"] = spec[0, 1:3], spec[1, 1:3], spec[2, 1:3], spec[3, 1:4]
        d["sum_slot"] = -1
        if all_sums or spec[0, 0]:
            d["sum_slot"] = slots
            slots += 1
    assert blocks < 2 ** 31
    return desc[:n], blocks, slots


def _jitter_upload(desc, device):
    """the descriptors on the device, through the pinned arena of the resize upload"""
    nbytes = max(desc.nbytes, 16)
    arena = _RESIZE_ARENA.take(nbytes)
    arena.numpy()[:desc.nbytes] = desc.view(np.uint8).reshape(-1)
    dev = torch.empty(nbytes, dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        dev.copy_(arena[:nbytes], non_blocking=True)
        _RESIZE_ARENA.uploaded()
    return dev


def colour_jitter_u8_prepare(images, specs):
    """everything of colour_jitter_u8 but the launches: a JitterLaunch"""
    assert len(images) == len(specs)
    desc, blocks, slots = _jitter_table(images, specs)
    device = images[0].device if len(images) else torch.device("cuda", torch.cuda.current_device())
    sums = torch.empty(slots, dtype=torch.int64, device=device)      # cleared by the sum call, on the stream
    dev = _jitter_upload(desc, device) if len(desc) else None
    return JitterLaunch(dev, len(desc), blocks, sums, images)


def colour_jitter_u8(images, specs):
    """The training mapper's colour jitters (data.transforms: RandomContrast, RandomBrightness, RandomSaturation,
    RandomLighting, in that order) on device images, in place, to the bytes the host's BlendTransform chain gives.

    images: device uint8 views [3, h, w] with any strides (what resize_u8 returns, or windows of a batch).
    specs: per image the draws, a float64 [4, 4] array / tensor (data.jitter: row t = (drawn, parameters of transform t)) or
      None for an image that drew nothing.
    One pinned upload carries the descriptors; one launch sums the bytes of the images whose contrast was drawn (the image
    mean is formed on the device), one launch applies every transform of every image.  Images that drew nothing are not
    touched; a batch in which nothing was drawn launches nothing.  Returns images."""
    if len(images) == 0:
        return images
    return colour_jitter_u8_prepare(images, specs).launch()


def byte_sum_u8(images):
    """int64 device tensor [n]: the sum of the 3 * h * w bytes of each device uint8 view [3, h, w], one launch for all"""
    if len(images) == 0:
        return torch.empty(0, dtype=torch.int64)
    desc, blocks, slots = _jitter_table(images, [None] * len(images), all_sums=True)
    sums = torch.empty(slots, dtype=torch.int64, device=images[0].device)
    JitterLaunch(_jitter_upload(desc, images[0].device), len(desc), blocks, sums, images).launch_sum()
    return sums


class PackedDlaBase:
    """operands of ctdet_dla_base_fwd: the 7x7 stem [16,3,7,7], level0 [16,16,3,3] and level1 [32,16,3,3] weights with
    their folded BatchNorm (scale, bias) pairs."""

    def __init__(self, w_stem, sb_stem, w_l0, sb_l0, w_l1, sb_l1):
        assert tuple(w_stem.shape) == (16, 3, 7, 7) and tuple(w_l0.shape) == (16, 16, 3, 3) and tuple(w_l1.shape) == (32, 16, 3, 3)
        dev = w_stem.device
        # stem operand: k = (r*8 + s)*4 + c -- 4-channel pixels, kernel rows padded to 8 taps (one MFMA K step per row)
        w4 = torch.zeros(16, 7, 8, 4, dtype=torch.float32, device=dev)
        w4[:, :, :7, :3] = w_stem.detach().float().permute(0, 2, 3, 1)
        self.w0 = w4.reshape(16, 224).to(torch.float16).contiguous()
        self.p1 = PackedConv(w_l0, sb_l0[0], sb_l0[1], stride=1, pad=1, compute=F16)
        self.p2 = PackedConv(w_l1, sb_l1[0], sb_l1[1], stride=2, pad=1, compute=F16)
        assert self.p1.korder == 0 and self.p1.Kpad == 160 and self.p2.korder == 0 and self.p2.Kpad == 160
        self.s0 = sb_stem[0].detach().float().contiguous()
        self.b0 = sb_stem[1].detach().float().contiguous()


class PackedDlaBaseX3:
    """operands of ctdet_dla_base_x3_fwd: the three layers as f16x3 PackedConvs (the split tap-major images of
    ctdet_pack_weights_x3, the stem on 4-channel pixels) -- exactly what the layer-by-layer f16x3 path contracts with."""
    x3 = True

    def __init__(self, w_stem, sb_stem, w_l0, sb_l0, w_l1, sb_l1):
        assert tuple(w_stem.shape) == (16, 3, 7, 7) and tuple(w_l0.shape) == (16, 16, 3, 3) and tuple(w_l1.shape) == (32, 16, 3, 3)
        # stem operand: k = (r*8 + s)*4 + c -- 4-channel pixels, kernel rows padded to 8 taps (a K step = four consecutive
        # taps of a row); packed as the [16, 224, 1, 1] weight of a 1x1 contraction
        w4 = torch.zeros(16, 7, 8, 4, dtype=torch.float32, device=w_stem.device)
        w4[:, :, :7, :3] = w_stem.detach().float().permute(0, 2, 3, 1)
        self.p0 = PackedConv(w4.reshape(16, 224, 1, 1), sb_stem[0], sb_stem[1], compute=F16X3)
        self.p1 = PackedConv(w_l0.detach().float().contiguous(), sb_l0[0], sb_l0[1], stride=1, pad=1, compute=F16X3)
        self.p2 = PackedConv(w_l1.detach().float().contiguous(), sb_l1[0], sb_l1[1], stride=2, pad=1, compute=F16X3)
        for p, kpad, rows in ((self.p0, 224, 16), (self.p1, 144, 16), (self.p2, 144, 32)):
            assert p.korder == 0 and p.Kpad == kpad and p.w.shape[0] >= rows and p.w.shape[1] == kpad, (p.korder, p.Kpad, p.w.shape)
            assert p.scale.numel() >= rows and p.bias.numel() >= rows


BASE_FUSED = os.environ.get("CTDET_NO_FUSED_BASE", "0") != "1"


def dla_base_fused_ok(Hp, Wp):
    return BASE_FUSED and Hp % 16 == 0 and Wp % 32 == 0


def dla_base_fused(images, mean, std, Hp, Wp, p, out=None, pooled=None, mirror=False):
    """images [B,3,H,W] uint8/f32 on device -> level1 output of DLA (NHWC [B,Hp/2,Wp/2,32]; f16, or f32 when p is a
    PackedDlaBaseX3: f16x3 arithmetic) in one launch: normalisation, 7x7 stem, level0, level1 (stride 2), BatchNorm folded,
    ReLU after each.  pooled: optional [B,Hp/4,Wp/4,>=32] buffer of the output's dtype that receives MaxPool2d(2) of the
    output (what level2's Tree starts with).
    mirror (flip test, see preprocess): True = computed from the mirrored network input, which makes the output the plain
    output mirrored; "both" = 2B output images, plain then mirrored, the B images read in place twice."""
    _require_cuda(images, out, pooled)
    B, Cc, H, W = images.shape
    assert Cc == 3 and images.stride(3) == 1 and images.stride(2) == W and images.stride(1) == H * W
    B, mfrom = _mirror_from(mirror, B)
    x3 = getattr(p, "x3", False)
    odt = torch.float32 if x3 else torch.float16
    if out is None:
        out = torch.empty(B, Hp // 2, Wp // 2, 32, dtype=odt, device=images.device)
    assert out.dtype == odt and tuple(out.shape[:3]) == (B, Hp // 2, Wp // 2) and out.shape[3] >= 32
    d = _lib.DlaBaseDesc()
    d.B, d.H, d.W, d.Hp, d.Wp, d.img_dtype = B, H, W, Hp, Wp, dt_of(images)
    d.img_batch_stride = images.stride(0)
    for i in range(3):
        d.mean[i], d.std[i] = float(mean[i]), float(std[i])
    d.out_stride = _nhwc_stride(out)
    if pooled is not None:
        assert pooled.dtype == odt and tuple(pooled.shape[:3]) == (B, Hp // 4, Wp // 4) and pooled.shape[3] >= 32
        d.pool_stride = _nhwc_stride(pooled)
    px = B * Hp * Wp
    prof = _Prof(None, px, False, F16X3 if x3 else F16,
                 flops=2.0 * (px * 16 * 147 + px * 16 * 144 + (px // 4) * 32 * 144))
    L = _lib.lib()
    if x3:
        operands = (_ptr(images), _ptr(p.p0.w), _ptr(p.p0.scale), _ptr(p.p0.bias), _ptr(p.p1.w), _ptr(p.p1.scale),
                    _ptr(p.p1.bias), _ptr(p.p2.w), _ptr(p.p2.scale), _ptr(p.p2.bias), _ptr(out), _ptr(pooled), _stream())
        fn = L.ctdet_dla_base_x3_fwd if mfrom is None else L.ctdet_dla_base_x3_mirror_fwd
    else:
        operands = (_ptr(images), _ptr(p.w0), _ptr(p.s0), _ptr(p.b0), _ptr(p.p1.w), _ptr(p.p1.scale), _ptr(p.p1.bias),
                    _ptr(p.p2.w), _ptr(p.p2.scale), _ptr(p.p2.bias), _ptr(out), _ptr(pooled), _stream())
        fn = L.ctdet_dla_base_fwd if mfrom is None else L.ctdet_dla_base_mirror_fwd
    for _ in range(prof.reps()):
        rc = fn(C.byref(d), *operands) if mfrom is None else fn(C.byref(d), mfrom, *operands)
    _lib.check(rc, "ctdet_dla_base_fwd")
    if prof.on:
        prof.bytes = images.numel() * images.element_size() + (px // 4) * 32 * out.element_size() * (1.25 if pooled is not None else 1.0)
        prof.info = f"M={px} 3->16->16->32 fused"
    prof.done()
    return out


class PackedHeads:
    """weights of the fused CenterNet heads: first convs [256, Cin, 3, 3] + bias per head, final 1x1 convs [cout, 256, 1, 1]
    + bias per head, acts per head.  compute F16: ctdet_head_fused_fwd (f16 activations).  F16X3: ctdet_head_fused_x3_fwd
    (f32 activations) -- the first convs as the korder-3 pair image of the 3x3 halo kernels, the final convs split per row
    into {w_hi, w_lo} after a power-of-two scaling into [1024, 2048) (as every f16x3 operand), b2 = [bias, inverse scale]."""

    HID = 256

    def __init__(self, first_weights, first_biases, final_weights, final_biases, acts, compute=F16):
        n = len(first_weights)
        assert 1 <= n <= 4 and all(w.shape[0] == self.HID and tuple(w.shape[2:]) == (3, 3) for w in first_weights)
        assert all(tuple(w.shape[1:]) == (self.HID, 1, 1) for w in final_weights)
        assert compute in (F16, F16X3)
        dev = first_weights[0].device
        self.n, self.Cin, self.acts, self.compute = n, first_weights[0].shape[1], list(acts), compute
        w1 = torch.cat([w.detach().float() for w in first_weights], 0).contiguous()
        b1 = torch.cat([b.detach().float() for b in first_biases]).contiguous()
        self.couts = [w.shape[0] for w in final_weights]
        self.w2, self.b2 = [], []
        if compute == F16X3:
            assert self.Cin % 32 == 0, "f16x3 fused heads: Cin % 32 == 0"
            self.p1 = PackedConv(w1, None, b1, stride=1, pad=1, compute=F16X3)
            self.w1, self.s1 = self.p1._x3_operand(3)
            self.b1 = self.p1.bias
            for w, b in zip(final_weights, final_biases):
                c = w.shape[0]
                rows = round_up(c, 16)
                wp = torch.zeros(rows, self.HID, dtype=torch.float32, device=dev)
                wp[:c] = w.detach().reshape(c, self.HID).float()
                amax = wp.abs().amax(dim=1)
                e = torch.floor(torch.log2(amax.clamp_min(1e-30)))
                pw = torch.where(amax > 0, torch.exp2(10.0 - e), torch.ones_like(amax))
                ws = wp * pw[:, None]
                hi = ws.to(torch.float16)
                lo = (ws - hi.float()).to(torch.float16)
                self.w2.append(torch.stack([hi, lo], 1).contiguous())          # [rows, 2, 256]
                bp = torch.zeros(2, rows, dtype=torch.float32, device=dev)
                bp[0, :c] = b.detach().float()
                bp[1] = 1.0 / pw
                self.b2.append(bp)
            return
        self.p1 = PackedConv(w1, None, None, stride=1, pad=1, compute=F16)
        assert self.p1.korder == 1 and self.p1.Kpad == 9 * self.Cin
        self.b1 = b1
        for w, b in zip(final_weights, final_biases):
            c = w.shape[0]
            wp = torch.zeros(round_up(c, 16), self.HID, dtype=torch.float16, device=dev)
            wp[:c] = w.detach().reshape(c, self.HID).half()
            bp = torch.zeros(round_up(c, 16), dtype=torch.float32, device=dev)
            bp[:c] = b.detach().float()
            self.w2.append(wp)
            self.b2.append(bp)


def heads_fused_ok(x, compute):
    """may the fused head kernel of `compute` take the NHWC map x? (shapes, strides and alignment: the library's rule,
    ctdet_head_fused_supported; never the batch).  Under RANGE_CHECK the f16x3 heads stay unfused: the fused kernel never
    materialises the hidden map the check reads."""
    if compute not in (F16, F16X3) or x.dtype != _TORCH_DT[F16 if compute == F16 else F32] or (compute == F16X3 and RANGE_CHECK):
        return False
    _, H, W, Cin = x.shape
    return bool(_lib.lib().ctdet_head_fused_supported(compute, H, W, Cin, _nhwc_stride(x), _ptr(x)))


def heads_fused(x, ph, clamp=(0.0, 1.0), outs=None):
    """x NHWC [B,H,W,Cin] (f16 for an F16 pack, f32 for an F16X3 one) -> list of f32 NHWC maps [B,H,W,round_up(cout,4)],
    one per head."""
    _require_cuda(x)
    x3 = ph.compute == F16X3
    assert x.dtype == (torch.float32 if x3 else torch.float16) and x.shape[3] == ph.Cin
    B, H, W, _ = x.shape
    if outs is None:
        outs = [torch.empty(B, H, W, round_up(c, 4), dtype=torch.float32, device=x.device) for c in ph.couts]
    d = HeadDesc()
    d.nheads, d.B, d.H, d.W, d.Cin, d.in_stride = ph.n, B, H, W, ph.Cin, _nhwc_stride(x)
    for h in range(ph.n):
        d.w2[h], d.b2[h], d.y[h] = ph.w2[h].data_ptr(), ph.b2[h].data_ptr(), outs[h].data_ptr()
        d.y_stride[h], d.cout[h], d.act[h] = _nhwc_stride(outs[h]), ph.couts[h], ph.acts[h]
    d.clamp_lo, d.clamp_hi = clamp
    M = B * H * W
    prof = _Prof(None, M, False, F32, flops=sum(2.0 * M * PackedHeads.HID * (9 * ph.Cin + c) for c in ph.couts))
    if prof.on:
        prof.bytes = float(M * 4 * (ph.Cin + sum(round_up(c, 4) for c in ph.couts))) if x3 else prof.bytes
        prof.info = f"M={M} {ph.Cin}->{PackedHeads.HID}->{','.join(str(c) for c in ph.couts)}"
    for _ in range(prof.reps()):
        if x3:
            rc = _lib.lib().ctdet_head_fused_x3_fwd(C.byref(d), _ptr(x), _ptr(ph.w1), _ptr(ph.s1), _ptr(ph.b1), _stream())
        else:
            rc = _lib.lib().ctdet_head_fused_fwd(C.byref(d), _ptr(x), _ptr(ph.p1.w), _ptr(ph.b1), _stream())
    _lib.check(rc, "ctdet_head_fused_x3_fwd" if x3 else "ctdet_head_fused_fwd")
    prof.done()
    return outs


# CTDET_NO_TREE_DEDUP=1: a DLA tree of more than one level runs its unread 1x1 projection and its second max-pool of the same
# input again (modeling/backbone/dla.py: Tree.hip_forward); the A/B switch of their removal
TREE_DEDUP = os.environ.get("CTDET_NO_TREE_DEDUP", "0") != "1"

# CTDET_NO_SPARSE_HEADS=1: the f16x3 eval step computes the wh / reg heads densely again (the launches before heads_sparse existed)
HEADS_SPARSE = os.environ.get("CTDET_NO_SPARSE_HEADS", "0") != "1"


def heads_sparse(y, ph, inds, down_ratio, flip=False):
    """the wh / reg heads at the decoded peaks only, and the decode's boxes from them.  y f32 NHWC [NB,H,W,64] (the heads' input;
    NB = 2B under flip), ph an F16X3 PackedHeads of exactly (wh, reg), inds i32 [B,K] from decode(...).  flip: wh is the mean
    with the mirrored pixel of image b + B, reg image b's (decode's flip rule).  Returns (whreg [B,K,4] = (w, h, off_x, off_y),
    boxes [B,K,4])."""
    _require_cuda(y, inds)
    assert ph.compute == F16X3 and ph.n == 2 and ph.couts == [2, 2], "heads_sparse: a pack of the wh and reg heads"
    assert y.dtype == torch.float32 and y.shape[3] == ph.Cin and inds.dtype == torch.int32 and inds.is_contiguous()
    assert ph.w1.shape[0] >= 2 * PackedHeads.HID and ph.w1.shape[1] == ph.Cin // 32 * 288 and ph.Cin == 64
    NB, H, W, _ = y.shape
    B, K = inds.shape
    assert NB == (2 * B if flip else B) and y.stride(0) == H * W * y.stride(2) and y.stride(1) == W * y.stride(2)
    whreg = torch.empty(B, K, 4, dtype=torch.float32, device=y.device)
    boxes = torch.empty(B, K, 4, dtype=torch.float32, device=y.device)
    d = HeadDesc()
    d.nheads, d.B, d.H, d.W, d.Cin, d.in_stride = 2, B, H, W, ph.Cin, _nhwc_stride(y)
    for h in range(2):
        d.w2[h], d.b2[h], d.cout[h] = ph.w2[h].data_ptr(), ph.b2[h].data_ptr(), ph.couts[h]
    M = (2 if flip else 1) * B * K
    prof = _Prof(None, M, False, F32, flops=2.0 * M * PackedHeads.HID * (9 * ph.Cin + 2) * 2)
    if prof.on:      # algorithmic bytes: the patches once, the two heads' weights once
        prof.bytes = float(M * 9 * ph.Cin * 4 + ph.w1.numel() * 4)
        prof.info = f"peaks={M} {ph.Cin}->{PackedHeads.HID}->2,2 at inds" + (" flip" if flip else "")
    for _ in range(prof.reps()):
        rc = _lib.lib().ctdet_head_sparse_x3_fwd(C.byref(d), _ptr(y), _ptr(ph.w1), _ptr(ph.s1), _ptr(ph.b1), _ptr(inds), K,
                                                 float(down_ratio), int(bool(flip)), _ptr(whreg), _ptr(boxes), _stream())
    _lib.check(rc, "ctdet_head_sparse_x3_fwd")
    prof.done()
    return whreg, boxes


def maxpool3x3s2(x, out=None):
    """F.max_pool2d(x, 3, stride=2, padding=1) on NHWC (BasicStem, resnet.py:341-345)."""
    _require_cuda(x, out)
    B, H, W, Cc = x.shape
    if out is None:
        out = torch.empty(B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cc, dtype=x.dtype, device=x.device)
    rc = _lib.lib().ctdet_maxpool3x3s2(_ptr(x), _ptr(out), dt_of(x), B, H, W, Cc, _nhwc_stride(x), _nhwc_stride(out),
                                       _stream())
    _lib.check(rc, "ctdet_maxpool3x3s2")
    return out


def maxpool3x3s2_ceil(x, out=None):
    """nn.MaxPool2d(3, stride=2, ceil_mode=True) on NHWC (VoVNet stages, vovnet.py:291-292)."""
    _require_cuda(x, out)
    B, H, W, Cc = x.shape
    Ho, Wo = -(-(H - 3) // 2) + 1, -(-(W - 3) // 2) + 1
    if (Ho - 1) * 2 >= H:
        Ho -= 1
    if (Wo - 1) * 2 >= W:
        Wo -= 1
    if out is None:
        out = torch.empty(B, Ho, Wo, Cc, dtype=x.dtype, device=x.device)
    assert tuple(out.shape[:3]) == (B, Ho, Wo)
    rc = _lib.lib().ctdet_maxpool3x3s2_ceil(_ptr(x), _ptr(out), dt_of(x), B, H, W, Cc, _nhwc_stride(x), _nhwc_stride(out),
                                            _stream())
    _lib.check(rc, "ctdet_maxpool3x3s2_ceil")
    return out


# CTDET_NO_FINITE_FOLD=1: the sparse eval step scans the heads' input map with finite_flag again instead of having the DCNv2
# layer that writes it test its own stores (dcnv2_offset(..., finite_flag=)); the A/B switch of that fold
FINITE_FOLD = os.environ.get("CTDET_NO_FINITE_FOLD", "0") != "1"


class FiniteFold:
    """The eval step's finite flag on its way down to the layer that writes the heads' input: `flag` (int32 [1], set to 1
    here) and `folded`, which that layer sets once its kernel has taken the flag -- if no layer did (two-launch DCNv2, range
    check, another backbone, an unsupported shape), the caller scans the map as before."""

    def __init__(self, device):
        self.flag = torch.ones(1, dtype=torch.int32, device=device)
        self.folded = False


def finite_flag(*tensors, flag=None):
    """int32 [1] on the device: 1 if every value of the f32 NHWC maps (channel slices of wider buffers allowed) is finite, else
    0 -- kernels only (no torch reduction: those clear their semaphores with a memset, which a captured step must not hold).
    flag: an existing flag to go on with (it holds 1, or the 0 an earlier test left) instead of a fresh one."""
    _require_cuda(*tensors)
    if flag is None:
        flag = torch.ones(1, dtype=torch.int32, device=tensors[0].device)
    assert flag.dtype == torch.int32 and flag.numel() == 1 and flag.is_cuda
    for t in tensors:
        assert t.dtype == torch.float32 and t.dim() == 4 and t.stride(3) == 1
        B, H, W, Cc = t.shape
        with prof_region("finite_flag", nbytes=float(t.numel() * 4), info="x".join(str(n) for n in t.shape)):
            _lib.check(_lib.lib().ctdet_finite_flag(_ptr(t), B * H * W, Cc, _nhwc_stride(t), _ptr(flag), _stream()), "ctdet_finite_flag")
    return flag


def global_avgpool(x):
    """NHWC x -> f32 [B, C]: the mean over the pixels (nn.AdaptiveAvgPool2d(1) of the eSE module, vovnet.py:203)."""
    _require_cuda(x)
    B, H, W, Cc = x.shape
    out = torch.empty(B, Cc, dtype=torch.float32, device=x.device)
    rc = _lib.lib().ctdet_global_avgpool(_ptr(x), dt_of(x), B, H * W, Cc, _nhwc_stride(x), _ptr(out), _stream())
    _lib.check(rc, "ctdet_global_avgpool")
    return out


def ese_scale(x, s, identity=None, out=None):
    """y = x * hsigmoid(s[b, c]) (+ identity); s f32 [B, C] (vovnet.py:186-213, 268-271)."""
    _require_cuda(x, s, identity, out)
    B, H, W, Cc = x.shape
    s = s.contiguous()
    assert s.dtype == torch.float32 and tuple(s.shape) == (B, Cc)
    if out is None:
        out = torch.empty(B, H, W, Cc, dtype=x.dtype, device=x.device)
    if identity is not None:
        assert identity.dtype == x.dtype and tuple(identity.shape) == tuple(x.shape)
    rc = _lib.lib().ctdet_ese_scale(_ptr(x), _nhwc_stride(x), _ptr(s), _ptr(identity),
                                    _nhwc_stride(identity) if identity is not None else 0, _ptr(out), _nhwc_stride(out),
                                    dt_of(x), B, H * W, Cc, _stream())
    _lib.check(rc, "ctdet_ese_scale")
    return out


def conv_transpose2d(x, weight, scale, bias, stride, padding, compute, act=ACT_NONE, cache=None):
    """Dense nn.ConvTranspose2d (weight [Cin, Cout, k, k], output_padding 0) + per-channel scale/bias + act on NHWC:
    a stride-1 convolution with the flipped kernel over the zero-stuffed input (pad k-1-p); the kernels read the
    input as zero-stuffed in place (`in_dil`)."""
    _require_cuda(x, weight)
    Cin, Cout, k, k2 = weight.shape
    assert k == k2 and x.shape[3] == Cin
    p = cache.get("p") if cache is not None else None
    if p is None:
        wc = weight.detach().flip(2, 3).permute(1, 0, 2, 3).contiguous()  # [Cout, Cin, k, k]
        p = PackedConv(wc, scale, bias, stride=1, pad=k - 1 - padding, compute=compute, tap_major=True)
        if cache is not None:
            cache["p"] = p
    B, H, W, _ = x.shape
    Ho, Wo = (H - 1) * stride - 2 * padding + k, (W - 1) * stride - 2 * padding + k
    out = torch.empty(B, Ho, Wo, p.Cout_eff, dtype=x.dtype, device=x.device)
    p.in_dil = stride
    return conv2d(x, p, out=out, act=act)


def maxpool2x2(x, out=None):
    _require_cuda(x, out)
    B, H, W, Cc = x.shape
    if out is None:
        out = torch.empty(B, H // 2, W // 2, Cc, dtype=x.dtype, device=x.device)
    rc = _lib.lib().ctdet_maxpool2x2(_ptr(x), _ptr(out), dt_of(x), B, H, W, Cc, _nhwc_stride(x), _nhwc_stride(out),
                                     _stream())
    _lib.check(rc, "ctdet_maxpool2x2")
    return out


def _dw_weight(weight, Cc, f, fresh=False):
    """[C,1,2f,2f] -> f32 [2f,2f,C]; cached on the tensor object itself (an address-keyed cache would go stale
    when the allocator reuses a freed block)."""
    if fresh:
        # training: always re-derive from the live parameter -- a captured training step would otherwise replay with
        # the copy made at capture time
        return weight.detach().reshape(Cc, 2 * f, 2 * f).to(torch.float32).permute(1, 2, 0).contiguous()
    hit = getattr(weight, "_ctdet_dw", None)
    if hit is None or hit[0] != (weight.data_ptr(), weight._version):
        packed = weight.detach().reshape(Cc, 2 * f, 2 * f).to(torch.float32).permute(1, 2, 0).contiguous()
        hit = ((weight.data_ptr(), weight._version), packed)
        try:
            weight._ctdet_dw = hit
        except AttributeError:
            pass
    return hit[1]


def dwconvT_add(x, weight, f, skip=None, out=None, fresh_weight=False, prepared=None):
    """ConvTranspose2d(C,C,2f,stride=f,padding=f//2,groups=C)(x) + skip; weight f32 [C,1,2f,2f] or [C,2f,2f];
    prepared: its [2f,2f,C] f32 form if the caller already made it"""
    _require_cuda(x, weight, skip, out)
    B, H, W, Cc = x.shape
    w = prepared if prepared is not None else _dw_weight(weight, Cc, f, fresh_weight)
    if out is None:
        out = torch.empty(B, H * f, W * f, Cc, dtype=x.dtype, device=x.device)
    rc = _lib.lib().ctdet_dwconvT_add(_ptr(x), _ptr(w), _ptr(skip), _ptr(out), dt_of(x), B, H, W, Cc, f,
                                      _nhwc_stride(x), _nhwc_stride(skip) if skip is not None else 0,
                                      _nhwc_stride(out), _stream())
    _lib.check(rc, "ctdet_dwconvT_add")
    return out


def dw3_weight(weight, fresh=False):
    """Conv2d(C, C, 3, groups=C) weight [C,1,3,3] -> f32 tap-major [9][C] (t = ky*3 + kx), the layout of ctdet_dwconv3x3_fwd;
    cached on the tensor like _dw_weight.  fresh: re-derived from the live parameter (training: a captured step must not
    replay with the copy of capture time)."""
    Cc = weight.shape[0]
    assert tuple(weight.shape) == (Cc, 1, 3, 3), f"depthwise 3x3 weight expected, got {tuple(weight.shape)}"
    if fresh:
        return weight.detach().reshape(Cc, 9).to(torch.float32).t().contiguous()
    hit = getattr(weight, "_ctdet_dw3", None)
    if hit is None or hit[0] != (weight.data_ptr(), weight._version):
        hit = ((weight.data_ptr(), weight._version), weight.detach().reshape(Cc, 9).to(torch.float32).t().contiguous())
        try:
            weight._ctdet_dw3 = hit
        except AttributeError:
            pass
    return hit[1]


def dwconv3x3(x, weight, stride, out=None, rot180=False, prepared=None):
    """Conv2d(C, C, 3, stride, padding=1, groups=C, bias=False)(x) on NHWC x (f16 or f32; may be a channel slice), weight
    [C,1,3,3]; out: an NHWC tensor (or channel slice) of the output shape to write into.  rot180: the taps rotated by 180
    degrees (with stride 1: the input gradient of the layer for x = dY).  prepared: the weight's [9][C] f32 form if the
    caller already made it."""
    _require_cuda(x, weight, out)
    B, H, W, Cc = x.shape
    w = prepared if prepared is not None else dw3_weight(weight)
    assert w.shape == (9, Cc) and w.dtype == torch.float32 and w.is_contiguous()
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    if out is None:
        out = torch.empty(B, Ho, Wo, Cc, dtype=x.dtype, device=x.device)
    assert tuple(out.shape) == (B, Ho, Wo, Cc) and out.dtype == x.dtype
    with prof_region(f"dwconv3x3<s{stride}>", flops=2.0 * 9 * B * Ho * Wo * Cc,
                     nbytes=float(x.element_size() * (B * H * W + B * Ho * Wo) * Cc), info=f"{H}x{W} C={Cc}"):
        rc = _lib.lib().ctdet_dwconv3x3_fwd(_ptr(x), _nhwc_stride(x), _ptr(w), _ptr(out), _nhwc_stride(out), B, H, W, Cc,
                                            stride, int(rot180), dt_of(x), _stream())
    _lib.check(rc, "ctdet_dwconv3x3_fwd")
    return out


class DecodeWorkspace:
    """candidate lists of ctdet_decode for a (B, H, W, C, K) problem"""

    def __init__(self, B, H, W, Cc, K, device):
        n = _lib.lib().ctdet_decode_workspace_bytes(B, H, W, Cc, K)
        self.key = (B, H, W, Cc, K)
        self.buf = torch.empty(n // 4, dtype=torch.int32, device=device)


SIGMOID_CLAMP_FLOOR = 1e-4     # `_sigmoid`'s lower clamp (centernet.py:13-15); the head kernels' epilogue writes exactly this f32


def decode(heat, wh, reg, K, down_ratio, workspace=None, check_status=False, heat_floor=0.0, flip=False):
    """Batched ctdet_decode. heat f32 NHWC [B,H,W,C] (may be the channel slice [..., :C] of a wider buffer: padded head
    outputs are decoded in place); wh/reg f32 NHWC (2 channels, may be slices).  heat_floor: a lower bound of the positive
    heat values the caller vouches for (SIGMOID_CLAMP_FLOOR for a clamped map; same results, the background plateau is
    skipped).
    flip (flip test): heat / wh / reg hold 2B images, image b + B being the network's maps for the horizontally mirrored
    input of image b; decoded are hm = (hm[b] + mirror(hm[b+B])) * 0.5, wh = (wh[b] + mirror(wh[b+B])) * 0.5 and reg = reg[b]
    (mirror: x <-> W-1-x; one f32 add and one multiply in that order), merged inside the decode's one pass over the maps.
    wh = reg = None: the map-free mode -- scores, classes and inds as always, `boxes` comes back unwritten, for
    heads_sparse(..., inds) to supply.
    Returns boxes [B,K,4], scores [B,K], classes [B,K] (int32), inds [B,K] (int32)."""
    _require_cuda(heat, wh, reg)
    assert heat.dtype == torch.float32
    B, H, W, Cc = heat.shape
    assert wh is not None or reg is None, "decode: reg without wh"
    if flip:
        assert B % 2 == 0 and (wh is None or wh.shape[0] == B) and (reg is None or reg.shape[0] == B), \
            "flip decode: 2B images, plain half first"
        assert heat.stride(0) == H * W * heat.stride(2) and (wh is None or wh.stride(0) == H * W * wh.stride(2)), \
            "flip decode: dense batches"
        B //= 2
    if workspace is None or workspace.key != (B, H, W, Cc, K):
        workspace = DecodeWorkspace(B, H, W, Cc, K, heat.device)
    dev = heat.device
    boxes = torch.empty(B, K, 4, dtype=torch.float32, device=dev)
    scores = torch.empty(B, K, dtype=torch.float32, device=dev)
    classes = torch.empty(B, K, dtype=torch.int32, device=dev)
    inds = torch.empty(B, K, dtype=torch.int32, device=dev)
    with prof_region("decode", nbytes=float(B * H * W * Cc * 4), info=f"{B}x{H}x{W}x{Cc} K={K}"):
        fn = _lib.lib().ctdet_decode_flip if flip else _lib.lib().ctdet_decode
        rc = fn(_ptr(heat), _nhwc_stride(heat), _ptr(wh), _nhwc_stride(wh) if wh is not None else 0, _ptr(reg),
                _nhwc_stride(reg) if reg is not None else 0, B, H, W, Cc, K, float(down_ratio),
                float(heat_floor), _ptr(workspace.buf), _ptr(boxes), _ptr(scores), _ptr(classes), _ptr(inds), _stream())
    _lib.check(rc, "ctdet_decode")
    if check_status:
        _lib.check(_lib.lib().ctdet_decode_status(_ptr(workspace.buf), B, H, W, Cc, K, _stream()), "ctdet_decode_status")
    return boxes, scores, classes, inds


def postprocess(boxes, scores, classes, max_det, score_thresh, img_params):
    """Batched threshold + rescale + clip + drop-empty, order preserving. img_params f32 [B,4] on device
    = (scale_x, scale_y, out_w, out_h).  Returns compacted (boxes, scores, classes, counts[B] i32)."""
    _require_cuda(boxes, scores, classes, img_params)
    B, K = scores.shape
    ob, os_, oc = torch.empty_like(boxes), torch.empty_like(scores), torch.empty_like(classes)
    counts = torch.empty(B, dtype=torch.int32, device=boxes.device)
    rc = _lib.lib().ctdet_postprocess(_ptr(boxes), _ptr(scores), _ptr(classes), B, K, int(max_det), float(score_thresh),
                                      _ptr(img_params), _ptr(ob), _ptr(os_), _ptr(oc), _ptr(counts), _stream())
    _lib.check(rc, "ctdet_postprocess")
    return ob, os_, oc, counts


def postprocess_affine(boxes, scores, classes, max_det, score_thresh, img_params6, out=None):
    """ops.postprocess for a batch whose network input was an affine warp of the original image (INPUT.AFFINE.TEST_MODE,
    DESIGN.md 7.13): threshold + unwarp + clip + drop-empty, order preserving.  img_params6 f32 [B,6] on device = (sx, sy, tx,
    ty, orig_w, orig_h), data.warp.unwarp_params per image; x' = f32(f32(x * sx) + tx), bit for bit
    data.warp.unwarp_boxes_reference.  Returns compacted (boxes, scores, classes, counts[B] i32): fresh tensors, or `out`, a
    tuple of four the caller owns (rows behind counts[b] are left as they were)."""
    _require_cuda(boxes, scores, classes, img_params6)
    B, K = scores.shape
    assert boxes.dtype == scores.dtype == img_params6.dtype == torch.float32 and classes.dtype == torch.int32
    assert tuple(boxes.shape) == (B, K, 4) and tuple(classes.shape) == (B, K), (tuple(boxes.shape), tuple(classes.shape))
    assert tuple(img_params6.shape) == (B, 6) and img_params6.is_contiguous(), (
        f"postprocess_affine: img_params6 is a contiguous f32 [{B}, 6] tensor, got {tuple(img_params6.shape)}")
    assert boxes.is_contiguous() and scores.is_contiguous() and classes.is_contiguous()
    if out is None:
        out = (torch.empty_like(boxes), torch.empty_like(scores), torch.empty_like(classes),
               torch.empty(B, dtype=torch.int32, device=boxes.device))
    ob, os_, oc, counts = out
    _require_cuda(ob, os_, oc, counts)
    for t, like in ((ob, boxes), (os_, scores), (oc, classes)):
        assert t.shape == like.shape and t.dtype == like.dtype and t.is_contiguous(), "postprocess_affine: out mirrors the inputs"
    assert tuple(counts.shape) == (B,) and counts.dtype == torch.int32 and counts.is_contiguous()
    rc = _lib.lib().ctdet_postprocess_affine(_ptr(boxes), _ptr(scores), _ptr(classes), B, K, int(max_det), float(score_thresh),
                                             _ptr(img_params6), _ptr(ob), _ptr(os_), _ptr(oc), _ptr(counts), _stream())
    _lib.check(rc, "ctdet_postprocess_affine")
    return ob, os_, oc, counts


def soft_nms_merge(passes, num_classes, sigma, min_score, max_det):
    """Multi-scale test augmentation's merge: per-class Gaussian soft-NMS over the union of the passes'
    detections, then the per-image cap, on the device.  passes: a list of (boxes f32 [B,K_s,4], scores f32 [B,K_s], classes
    i32 [B,K_s], counts i32 [B]) device tuples in one frame -- what an eval step returns -- read in place when contiguous, as an
    eval step's are (a non-contiguous tensor is copied first; K_s may differ per pass; the counts are never read on the host).
    Candidates are ordered pass-major; ties of the score go to the earlier one.
    An image with a count of -1 in any pass (the engine's non-finite flag) gets the count -1.
    Returns fresh (boxes [B,max_det,4], scores [B,max_det], classes [B,max_det] i32, counts [B] i32), best score first."""
    passes = [tuple(p) for p in passes]
    if not passes:
        raise ValueError("soft_nms_merge: no pass to merge")
    _require_cuda(*[t for p in passes for t in p])
    B, dev = passes[0][3].shape[0], passes[0][0].device
    table = (_lib.SoftNmsPass * len(passes))()
    keep = []
    for i, (boxes, scores, classes, counts) in enumerate(passes):
        K = scores.shape[1]
        if not (boxes.dtype == torch.float32 and scores.dtype == torch.float32 and classes.dtype == torch.int32 and
                counts.dtype == torch.int32):
            raise ValueError(f"soft_nms_merge: pass {i}: boxes / scores must be f32, classes / counts i32")
        if not (tuple(boxes.shape) == (B, K, 4) and tuple(scores.shape) == (B, K) and tuple(classes.shape) == (B, K) and
                tuple(counts.shape) == (B,)):
            raise ValueError(f"soft_nms_merge: pass {i} is not ([B,K,4], [B,K], [B,K], [B]) with B={B}")
        ts = [t.contiguous() for t in (boxes, scores, classes, counts)]
        keep.append(ts)
        table[i].boxes, table[i].scores, table[i].classes, table[i].counts = (t.data_ptr() for t in ts)
        table[i].K = K
    total = sum(int(table[i].K) for i in range(len(passes)))
    md = max(int(max_det), 0)
    ws = torch.empty(max(B * total * 2, 1), dtype=torch.int32, device=dev)
    ob = torch.empty(B, md, 4, dtype=torch.float32, device=dev)
    os_ = torch.empty(B, md, dtype=torch.float32, device=dev)
    oc = torch.empty(B, md, dtype=torch.int32, device=dev)
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    rc = _lib.lib().ctdet_soft_nms_merge(table, len(passes), B, int(num_classes), float(sigma), float(min_score), int(max_det),
                                         _ptr(ws), _ptr(ob), _ptr(os_), _ptr(oc), _ptr(counts), _stream())
    _lib.check(rc, "ctdet_soft_nms_merge")
    return ob, os_, oc, counts


def gaussian_targets(boxes, classes, counts, H, W, num_classes, hm=None):
    """Batched gen_heatmap. boxes f32 [B,Nmax,4], classes i64 [B,Nmax], counts i32 [B].
    Returns dict(hm [B,H,W,C] NHWC f32, wh [B,128,2], reg [B,128,2], ind [B,128] i64, reg_mask [B,128] u8)."""
    _require_cuda(boxes, classes, counts)
    B, Nmax, _ = boxes.shape
    dev = boxes.device
    assert boxes.dtype == torch.float32 and classes.dtype == torch.int64 and counts.dtype == torch.int32
    boxes, classes = boxes.contiguous(), classes.contiguous()
    if hm is None:
        hm = torch.empty(B, H, W, num_classes, dtype=torch.float32, device=dev)
    wh = torch.empty(B, 128, 2, dtype=torch.float32, device=dev)
    reg = torch.empty(B, 128, 2, dtype=torch.float32, device=dev)
    ind = torch.empty(B, 128, dtype=torch.int64, device=dev)
    reg_mask = torch.empty(B, 128, dtype=torch.uint8, device=dev)
    rc = _lib.lib().ctdet_gaussian_targets(_ptr(boxes), _ptr(classes), _ptr(counts), B, Nmax, H, W, num_classes,
                                           _ptr(hm), _ptr(wh), _ptr(reg), _ptr(ind), _ptr(reg_mask), _stream())
    _lib.check(rc, "ctdet_gaussian_targets")
    return {"hm": hm, "wh": wh, "reg": reg, "ind": ind, "reg_mask": reg_mask}


def gaussian_radius(hw_pairs):
    """hw_pairs i32 [n,2] (h, w) on device -> (radius f64 [n], int radius i32 [n])."""
    _require_cuda(hw_pairs)
    n = hw_pairs.shape[0]
    r = torch.empty(n, dtype=torch.float64, device=hw_pairs.device)
    ri = torch.empty(n, dtype=torch.int32, device=hw_pairs.device)
    rc = _lib.lib().ctdet_gaussian_radius(_ptr(hw_pairs.contiguous()), n, _ptr(r), _ptr(ri), _stream())
    _lib.check(rc, "ctdet_gaussian_radius")
    return r, ri


def focal_loss(logits, gt, alpha, want_grad=True, grad_scale=1.0):
    """_neg_loss on sigmoid+clamp of logits. logits/gt f32 NHWC [B,H,W,C]; alpha f32 [C].
    Returns (loss [1], stats [4] = pos, neg, num_pos, 1/num_pos, grad or None)."""
    _require_cuda(logits, gt, alpha)
    assert logits.is_contiguous() and gt.is_contiguous() and logits.shape == gt.shape
    B, H, W, Cc = logits.shape
    dev = logits.device
    ws = torch.empty(_lib.lib().ctdet_focal_loss_workspace_bytes(logits.numel()) // 4, dtype=torch.float32, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    stats = torch.empty(4, dtype=torch.float32, device=dev)
    grad = torch.empty_like(logits) if want_grad else None
    rc = _lib.lib().ctdet_focal_loss(_ptr(logits), _ptr(gt), _ptr(alpha), B, H, W, Cc, float(grad_scale), _ptr(ws),
                                     _ptr(loss), _ptr(stats), _ptr(grad), _stream())
    _lib.check(rc, "ctdet_focal_loss")
    return loss, stats, grad


def reg_l1_loss(pred, mask, ind, target, want_grad=True, grad_scale=1.0, grad=None):
    """RegL1Loss. pred f32 NHWC [B,H,W,2] (may be a channel slice); mask u8 [B,N]; ind i64 [B,N]; target [B,N,2]."""
    _require_cuda(pred, mask, ind, target)
    B, H, W, _ = pred.shape
    N = mask.shape[1]
    dev = pred.device
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    if want_grad and grad is None:
        grad = torch.zeros(B, H, W, 2, dtype=torch.float32, device=dev)
    rc = _lib.lib().ctdet_reg_l1_loss(_ptr(pred), _nhwc_stride(pred), _ptr(mask.contiguous()), _ptr(ind.contiguous()),
                                      _ptr(target.contiguous()), B, N, H * W, float(grad_scale), _ptr(loss),
                                      _ptr(grad) if want_grad else C.c_void_p(0),
                                      _nhwc_stride(grad) if want_grad else 0, _stream())
    _lib.check(rc, "ctdet_reg_l1_loss")
    return loss, grad


def sgd_momentum_(param, grad, buf, lr_dev, momentum, weight_decay, first_step):
    """In-place fused SGD step on flat f32 tensors; lr_dev is a 1-element device tensor."""
    _require_cuda(param, grad, buf, lr_dev)
    assert param.is_contiguous() and grad.is_contiguous() and buf.is_contiguous()
    rc = _lib.lib().ctdet_sgd_momentum(_ptr(param), _ptr(grad), _ptr(buf), param.numel(), _ptr(lr_dev),
                                       float(momentum), float(weight_decay), int(bool(first_step)), _stream())
    _lib.check(rc, "ctdet_sgd_momentum")


def sgd_momentum_runs_(param, grad, buf, run_end, run_lr_index, run_wd, lr_table, momentum, first_step):
    """one launch over a flat buffer of consecutive hyper-parameter runs (see ctdet_sgd_momentum_runs)"""
    _require_cuda(param, grad, buf, run_end, run_lr_index, run_wd, lr_table)
    assert param.is_contiguous() and grad.is_contiguous() and buf.is_contiguous()
    assert run_end.dtype == torch.int64 and run_lr_index.dtype == torch.int32
    rc = _lib.lib().ctdet_sgd_momentum_runs(_ptr(param), _ptr(grad), _ptr(buf), param.numel(), _ptr(run_end),
                                            _ptr(run_lr_index), _ptr(run_wd), _ptr(lr_table), run_end.numel(),
                                            float(momentum), int(bool(first_step)), _stream())
    _lib.check(rc, "ctdet_sgd_momentum_runs")


def grad_chunk_norms_(grad, chunk_start, chunk_len, norm_type, partials):
    """pass 1 of the per-parameter gradient norms: partials[c] = sum g^2 / sum |g| / max |g| (norm_type: _lib.NORM_*) over
    chunk c of the flat gradient buffer (see ctdet_grad_chunk_norms)"""
    _require_cuda(grad, chunk_start, chunk_len, partials)
    assert grad.is_contiguous() and grad.dtype == torch.float32 and partials.dtype == torch.float32
    assert chunk_start.dtype == torch.int64 and chunk_len.dtype == torch.int32
    assert chunk_start.numel() == chunk_len.numel() == partials.numel()
    rc = _lib.lib().ctdet_grad_chunk_norms(_ptr(grad), grad.numel(), _ptr(chunk_start), _ptr(chunk_len), chunk_start.numel(),
                                           int(norm_type), _ptr(partials), _stream())
    _lib.check(rc, "ctdet_grad_chunk_norms")


def grad_clip_coefs_(partials, param_chunk_end, norm_type, clip_value, norms, coefs):
    """pass 2: norms[q] from the partials of parameter q's chunks, coefs[q] = min(1, clip_value / (norms[q] + 1e-6))"""
    _require_cuda(partials, param_chunk_end, norms, coefs)
    assert param_chunk_end.dtype == torch.int32 and norms.dtype == coefs.dtype == torch.float32
    assert param_chunk_end.numel() == norms.numel() == coefs.numel()
    rc = _lib.lib().ctdet_grad_clip_coefs(_ptr(partials), _ptr(param_chunk_end), param_chunk_end.numel(), partials.numel(),
                                          int(norm_type), float(clip_value), _ptr(norms), _ptr(coefs), _stream())
    _lib.check(rc, "ctdet_grad_clip_coefs")


def sgd_momentum_runs_clip_(param, grad, buf, run_end, run_lr_index, run_wd, lr_table, momentum, first_step, nesterov=False,
                            clip_type=_lib.CLIP_NONE, clip_value=0.0, coefs=None):
    """sgd_momentum_runs_ with per-parameter clipping (by value, or by the coefficients of grad_clip_coefs_: one run per
    parameter then) and / or Nesterov momentum (see ctdet_sgd_momentum_runs_clip); `grad` is left as it is"""
    _require_cuda(param, grad, buf, run_end, run_lr_index, run_wd, lr_table)
    assert param.is_contiguous() and grad.is_contiguous() and buf.is_contiguous()
    assert run_end.dtype == torch.int64 and run_lr_index.dtype == torch.int32
    if clip_type == _lib.CLIP_NORM:
        _require_cuda(coefs)
        assert coefs.dtype == torch.float32 and coefs.numel() == run_end.numel()
    else:
        coefs = None
    rc = _lib.lib().ctdet_sgd_momentum_runs_clip(_ptr(param), _ptr(grad), _ptr(buf), param.numel(), _ptr(run_end),
                                                 _ptr(run_lr_index), _ptr(run_wd), _ptr(lr_table), run_end.numel(),
                                                 float(momentum), int(bool(first_step)), int(bool(nesterov)), int(clip_type),
                                                 float(clip_value), _ptr(coefs), _stream())
    _lib.check(rc, "ctdet_sgd_momentum_runs_clip")


def adam_advance_(step_count, bias, beta1, beta2):
    """the first launch of an Adam step: step_count[0] += 1 (i64, device) and bias = [1 / (1 - beta1^t), 1 / sqrt(1 - beta2^t)]
    (see ctdet_adam_advance) -- a kernel, so that a captured step keeps counting when it is replayed"""
    _require_cuda(step_count, bias)
    assert step_count.dtype == torch.int64 and step_count.numel() == 1
    assert bias.dtype == torch.float32 and bias.numel() == 2 and bias.is_contiguous()
    rc = _lib.lib().ctdet_adam_advance(_ptr(step_count), _ptr(bias), float(beta1), float(beta2), _stream())
    _lib.check(rc, "ctdet_adam_advance")


def adam_runs_(param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq, run_end, run_lr_index, run_wd, lr_table, bias, beta1, beta2,
               eps, decoupled=False, amsgrad=False, clip_type=_lib.CLIP_NONE, clip_value=0.0, coefs=None):
    """one launch of Adam (decoupled: AdamW; amsgrad: with the running maximum `max_exp_avg_sq`) over a flat buffer of
    consecutive hyper-parameter runs, clipped like sgd_momentum_runs_clip_ (see ctdet_adam_runs); `grad` is left as it is,
    `bias` is what adam_advance_ wrote"""
    _require_cuda(param, grad, exp_avg, exp_avg_sq, run_end, run_lr_index, run_wd, lr_table, bias)
    state = [param, grad, exp_avg, exp_avg_sq]
    if amsgrad:
        _require_cuda(max_exp_avg_sq)
        state.append(max_exp_avg_sq)
    else:
        max_exp_avg_sq = None
    assert all(t.is_contiguous() and t.dtype == torch.float32 and t.numel() == param.numel() for t in state)
    assert run_end.dtype == torch.int64 and run_lr_index.dtype == torch.int32
    assert bias.dtype == torch.float32 and bias.numel() == 2
    if clip_type == _lib.CLIP_NORM:
        _require_cuda(coefs)
        assert coefs.dtype == torch.float32 and coefs.numel() == run_end.numel()
    else:
        coefs = None
    rc = _lib.lib().ctdet_adam_runs(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), _ptr(max_exp_avg_sq), param.numel(),
                                    _ptr(run_end), _ptr(run_lr_index), _ptr(run_wd), _ptr(lr_table), run_end.numel(), _ptr(bias),
                                    float(beta1), float(beta2), float(eps), int(bool(decoupled)), int(bool(amsgrad)),
                                    int(clip_type), float(clip_value), _ptr(coefs), _stream())
    _lib.check(rc, "ctdet_adam_runs")


def ema_advance_(updates, weight, decay, warmup):
    """the first launch of an EMA update: t = updates[0], updates[0] = t + 1 (i64, device) and weight[0] = 1 - d with
    d = min(decay, (1 + t) / (10 + t)) under warm-up, else decay (see ctdet_ema_advance) -- a kernel, so that a captured step
    keeps counting when it is replayed"""
    _require_cuda(updates, weight)
    assert updates.dtype == torch.int64 and updates.numel() == 1
    assert weight.dtype == torch.float32 and weight.numel() == 1
    rc = _lib.lib().ctdet_ema_advance(_ptr(updates), _ptr(weight), float(decay), int(bool(warmup)), _stream())
    _lib.check(rc, "ctdet_ema_advance")


def _ema_tables(live_ptrs, ema, seg_start):
    _require_cuda(live_ptrs, ema, seg_start)
    assert live_ptrs.dtype == torch.int64 and seg_start.dtype == torch.int64 and live_ptrs.is_contiguous()
    assert seg_start.is_contiguous() and seg_start.numel() == live_ptrs.numel() + 1
    assert ema.dtype == torch.float32 and ema.is_contiguous()


def ema_lerp_segments_(live_ptrs, ema, seg_start, max_len, weight):
    """ema[seg_start[s] + i] += weight[0] * (live[s][i] - ema[seg_start[s] + i]) in torch's lerp_ form, over the device tables
    `live_ptrs` (i64 addresses of f32 data, one per segment) and `seg_start` (i64, one more entry than segments); `max_len`
    bounds the segment lengths (see ctdet_ema_lerp_segments)"""
    _ema_tables(live_ptrs, ema, seg_start)
    _require_cuda(weight)
    assert weight.dtype == torch.float32 and weight.numel() == 1
    rc = _lib.lib().ctdet_ema_lerp_segments(_ptr(live_ptrs), _ptr(ema), _ptr(seg_start), live_ptrs.numel(), int(max_len),
                                            _ptr(weight), _stream())
    _lib.check(rc, "ctdet_ema_lerp_segments")


def ema_swap_segments_(live_ptrs, ema, seg_start, max_len):
    """exchanges live[s][i] and ema[seg_start[s] + i] bit for bit over the same tables (see ctdet_ema_swap_segments)"""
    _ema_tables(live_ptrs, ema, seg_start)
    rc = _lib.lib().ctdet_ema_swap_segments(_ptr(live_ptrs), _ptr(ema), _ptr(seg_start), live_ptrs.numel(), int(max_len),
                                            _stream())
    _lib.check(rc, "ctdet_ema_swap_segments")


def _precise_bn_tables(mean_ptrs, var_ptrs, seg_start, buf, lead):
    """the checks the two PreciseBN wrappers share; `buf` is the f64 state / slot buffer whose leading dimensions are `lead`"""
    for name, t in (("mean_ptrs", mean_ptrs), ("var_ptrs", var_ptrs), ("seg_start", seg_start)):
        if t.dtype != torch.int64:
            raise TypeError(f"precise_bn: {name} must be int64, got {t.dtype}")
        if t.dim() != 1 or not t.is_contiguous():
            raise ValueError(f"precise_bn: {name} must be a contiguous vector")
    if buf.dtype != torch.float64:
        raise TypeError(f"precise_bn: the state must be float64, got {buf.dtype}")
    nseg = mean_ptrs.numel()
    if var_ptrs.numel() != nseg or seg_start.numel() != nseg + 1:
        raise ValueError(f"precise_bn: {nseg} mean pointers go with {nseg} variance pointers and {nseg + 1} offsets, got "
                         f"{var_ptrs.numel()} and {seg_start.numel()}")
    if buf.dim() != len(lead) + 1 or tuple(buf.shape[:-1]) != tuple(lead) or not buf.is_contiguous():
        raise ValueError(f"precise_bn: the state must be a contiguous [{', '.join(map(str, lead))}, total] tensor, got "
                         f"{tuple(buf.shape)}")
    _require_cuda(mean_ptrs, var_ptrs, seg_start, buf)
    if len({t.device for t in (mean_ptrs, var_ptrs, seg_start, buf)}) != 1:
        raise ValueError("precise_bn: the tables and the state must live on one device")
    return nseg, buf.shape[-1]


def precise_bn_rows(rows):
    """the per-segment row counts of one batch as a CPU int64 vector; a count below 2 raises ValueError naming its index (a
    batch statistic over one row has no unbiased variance: torch refuses a training-mode BatchNorm over one value per channel
    for the same reason)"""
    if not isinstance(rows, torch.Tensor):
        rows = torch.tensor([r.__index__() for r in rows], dtype=torch.int64)      # integers only: a float has no __index__
    rows = rows.cpu()
    if rows.dtype != torch.int64:
        raise TypeError(f"precise_bn: rows must be int64, got {rows.dtype}")
    rows = rows.reshape(-1)
    bad = (rows < 2).nonzero()
    if bad.numel():
        i = int(bad[0])
        raise ValueError(f"precise_bn: rows[{i}] = {int(rows[i])}: every segment needs at least 2 rows per batch")
    return rows


def precise_bn_merge_(mean_ptrs, var_ptrs, seg_start, rows, max_len, state, rows_dev=None):
    """folds one batch into the f64 state [3, total] = (n, mean, M2) per channel (see ctdet_precise_bn_merge_segments): segment
    s reads its batch mean from the f32 data at address mean_ptrs[s], its unbiased batch variance at var_ptrs[s] and its row
    count from rows[s].  `mean_ptrs` / `var_ptrs` / `seg_start` are device int64 tables as for ema_lerp_segments_.  `rows`: the
    host's counts (a sequence or CPU int64 tensor), checked here; `rows_dev`: their device copy where the caller keeps one
    (None: uploaded here)."""
    rows = precise_bn_rows(rows)
    if rows.numel() != mean_ptrs.numel():
        raise ValueError(f"precise_bn_merge_: {mean_ptrs.numel()} segments, {rows.numel()} row counts")
    nseg, total = _precise_bn_tables(mean_ptrs, var_ptrs, seg_start, state, (3,))
    if rows_dev is None:
        rows_dev = rows.to(state.device)
    if rows_dev.dtype != torch.int64 or rows_dev.numel() != nseg or not rows_dev.is_contiguous() or rows_dev.device != state.device:
        raise ValueError("precise_bn_merge_: rows_dev must be the contiguous int64 device copy of rows")
    rc = _lib.lib().ctdet_precise_bn_merge_segments(_ptr(mean_ptrs), _ptr(var_ptrs), _ptr(seg_start), _ptr(rows_dev), nseg,
                                                    int(max_len), _ptr(state), total, _stream())
    _lib.check(rc, "ctdet_precise_bn_merge_segments")


def precise_bn_finish_(mean_ptrs, var_ptrs, seg_start, max_len, slots):
    """combines the rank slots of the f64 buffer [world, 3, total] in rank order and writes (float)mean to the f32 data at
    mean_ptrs[s], the population variance (float)(M2 / n) at var_ptrs[s]; channels without rows keep their values (see
    ctdet_precise_bn_finish_segments).  The written tensors are raw addresses: the caller bumps their versions."""
    if slots.dim() != 3:
        raise ValueError(f"precise_bn_finish_: slots must be [world, 3, total], got {tuple(slots.shape)}")
    nseg, total = _precise_bn_tables(mean_ptrs, var_ptrs, seg_start, slots, (slots.shape[0], 3))
    rc = _lib.lib().ctdet_precise_bn_finish_segments(_ptr(mean_ptrs), _ptr(var_ptrs), _ptr(seg_start), nseg, int(max_len),
                                                     _ptr(slots), slots.shape[0], total, _stream())
    _lib.check(rc, "ctdet_precise_bn_finish_segments")
