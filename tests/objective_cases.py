"""Case tables and float64 references for the kernels that define the training objective -- gaussian_targets, focal_loss,
reg_l1_loss (csrc/train_ops.hip) -- and for the eval step's guard finite_flag (csrc/pointwise.hip).  Every shape is the
smallest at which the branch named next to it is taken.  test_objective_host.py checks the tables against their own
conditions on the CPU; test_objective_gpu.py runs the kernels over them.

References: the project's oracle (oracle/ctdet_oracle.py) evaluated in float64 under autograd, gen_heatmap as it is, and
torch.isfinite(slice).all() on the CPU.  The inputs are f32 values (the alpha weights included), so the kernel and the reference
start from the same numbers.
"""
import functools
import math
from collections import namedtuple

import numpy as np
import torch

from oracle import ctdet_oracle as O

FL_VEC_PER_BLOCK = 256 * 8            # train_ops.hip: 4-element vectors per workgroup of focal_main_kernel
FL_FINALIZE_THREADS = 256             # focal_finalize_kernel: block partials taken per pass of its strided loop
ZERO_GRID_CAP = 2048                  # zero_f32_kernel: workgroups (of 256 float4 stores) at the most
FINITE_GRID_CAP = 4096                # finite_flag_kernel: workgroups (of 256 elements) at the most
CLAMP_LOGIT = math.log(9999.0)        # sigmoid(+-CLAMP_LOGIT) = 1 - 1e-4 / 1e-4: the clamp of centernet.py:204
CLAMP_MARGIN = 1e-3                   # no logit this close to the clamp: the gradient jumps there, f32 and f64 may disagree
FLT_MAX = 3.4028234663852886e38

# ------------------------------------------------------------------------------------------------------------------------
# focal loss
# ------------------------------------------------------------------------------------------------------------------------
FocalCase = namedtuple("FocalCase", "B C H W with_pos pinned")

FOCAL_SHAPES = [          # (B, C, H, W) as the oracle sees them (NCHW); the kernel gets NHWC
    (1, 1, 6, 10),        # C < 4
    (1, 2, 5, 6),         # C < 4
    (2, 3, 14, 18),       # C no multiple of 4: 4-vectors straddle pixels
    (1, 5, 6, 10),        # as above
    (1, 7, 4, 8),         # as above
    (1, 80, 16, 20),      # the model's class count; 6400 vectors = 3 full blocks and a ragged fourth
    (2, 80, 101, 130),    # 525 200 vectors = 257 blocks, the last one ragged: the finalize loop takes a second pass
]
FOCAL_PINNED_SHAPE = (2, 3, 14, 18)   # this shape (with positives) carries the two logits beyond the clamp
FOCAL_CASES = [FocalCase(*s, wp, wp and s == FOCAL_PINNED_SHAPE) for s in FOCAL_SHAPES for wp in (True, False)]
FOCAL_RAISES = (1, 3, 5, 7)           # 105 elements, no multiple of 4: the launcher must refuse it
PIN_LOGIT = 12.0


def focal_id(c):
    return f"{c.B}x{c.C}x{c.H}x{c.W}-{'pos' if c.with_pos else 'nopos'}{'-pinned' if c.pinned else ''}"


def straddling_element(C, numel):
    """flat NHWC index of an element that lies in a later pixel, and in another class, than the first element of its 4-vector
    (None where no vector straddles: C a multiple of 4, or one class).  Searched from the middle of the map on."""
    if C % 4 == 0 or C == 1:
        return None
    for v in range(numel // 8, numel // 4):
        for e in (4 * v + 3, 4 * v + 2, 4 * v + 1):
            if e // C != (4 * v) // C and (e - 4 * v) % C != 0:
                return e
    return None


@functools.lru_cache(maxsize=None)
def focal_inputs(case):
    """dict: logits, gt f32 NHWC [B,H,W,C]; alpha f32 [C] (distinct values 0.25 + k/C, shuffled); marks: flat NHWC indices of the
    positives and pinned logits that the case promises"""
    B, C, H, W = case.B, case.C, case.H, case.W
    g = torch.Generator().manual_seed(1000 + 7 * C + H + W + (1 if case.with_pos else 0))
    numel = B * H * W * C
    logits = torch.randn(numel, generator=g) * 3 - 2
    while True:       # redraw the values next to the clamp
        near = ((logits.abs() - CLAMP_LOGIT).abs() < 2 * CLAMP_MARGIN).nonzero().flatten()
        if near.numel() == 0:
            break
        logits[near] = torch.randn(near.numel(), generator=g) * 3 - 2
    gt = torch.rand(numel, generator=g) ** 4
    alpha = torch.tensor([0.25 + k / C for k in range(C)], dtype=torch.float32)[torch.randperm(C, generator=g)]
    marks = {}
    if case.with_pos:
        gt[torch.randint(0, numel, (max(2, numel // 400),), generator=g)] = 1.0
        marks["last_class"] = numel - 1                    # class C-1 of the last pixel: in the last (ragged) block
        marks["first_class"] = (numel // (2 * C)) * C      # class 0 of a pixel in the middle
        e = straddling_element(C, numel)
        if e is not None:
            marks["straddle"] = e
        for e in marks.values():
            gt[e] = 1.0
        if case.pinned:
            marks["pin_pos"], marks["pin_neg"] = 5, 6
            gt[5], gt[6] = 1.0, 0.3
            logits[5], logits[6] = PIN_LOGIT, -PIN_LOGIT
    return {"logits": logits.view(B, H, W, C), "gt": gt.view(B, H, W, C), "alpha": alpha, "marks": marks}


def _focal_reference(case, dtype):
    inp = focal_inputs(case)
    x = inp["logits"].permute(0, 3, 1, 2).clone().to(dtype).requires_grad_(True)
    gt = inp["gt"].permute(0, 3, 1, 2).to(dtype)
    loss = O.focal_loss_from_logits(x, gt, inp["alpha"].double().tolist())
    loss.backward()
    with torch.no_grad():     # all-zero weights leave the negative sum alone: -neg / num_pos (or -neg without positives)
        loss0 = O.focal_loss_from_logits(x.detach(), gt, [0.0] * case.C)
    num_pos = int((inp["gt"] == 1).sum())
    scale = float(num_pos) if num_pos else 1.0
    neg = -loss0.item() * scale
    pos = -loss.item() * scale - neg if num_pos else 0.0
    return {"loss": loss.item(), "grad": x.grad.permute(0, 2, 3, 1).contiguous(), "pos": pos, "neg": neg, "num_pos": num_pos}


@functools.lru_cache(maxsize=None)
def focal_reference(case):
    """the oracle in float64: loss, grad (NHWC f64), pos sum, neg sum, num_pos"""
    return _focal_reference(case, torch.float64)


def focal_reference_f32(case):
    return _focal_reference(case, torch.float32)


# ------------------------------------------------------------------------------------------------------------------------
# gaussian targets
# ------------------------------------------------------------------------------------------------------------------------
# dropped: (image, slot) of the boxes whose centre lies outside the map -- the kernel's documented behaviour is to drop the object
# and zero its slot.  oob_class: (image, slot) of the objects whose class id is outside [0, C) -- slot written, nothing drawn.
TargetCase = namedtuple("TargetCase", "name H W C boxes classes counts prefill dropped oob_class")


def _edges_case():
    """H = 24 < W = 40 (input 96 x 160), C = 5, B = 3, Nmax = 6.  Image 0 lists seven objects for six slots: the two identical
    boxes of one class are the ordinary box and its twin."""
    H, W, C, Nmax = 24, 40, 5, 6
    boxes = torch.zeros(3, Nmax, 4)
    classes = torch.zeros(3, Nmax, dtype=torch.int64)
    img0 = [([30.0, 20.0, 70.0, 52.0], 1),            # an ordinary box
            ([30.0, 20.0, 70.0, 52.0], 1),            # ... and an identical one of the same class
            ([156.0, 92.0, 159.9, 95.9], 4),          # the bottom-right corner: ind = 23 * 40 + 39 = 959
            ([10.0, 10.0, 10.5, 10.5], 0),            # radius 0
            ([-40.0, -40.0, 200.0, 140.0], 2),        # larger than the map, centre inside
            ([80.0, 30.0, 120.0, 70.0], 5)]           # class id out of range
    img2 = [([-30.0, 40.0, 10.0, 60.0], 0),           # centre x = -2.5
            ([-12.0, 40.0, 8.0, 60.0], 1),            # centre x = -0.5: the oracle truncates it to column 0 and keeps it
            ([40.0, -30.0, 60.0, 10.0], 2),           # centre y = -2.5
            ([150.0, 40.0, 180.0, 60.0], 3),          # centre x = 41.25 >= W
            ([40.0, 90.0, 60.0, 110.0], 4),           # centre y = 25 >= H
            ([60.0, 30.0, 100.0, 62.0], 3)]           # an ordinary box among them
    for k, (bx, c) in enumerate(img0):
        boxes[0, k], classes[0, k] = torch.tensor(bx), c
        boxes[1, k], classes[1, k] = torch.tensor(bx), min(c, C - 1)       # image 1: counts = 0, its rows must be ignored
    for k, (bx, c) in enumerate(img2):
        boxes[2, k], classes[2, k] = torch.tensor(bx), c
    counts = torch.tensor([6, 0, 9], dtype=torch.int32)                    # 9 > Nmax behaves as Nmax
    return TargetCase("edges_24x40", H, W, C, boxes, classes, counts, False,
                      frozenset((2, k) for k in range(5)), frozenset({(0, 5)}))


def _tail_case():
    """105 floats: the zero kernel's scalar tail (n & 3 = 1) runs; the map is caller-owned and holds NaN"""
    boxes = torch.tensor([[[2.0, 2.0, 14.0, 12.0], [16.0, 8.0, 27.9, 19.9], [0.0, 0.0, 28.0, 20.0], [4.0, 4.0, 20.0, 16.0]]])
    classes = torch.tensor([[0, 2, 1, 2]])
    return TargetCase("tail_5x7", 5, 7, 3, boxes, classes, torch.tensor([3], dtype=torch.int32), True, frozenset(), frozenset())


def _wrap_case():
    """2.6 M floats = 655 360 vectors > 2048 x 256: the zero kernel's grid-stride loop wraps; NaN-filled map, a dozen boxes"""
    B, C, size, Nmax = 2, 80, 512, 6
    g = torch.Generator().manual_seed(77)
    wh = torch.rand(B, Nmax, 2, generator=g) * 200 + 8
    ctr = torch.rand(B, Nmax, 2, generator=g) * (size - wh) + wh / 2
    boxes = torch.cat([ctr - wh / 2, ctr + wh / 2], 2)
    classes = torch.randint(0, C, (B, Nmax), generator=g)
    classes[1, Nmax - 1] = C - 1
    return TargetCase("wrap_128x128", size // 4, size // 4, C, boxes, classes, torch.tensor([Nmax, Nmax], dtype=torch.int32),
                      True, frozenset(), frozenset())


TARGET_CASES = [_edges_case(), _tail_case(), _wrap_case()]


def target_objects(case, b):
    """the number of objects the kernel looks at in image b"""
    return min(int(case.counts[b]), case.boxes.shape[1], 128)


@functools.lru_cache(maxsize=None)
def _target_reference(name):
    case = next(c for c in TARGET_CASES if c.name == name)
    out = {k: [] for k in ("hm", "wh", "reg", "ind", "reg_mask")}
    for b in range(case.boxes.shape[0]):
        n = target_objects(case, b)
        boxes, classes = case.boxes[b, :n].clone(), case.classes[b, :n].clone()
        for (bb, k) in case.dropped:
            if bb == b and k < n:
                boxes[k] = 0.0                      # a zero-area box: the oracle skips it and leaves its slot zero
        keep = [k for k in range(n) if (b, k) not in case.oob_class]
        hm = O.gen_heatmap(boxes[keep], classes[keep], case.H, case.W, case.C)["hm"]      # the map: without that object
        for (bb, k) in case.oob_class:
            if bb == b and k < n:
                classes[k] = 0                      # the slot outputs: as if it had class 0
        slots = O.gen_heatmap(boxes, classes, case.H, case.W, case.C)
        out["hm"].append(hm)
        for key in ("wh", "reg", "ind", "reg_mask"):
            out[key].append(slots[key])
    return {k: np.stack(v) for k, v in out.items()}


def target_reference(case):
    """gen_heatmap per image: hm [B,C,H,W] f32, wh / reg [B,128,2], ind [B,128] i64, reg_mask [B,128] u8 -- all 128 slots"""
    return _target_reference(case.name)


# ------------------------------------------------------------------------------------------------------------------------
# RegL1Loss on channel slices of wider buffers
# ------------------------------------------------------------------------------------------------------------------------
RegCase = namedtuple("RegCase", "B N S lo")       # pred = buf[..., lo:lo+2] of a [B, REG_H, REG_W, S] buffer
REG_H, REG_W = 6, 10
REG_CASES = [RegCase(B, N, S, lo)
             for (B, N) in ((1, 5), (3, 128), (2, 37))          # B*N = 5 < 256 (one pass), 384 > 256 (two passes), 74
             for S in (4, 8) for lo in (0, 2)]
REG_GRAD_SCALES = (1.0, 1024.0)


def reg_id(c):
    return f"B{c.B}-N{c.N}-stride{c.S}-ch{c.lo}"


@functools.lru_cache(maxsize=None)
def reg_inputs(case):
    """dict: buf f32 [B,H,W,S]; mask u8 [B,N]; ind i64 [B,N]; target f32 [B,N,2]; ref_mask / ref_ind: the same with the entries at
    out-of-range indices masked off (the kernel ignores them; the oracle's gather would raise)"""
    B, N, S, lo = case
    HW = REG_H * REG_W
    g = torch.Generator().manual_seed(300 + 13 * N + S + lo)
    buf = torch.randn(B, REG_H, REG_W, S, generator=g)
    mask = (torch.rand(B, N, generator=g) < 0.3).to(torch.uint8)
    ind = torch.randint(0, HW, (B, N), generator=g)
    tgt = torch.randn(B, N, 2, generator=g)
    ind[0, 1] = ind[0, 0]
    mask[0, 0] = mask[0, 1] = 1                  # duplicate index: the gradients accumulate
    ind[0, 2], mask[0, 2] = HW, 1                # mask 1 at the first index past the map
    mask[0, 3] = 1                               # pred == target exactly in component 0: sign 0
    tgt[0, 3, 0] = buf[0].view(HW, S)[ind[0, 3], lo]
    mask[0, 4] = 0
    oob = [(0, 2)]
    if N > 5:
        ind[B - 1, N - 1], mask[B - 1, N - 1] = -1, 1
        oob.append((B - 1, N - 1))
    ref_mask, ref_ind = mask.clone(), ind.clone()
    for (b, k) in oob:
        ref_mask[b, k], ref_ind[b, k] = 0, 0
    return {"buf": buf, "mask": mask, "ind": ind, "target": tgt, "ref_mask": ref_mask, "ref_ind": ref_ind, "oob": oob}


def reg_reference(case, zero_mask=False, dtype=torch.float64):
    """the oracle under autograd: loss, and the gradient with respect to the whole buffer [B,H,W,S] (zero outside the slice)"""
    inp = reg_inputs(case)
    buf = inp["buf"].clone().to(dtype).requires_grad_(True)
    pred = buf[..., case.lo:case.lo + 2].permute(0, 3, 1, 2)
    mask = torch.zeros_like(inp["ref_mask"]) if zero_mask else inp["ref_mask"]
    loss = O.reg_l1_loss(pred, mask, inp["ref_ind"], inp["target"].to(dtype))
    loss.backward()
    return {"loss": loss.item(), "grad": buf.grad}


# ------------------------------------------------------------------------------------------------------------------------
# finite_flag on channel slices
# ------------------------------------------------------------------------------------------------------------------------
FiniteCase = namedtuple("FiniteCase", "shape lo hi")      # the slice [..., lo:hi] of an f32 buffer of this NHWC shape
FINITE_CASES = [
    FiniteCase((2, 100, 1, 4), 0, 2),           # the decoded [B, K, 1, 4] size / offset rows
    FiniteCase((5, 128, 128, 16), 0, 13),       # 1 064 960 elements > 4096 x 256: the grid-stride loop takes a second pass
    FiniteCase((2, 9, 7, 4), 1, 2),             # a one-channel slice
]
FINITE_WAYS = ["finite", "nan_first", "inf_last", "ninf_middle", "bad_outside", "second_bad"]


def finite_id(c):
    return "x".join(str(n) for n in c.shape) + f"-ch{c.lo}to{c.hi}"


def finite_numel(case):
    return case.shape[0] * case.shape[1] * case.shape[2] * (case.hi - case.lo)


@functools.lru_cache(maxsize=None)
def _finite_base(case):
    g = torch.Generator().manual_seed(500 + case.shape[1])
    buf = torch.randn(*case.shape, generator=g)
    _set_slice_element(case, buf, 1, FLT_MAX)
    _set_slice_element(case, buf, finite_numel(case) - 2, -FLT_MAX)
    return buf


def _set_slice_element(case, buf, i, value):
    """element i of the slice, in the kernel's order (pixel-major, channel-minor)"""
    Cs = case.hi - case.lo
    buf.view(-1, case.shape[3])[i // Cs, case.lo + i % Cs] = value


def finite_buffers(case, way):
    """the full buffers (one, or two for "second_bad") whose [..., lo:hi] slices go to one finite_flag call"""
    n = finite_numel(case)
    buf = _finite_base(case).clone()
    if way == "finite":
        return [buf]
    if way == "nan_first":
        _set_slice_element(case, buf, 0, float("nan"))
    elif way == "inf_last":
        _set_slice_element(case, buf, n - 1, float("inf"))
    elif way == "ninf_middle":
        _set_slice_element(case, buf, n // 2, float("-inf"))
    elif way == "bad_outside":              # every channel outside the slice: the flag must stay 1
        outside = [c for c in range(case.shape[3]) if not case.lo <= c < case.hi]
        buf[..., outside[0::2]] = float("inf")
        buf[..., outside[1::2]] = float("nan")
    elif way == "second_bad":
        _set_slice_element(case, buf, n // 3, float("nan"))
        return [_finite_base(case).clone(), buf]
    else:
        raise ValueError(way)
    return [buf]


def finite_reference(case, buffers):
    return int(all(bool(torch.isfinite(b[..., case.lo:case.hi]).all()) for b in buffers))
