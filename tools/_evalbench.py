"""What the bench_*eval.py dev tools share: the windowed HIP-event timer, and the raw-call idiom of the two that time the entry
points of a side library on their own (pointers, f64 uploads, the 256-byte aligned workspace, the current stream)."""
import ctypes as C

import numpy as np
import torch


def timed(fn, warmup, iters, repeats):
    """ms per call: the mean of each of `repeats` windows of `iters` calls"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return out


def ptr(t):
    return C.c_void_p(t.data_ptr())


def f64(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def workspace(nbytes, dev):
    """nbytes of a *_workspace_bytes entry point -> (owning tensor, 256-byte aligned address)"""
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
    return ws, C.c_void_p((ws.data_ptr() + 255) & ~255)


def stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
