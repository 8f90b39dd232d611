"""The depthwise 3x3 case table (tests/dwconv_cases.py) validated on the CPU: its constants are dwconv.hip's, every row has the
property it is there for, the nine-shifted-products reference is torch's float64 convolution, and the bound admits an f32
evaluation and rejects wrong ones.  Nothing here needs a GPU."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import dwconv_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _const(name):
    src = open(os.path.join(ROOT, "detectron2-centernet_amd", "csrc", "dwconv.hip")).read()
    return int(re.search(r"constexpr int " + name + r" = (\d+);", src).group(1))


def test_constants_and_geometry_are_the_kernels():
    assert (_const("DW3_ROWS"), _const("WG3_ROWS"), _const("WG3_MAX_GROUPS")) == (D.DW3_ROWS, D.WG3_ROWS, D.WG3_MAX_GROUPS)
    src = open(os.path.join(ROOT, "detectron2-centernet_amd", "csrc", "dwconv.hip")).read()
    # wgrad_geom, restated in dwconv_cases: the lines it restates
    for line in ("g.XL = 256 / (C / N);", "g.ncol = (W + g.XL - 1) / g.XL;", "g.nstrip = (H + WG3_ROWS - 1) / WG3_ROWS;",
                 "const long nt = (long)B * g.ncol * g.nstrip;", "g.G = (int)(nt < WG3_MAX_GROUPS ? nt : WG3_MAX_GROUPS);",
                 "for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x)", "const int i = blockIdx.x * 256 + threadIdx.x;"):
        assert line in src, line
    assert D.wgrad_geom(2, 33, 47, 96, 4) == (10, 5, 3, 30, 30)
    assert D.wgrad_geom(0, 33, 47, 96, 4)[3:] == (0, 0)


def test_forward_rows_have_their_properties():
    rows = {r[0]: r for r in D.FWD_ROWS}
    assert len(rows) == len(D.FWD_ROWS)
    assert {(rows[n][3], rows[n][4]) for n in ("1x1", "1x9", "9x1", "2x2")} == {(1, 1), (1, 9), (9, 1), (2, 2)}
    assert {(r[3], r[4]) for r in D.FWD_ROWS if r[0].startswith("s2 ")} == {(4, 6), (5, 6), (4, 7), (5, 7)}
    assert all(r[5] == (2,) for r in D.FWD_ROWS if r[0].startswith("s2 "))
    # Ho at, one above, at twice and one above twice the rows a thread walks: the last strip of two of them holds one row
    hs = [rows[n][3] for n in ("H4", "H5", "H8", "H9")]
    assert hs == [D.DW3_ROWS, D.DW3_ROWS + 1, 2 * D.DW3_ROWS, 2 * D.DW3_ROWS + 1] and all(rows[n][5] == (1,) for n in rows if n[0] == "H")
    assert [h % D.DW3_ROWS for h in hs] == [0, 1, 0, 1] and D.DW3_ROWS - 1 in [h % D.DW3_ROWS for h in (hs[0] - 1, hs[2] - 1)]
    # the seam: 20 channel vectors (f32 C = 80, f16 C = 160), Wo = 13 -> 260 threads, thread 256 is vector 16 of pixel 12
    for n in ("seam", "seam s2"):
        _, B, CV, H, W, strides = rows[n]
        Wo = D.out_size(W, strides[0])
        assert (CV, Wo) == (20, 13) and Wo * CV == 260 and 256 // CV == 12 and 256 % CV != 0
        assert CV * D.VEC[torch.float32] == 80 and CV * D.VEC[torch.float16] == 160
    assert rows["Cmin"][2] == 1 and rows["Cmax"][2] == 256                     # C / N <= 256 is the launcher's limit
    assert (rows["Cmin"][3], rows["Cmin"][4]) == (3, 5) == (rows["Cmax"][3], rows["Cmax"][4])
    _, B, CV, H, W, strides = rows["B3"]
    assert B == 3 and -(-H // D.DW3_ROWS) > 1                                  # several strips per image in blockIdx.y
    assert set(D.SLICE_ROWS) == {"9x1", "seam"} and rows["9x1"][4] == 1
    assert all(1 in r[5] or 2 in r[5] for r in D.FWD_ROWS) and any(r[5] == (1, 2) for r in D.FWD_ROWS)


def test_wgrad_rows_have_their_properties():
    rows = {r[0]: r for r in D.WGRAD_ROWS}
    assert len(rows) == len(D.WGRAD_ROWS) and {"1x1", "1x9", "9x1", "2x2", "seam", "Cmin", "Cmax", "B3"} <= set(rows)
    assert [rows[n][3] for n in ("H16", "H17", "H33")] == [D.WG3_ROWS, D.WG3_ROWS + 1, 2 * D.WG3_ROWS + 1]
    for name, extra in (("W=XL", 0), ("W=XL+1", 1)):
        _, B, CV, H, W = rows[name]
        XL, ncol, _, _, _ = D.wgrad_geom(B, H, W, CV * 4, 4)
        assert W == XL + extra and ncol == 1 + extra
    _, B, CV, H, W = rows["W=2XL"]
    XL, ncol, _, _, _ = D.wgrad_geom(B, H, W, CV * 4, 4)
    assert W == 2 * XL and ncol == 2
    for name, B, CV, H, W in D.WGRAD_ROWS:                                      # none of the small rows reaches the cap
        for N in (4, 8):
            _, _, _, ntiles, G = D.wgrad_geom(B, H, W, CV * N, N)
            assert G == ntiles < D.WG3_MAX_GROUPS
    assert set(D.BEHAVIOUR_SMALL) <= set(rows)
    # the rows where the cap binds: workgroups take two and three tiles
    for name, dtype, B, C, H, W, want_tiles, second, third in D.CAPPED_ROWS:
        XL, ncol, nstrip, ntiles, G = D.wgrad_geom(B, H, W, C, D.VEC[dtype])
        assert ntiles == want_tiles and G == D.WG3_MAX_GROUPS, (name, ntiles, G)
        loads = [len(range(g, ntiles, G)) for g in range(G)]
        assert sum(l >= 2 for l in loads) == second and sum(l >= 3 for l in loads) == third and max(loads) == (3 if third else 2)
        assert D.wgrad_depth(B, H, W, C, D.VEC[dtype]) == D.WG3_ROWS * max(loads) + XL
        assert B * H * W * C <= 22 * 10 ** 6
    name, dtype, B, C, H, W = D.CAPPED_ROWS[0][:6]
    assert D.wgrad_geom(B, H, W, C, 4)[0] == 1                                  # one column a tile: XL = 1
    name, dtype, B, C, H, W = D.CAPPED_ROWS[2][:6]
    XL, ncol, nstrip, _, _ = D.wgrad_geom(B, H, W, C, 8)
    assert XL == 12 and W - (ncol - 1) * XL == 5 and H - (nstrip - 1) * D.WG3_ROWS == 1   # a partial last tile both ways


def test_wgrad_entry_refuses_null_pointers_of_a_non_empty_problem():
    """x and dy may be null only when the problem is empty (the tensors of an empty batch have no storage); dw never.  The
    checks come before any device work: none of these calls reaches a launch."""
    import ctypes
    from detectron2_centernet_amd import _lib
    l = _lib.lib()
    one = ctypes.c_void_p(16)
    assert l.ctdet_dwconv3x3_wgrad(None, 8, one, 8, one, one, 1.0, 0, 1, 5, 6, 8, 1, 1, None) == -22
    assert b"null" in l.ctdet_last_error()
    assert l.ctdet_dwconv3x3_wgrad(one, 8, None, 8, one, one, 1.0, 0, 1, 5, 6, 8, 1, 1, None) == -22
    assert b"null" in l.ctdet_last_error()
    assert l.ctdet_dwconv3x3_wgrad(None, 8, None, 8, None, None, 1.0, 0, 0, 5, 6, 8, 1, 1, None) == -22
    assert b"null" in l.ctdet_last_error()
    assert l.ctdet_dwconv3x3_wgrad_workspace_bytes(0, 5, 6, 8, 1) == 0


def _nchw(t):
    return t.permute(0, 3, 1, 2)


@pytest.mark.parametrize("dtype", D.DTYPES)
def test_reference_is_torchs_convolution_and_bound_admits_f32(dtype):
    """the shifted-product reference against float64 F.conv2d / conv_transpose2d / conv2d_weight on every small row; torch's own
    f32 kernels inside the tolerance, and an unrotated input gradient, a shifted window and a dropped tap outside it"""
    N = D.VEC[dtype]
    f16 = dtype == torch.float16
    worst = {"fwd": 0.0, "dx": 0.0, "dw": 0.0}
    rejected = {"unrotated": 0, "shifted": 0, "dropped tap": 0}
    for k, (name, B, CV, H, W, strides) in enumerate(D.FWD_ROWS):
        C = CV * N
        x, w, dy = D.make_inputs(100 + k, dtype, B, H, W, C, with_dy=True)
        for stride in strides:
            ref, mag = D.fwd_ref(x, w, stride)
            t64 = F.conv2d(_nchw(x).double(), w.double(), None, stride, 1, 1, C).permute(0, 2, 3, 1)
            assert (ref - t64).abs().max() <= 1e-13 * max(1.0, float(mag.max()))
            t32 = F.conv2d(_nchw(x), w, None, stride, 1, 1, C).permute(0, 2, 3, 1)
            got = t32.to(dtype).float() if f16 else t32
            worst["fwd"] = max(worst["fwd"], D.worst_ratio(got, ref, D.fwd_tol(ref, mag, f16)))
        if 1 in strides:
            ref, mag = D.fwd_ref(dy, w, 1, rot180=True)
            t64 = F.conv_transpose2d(_nchw(dy).double(), w.double(), None, 1, 1, 0, C).permute(0, 2, 3, 1)
            assert (ref - t64).abs().max() <= 1e-13 * max(1.0, float(mag.max()))
            t32 = F.conv_transpose2d(_nchw(dy), w, None, 1, 1, 0, C).permute(0, 2, 3, 1)
            worst["dx"] = max(worst["dx"], D.worst_ratio(t32.to(dtype).float() if f16 else t32, ref, D.fwd_tol(ref, mag, f16)))
            tol = D.fwd_tol(ref, mag, f16)
            if H * W > 1:
                rejected["unrotated"] += int(((D.fwd_ref(dy, w, 1)[0] - ref).abs() > tol).any())
    for k, (name, B, CV, H, W) in enumerate(D.WGRAD_ROWS):
        C = CV * N
        x, w, dy = D.make_inputs(200 + k, dtype, B, H, W, C, with_dy=True)
        ref, mag = D.wgrad_ref(x, dy)
        t64 = torch.nn.grad.conv2d_weight(_nchw(x).double(), w.shape, _nchw(dy).double(), 1, 1, 1, C)
        assert (ref - t64).abs().max() <= 1e-12 * max(1.0, float(mag.max()))
        t32 = torch.nn.grad.conv2d_weight(_nchw(x).contiguous(), w.shape, _nchw(dy).contiguous(), 1, 1, 1, C)
        tol = D.wgrad_tol(ref, mag, D.wgrad_depth(B, H, W, C, N))
        worst["dw"] = max(worst["dw"], D.worst_ratio(t32, ref, tol))
        if W > 2:
            shifted = D.wgrad_ref(torch.roll(x, 1, 2), dy)[0]
            rejected["shifted"] += int(((shifted - ref).abs() > tol).any())
        if B * H * W > 1:
            dropped = D.wgrad_ref(x[:, :, :-1] if W > 1 else x[:, :-1], dy[:, :, :-1] if W > 1 else dy[:, :-1])[0]
            rejected["dropped tap"] += int(((dropped - ref).abs() > tol).any())
    print(dtype, "torch f32 / tolerance", {k: round(v, 3) for k, v in worst.items()}, "wrong references rejected on", rejected)
    assert max(worst.values()) < 1.0
    assert rejected["unrotated"] >= 10 and rejected["shifted"] >= 5 and rejected["dropped tap"] >= 10
