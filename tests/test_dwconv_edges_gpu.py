"""The depthwise 3x3 kernels (csrc/dwconv.hip) at their edges against float64 (tests/dwconv_cases.py; the table and the
reference are validated on the CPU by tests/test_dwconv_edges_host.py): maps one pixel wide or high, odd and even sizes at
stride 2, row-strip boundaries, a workgroup seam inside a pixel, the smallest and largest channel counts, channel-slice
views, and the weight gradient where its grid hits WG3_MAX_GROUPS and workgroups loop over two and three tiles.

Tolerances are the derived ones of dwconv_cases (2 * 9 u sum |w| |x|, plus one f16 output rounding; 2 D u sum |dy| |x| with D
the depth of the weight gradient's summation shape); every test prints its worst error / tolerance."""
import pytest
import torch

import dwconv_cases as D

pytestmark = pytest.mark.gpu


def _fwd(x, w, stride, rot180, dtype, dev, out=None):
    import detectron2_centernet_amd.ops as ops
    return ops.dwconv3x3(x.to(dtype).to(dev) if not x.is_cuda else x, w.to(dev), stride, out=out, rot180=rot180)


@pytest.mark.parametrize("dtype", D.DTYPES)
def test_forward_and_input_gradient_edges(dev, dtype):
    N, f16 = D.VEC[dtype], dtype == torch.float16
    worst = (0.0, "")
    for k, (name, B, CV, H, W, strides) in enumerate(D.FWD_ROWS):
        C = CV * N
        x, w, _ = D.make_inputs(300 + k, dtype, B, H, W, C)
        for stride in strides:
            for rot180 in ((False, True) if stride == 1 else (False,)):
                y = _fwd(x, w, stride, rot180, dtype, dev)
                assert y.dtype == dtype and tuple(y.shape) == (B, D.out_size(H, stride), D.out_size(W, stride), C)
                ref, mag = D.fwd_ref(x, w, stride, rot180)
                r = D.worst_ratio(y.float().cpu(), ref, D.fwd_tol(ref, mag, f16))
                worst = max(worst, (r, f"{name} s{stride} rot{int(rot180)}"))
                assert r < 1.0, (name, stride, rot180, r)
                assert torch.equal(y, _fwd(x, w, stride, rot180, dtype, dev))         # the same bits on a second launch
    print(dtype, "forward / input gradient: worst error / tolerance %.3f (%s)" % worst)


@pytest.mark.parametrize("dtype", D.DTYPES)
def test_forward_channel_slices(dev, dtype):
    """input and output as channel slices of wider buffers, on the 1-wide map and on the seam case: outside the output slice
    only sentinels, unchanged (16-element offsets keep the 16-byte alignment in both dtypes)"""
    N, f16 = D.VEC[dtype], dtype == torch.float16
    for k, name in enumerate(D.SLICE_ROWS):
        _, B, CV, H, W, strides = D.fwd_row(name)
        C = CV * N
        x, w, _ = D.make_inputs(400 + k, dtype, B, H, W, C)
        xb = torch.full((B, H, W, C + 48), 1e4, dtype=dtype, device=dev)                # anything read outside the slice shows
        xb[..., 16:16 + C] = x.to(dtype).to(dev)
        for stride in (1, 2):
            for rot180 in ((False, True) if stride == 1 else (False,)):
                Ho, Wo = D.out_size(H, stride), D.out_size(W, stride)
                ob = torch.full((B, Ho, Wo, C + 32), 7.0, dtype=dtype, device=dev)
                y = _fwd(xb[..., 16:16 + C], w, stride, rot180, dtype, dev, out=ob[..., 16:16 + C])
                assert y.data_ptr() == ob[..., 16:16 + C].data_ptr()
                ref, mag = D.fwd_ref(x, w, stride, rot180)
                r = D.worst_ratio(ob[..., 16:16 + C].float().cpu(), ref, D.fwd_tol(ref, mag, f16))
                print(dtype, name, f"s{stride} rot{int(rot180)} slices: error / tolerance {r:.3f}")
                assert r < 1.0, (name, stride, rot180, r)
                assert (ob[..., :16] == 7.0).all() and (ob[..., 16 + C:] == 7.0).all()
                assert (xb[..., :16] == 1e4).all() and (xb[..., 16 + C:] == 1e4).all()


@pytest.mark.parametrize("dtype", D.DTYPES)
def test_wgrad_small_rows(dev, dtype):
    from detectron2_centernet_amd import ops_train
    N = D.VEC[dtype]
    worst = (0.0, "")
    for k, (name, B, CV, H, W) in enumerate(D.WGRAD_ROWS):
        C = CV * N
        x, _, dy = D.make_inputs(500 + k, dtype, B, H, W, C, with_dy=True)
        got = ops_train.dwconv3x3_wgrad(x.to(dtype).to(dev), dy.to(dtype).to(dev), scale=1.0)
        assert tuple(got.shape) == (C, 1, 3, 3) and got.dtype == torch.float32
        ref, mag = D.wgrad_ref(x, dy)
        r = D.worst_ratio(got.cpu(), ref, D.wgrad_tol(ref, mag, D.wgrad_depth(B, H, W, C, N)))
        worst = max(worst, (r, name))
        assert r < 1.0, (name, r)
    print(dtype, "weight gradient, small rows: worst error / tolerance %.3f (%s)" % worst)


_BEHAVIOUR = [(n, t, B, C, H, W) for n, t, B, C, H, W, _, _, _ in D.CAPPED_ROWS] + \
    [(n, t, D.wgrad_row(n)[1], D.wgrad_row(n)[2] * D.VEC[t], D.wgrad_row(n)[3], D.wgrad_row(n)[4])
     for n in D.BEHAVIOUR_SMALL for t in D.DTYPES]


@pytest.mark.parametrize("name,dtype,B,C,H,W", _BEHAVIOUR, ids=[f"{r[0]}-{str(r[1])[6:]}" for r in _BEHAVIOUR])
def test_wgrad_capped_grid_and_behaviour(dev, name, dtype, B, C, H, W):
    """the rows where the grid is capped (a workgroup takes two or three tiles) and two small ones: against float64; a
    NaN-filled workspace changes nothing and holds no NaN afterwards; `into=` adds to what is there; `scale` is applied once;
    two launches give the same bits"""
    from detectron2_centernet_amd import _lib, ops_train
    N = D.VEC[dtype]
    XL, ncol, nstrip, ntiles, G = D.wgrad_geom(B, H, W, C, N)
    x, _, dy = D.make_inputs(600 + B + C + H, dtype, B, H, W, C, with_dy=True)
    ref, mag = D.wgrad_ref(x, dy)
    depth = D.wgrad_depth(B, H, W, C, N)
    xd, dyd = x.to(dtype).to(dev), dy.to(dtype).to(dev)
    del x, dy
    a = ops_train.dwconv3x3_wgrad(xd, dyd, scale=1.0)
    r = D.worst_ratio(a.cpu(), ref, D.wgrad_tol(ref, mag, depth))
    assert torch.equal(a, ops_train.dwconv3x3_wgrad(xd, dyd, scale=1.0))
    nb = _lib.lib().ctdet_dwconv3x3_wgrad_workspace_bytes(B, H, W, C, 0 if dtype == torch.float16 else 1)
    assert nb == G * 9 * C * 4
    ws = torch.full((nb // 4 + 64,), float("nan"), device=dev)
    c = ops_train.dwconv3x3_wgrad(xd, dyd, scale=1.0, workspace=ws)
    assert torch.equal(a, c) and not torch.isnan(ws[:nb // 4]).any() and torch.isnan(ws[nb // 4:]).all()
    scale = 0.375
    s = ops_train.dwconv3x3_wgrad(xd, dyd, scale=scale, workspace=ws)
    r_scale = D.worst_ratio(s.cpu(), scale * ref, D.wgrad_tol(ref, mag, depth, scale))
    base = torch.randn(C, 1, 3, 3, generator=torch.Generator().manual_seed(7))
    into = base.to(dev)
    assert ops_train.dwconv3x3_wgrad(xd, dyd, scale=scale, into=into, workspace=ws) is None
    r_into = D.worst_ratio(into.cpu(), base.double() + scale * ref, D.wgrad_tol(ref, mag, depth, scale, base.double()))
    assert torch.equal(into, base.to(dev) + s)                                       # the add is one f32 add of the same sum
    print(f"{name} {dtype} ntiles / G = {ntiles} / {G}, depth {depth}: error / tolerance {r:.3f}, scaled {r_scale:.3f}, "
          f"accumulated {r_into:.3f}")
    assert r < 1.0 and r_scale < 1.0 and r_into < 1.0


@pytest.mark.parametrize("dtype", D.DTYPES)
def test_wgrad_empty_batch(dev, dtype):
    """B = 0: zeros are written, or with `into=` the slot stays as it is"""
    from detectron2_centernet_amd import ops_train
    C = 8 * D.VEC[dtype]
    x = torch.empty(0, 5, 6, C, dtype=dtype, device=dev)
    got = ops_train.dwconv3x3_wgrad(x, x.clone(), scale=1.0)
    assert tuple(got.shape) == (C, 1, 3, 3) and not got.any()
    base = torch.randn(C, 1, 3, 3, generator=torch.Generator().manual_seed(8)).to(dev)
    into = base.clone()
    assert ops_train.dwconv3x3_wgrad(x, x.clone(), scale=1.0, into=into) is None
    assert torch.equal(into, base)
