"""dec_tile_kernel / dec_final_kernel (ops.decode) and dec_postprocess_kernel (ops.postprocess) against the oracle over the tables
of decode_cases.py: more than one channel chunk, the 4-row tile, a partial last channel vector on the vector-load path, ties across
the chunk seam, K up to 1024, maps that sit in the first radix bin, the clamp floor and the flip merge on chunked, strided maps;
every way a detection is kept or dropped, at 1 .. 1024 rows and four settings of max_det.

Bounds.  Decode: scores, classes and peak indices equal the oracle's in all K slots, zero-score slots included (its stable sort
orders non-peaks by flat index, as the fill path does); boxes atol 1e-4, rtol 1e-6, the bound of the decode tests in
test_hip_ops.py.  Every case is decoded twice into fresh outputs, bit-identical: the candidate list is built with atomics and the
sort has to hide their order.  Postprocess: the counts and the first counts[b] rows equal the reference path's (scaling is one f32
multiply, the clip is exact); rows behind counts[b] are unspecified.  test_decode_host.py proves the tables.

Measured on an MI355X (every test prints its figures before it asserts, run with -s): all 28 decode cases equal the oracle in every
slot, boxes included (error 0).  Postprocess before the NaN rule in dec_postprocess_kernel: the rows with a NaN x1 or y1 and an
otherwise valid extent were kept with that coordinate set to 0 (3 to 73 rows too many in the mixed image of every case with
K >= 63); with it all 24 cases are equal.  What bites: the chunk offset left out of the tile pass's flat index fails all 15 cases
with more than one chunk; `>=` for `>` at the score threshold fails the 18 cases in which max_det lets a threshold-tie row through; a first
radix level that puts every key into one bin changes nothing, as it must.
"""
import pytest
import torch

import decode_cases as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    import detectron2_centernet_amd.ops as ops

    return ops


def _device_maps(case, dev):
    """the maps as the heads leave them: heat NHWC as the slice [..., :C] of a buffer of `stride` channels whose other channels
    hold 0.5 (above most of the map: they must not matter), wh and reg as slices of one 4-channel buffer"""
    heat, wh, reg = T.decode_inputs(case)
    n = heat.shape[0]
    buf = torch.full((n, case.H, case.W, case.stride), 0.5)
    buf[..., :case.C] = T.nhwc(heat)
    hm = buf.to(dev)[..., :case.C]
    assert hm.stride(2) == case.stride and (case.stride == case.C) == hm.is_contiguous()
    whreg = torch.cat([T.nhwc(wh), T.nhwc(reg)], dim=3).to(dev)
    return hm, whreg[..., 0:2], whreg[..., 2:4]


@pytest.mark.parametrize("case", T.DECODE_CASES, ids=T.decode_id)
def test_decode(ops, dev, case):
    rb, rs, rc, ri = T.decode_reference(case)
    hm, wh, reg = _device_maps(case, dev)
    runs = []
    for _ in range(2):
        out = ops.decode(hm, wh, reg, case.K, 4.0, check_status=True, heat_floor=case.floor, flip=case.flip)
        runs.append([t.cpu() for t in out])
    b, s, c, i = runs[0]
    assert s.shape == rs.shape and c.shape == rc.shape and b.shape == rb.shape
    wrong = (s != rs) | (c != rc) | (i.long() != ri)
    print(f"decode {T.decode_id(case)}: {int(wrong.sum())} of {wrong.numel()} slots differ from the oracle, "
          f"box err {(b - rb).abs().max().item():.2e}")
    assert torch.equal(s, rs), "scores differ"
    assert torch.equal(c, rc), "classes differ"
    assert torch.equal(i.long(), ri), "peak indices differ"
    assert torch.allclose(b, rb, atol=1e-4, rtol=1e-6), "boxes differ"
    for name, x, y in zip(("boxes", "scores", "classes", "inds"), runs[0], runs[1]):
        assert torch.equal(x, y), f"{name}: two runs on the same maps differ"


@pytest.mark.parametrize("case", T.POST_CASES, ids=T.post_id)
def test_postprocess(ops, dev, case):
    inp, ref = T.post_inputs(case), T.post_reference(case)
    ob, os_, oc, counts = ops.postprocess(inp["boxes"].to(dev), inp["scores"].to(dev), inp["classes"].to(dev), case.max_det,
                                          T.POST_THRESH, inp["img_params"].to(dev))
    ob, os_, oc, counts = ob.cpu(), os_.cpu(), oc.cpu(), counts.cpu().tolist()
    print(f"postprocess {T.post_id(case)}: counts {counts}, reference {[len(r[1]) for r in ref]}")
    for b, (rb, rs, rc) in enumerate(ref):
        n = len(rs)
        got = oc[b, :max(0, min(counts[b], case.K))].tolist()
        assert counts[b] == n, (f"image {b}: {counts[b]} rows kept, the reference keeps {n}; rows only the kernel keeps "
                                f"{sorted(set(got) - set(rc.tolist()))}, only the reference {sorted(set(rc.tolist()) - set(got))}")
        assert torch.equal(oc[b, :n], rc), f"image {b}: rows or their order differ"
        assert torch.equal(os_[b, :n], rs), f"image {b}: scores differ"
        assert torch.equal(ob[b, :n], rb), f"image {b}: boxes differ"
