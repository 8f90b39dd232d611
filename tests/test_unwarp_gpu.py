"""The box unwarp on the GPU (csrc/unwarp.hip through ops.postprocess_affine) against data.warp.unwarp_boxes_reference, bit for
bit, over tests/unwarp_cases.py; against ops.postprocess where the translation is zero; then CenterNet's fix_res / keep_res
test input end to end (INPUT.AFFINE.TEST_MODE): host-mapped and raw affine records against an exact oracle --
the same warped bytes as plain records at scale 1 through the existing kernel, their rows through the numpy oracle -- on the
captured engine, under the flip test and for keep_res."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import decode_cases as DC
import unwarp_cases as UC

pytestmark = pytest.mark.gpu
SENTINEL_F, SENTINEL_I = -12345.5, -77
MIN_ROWS = 10      # compared rows per image an end-to-end comparison needs to mean something


@pytest.fixture(scope="module")
def ops(dev):
    import detectron2_centernet_amd.ops as ops
    return ops


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ kernel against the oracle
@pytest.mark.parametrize("case", UC.CASES, ids=UC.CASE_IDS)
def test_kernel_equals_the_oracle_bit_for_bit(ops, dev, case):
    inp, ref = UC.inputs(case), UC.reference(case)
    B, K = case.B, case.K
    boxes, scores, classes, params = (torch.from_numpy(np.array(inp[k])).to(dev) for k in ("boxes", "scores", "classes", "params"))
    out = (torch.full((B, K, 4), SENTINEL_F, dtype=torch.float32, device=dev), torch.full((B, K), SENTINEL_F, dtype=torch.float32, device=dev),
           torch.full((B, K), SENTINEL_I, dtype=torch.int32, device=dev), torch.full((B,), SENTINEL_I, dtype=torch.int32, device=dev))
    got = ops.postprocess_affine(boxes, scores, classes, case.max_det, UC.THRESH, params, out=out)
    assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
    ob, os_, oc, counts = (t.cpu().numpy() for t in out)
    print(f"postprocess_affine {case.name}: counts {counts.tolist()}, oracle {[len(r[1]) for r in ref]}")
    assert counts.tolist() == [len(r[1]) for r in ref]
    for b in range(B):
        n = counts[b]
        rb, rs, rc = ref[b]
        assert np.array_equal(oc[b, :n], rc), (case.name, b)
        assert np.array_equal(_bits(os_[b, :n]), _bits(rs)) and np.array_equal(_bits(ob[b, :n]), _bits(rb)), (case.name, b)
        # nothing behind the counts[b] rows the oracle defines
        assert (ob[b, n:] == SENTINEL_F).all() and (os_[b, n:] == SENTINEL_F).all() and (oc[b, n:] == SENTINEL_I).all(), (case.name, b)
    # fresh outputs give the same rows
    fb, fs, fc, fcounts = ops.postprocess_affine(boxes, scores, classes, case.max_det, UC.THRESH, params)
    assert fcounts.cpu().numpy().tolist() == counts.tolist()
    for b in range(B):
        assert np.array_equal(_bits(fb[b, :counts[b]].cpu().numpy()), _bits(ref[b][0]))


def test_the_table_would_catch_a_fused_multiply_add(ops, dev):
    """the kernel's rows differ from what one rounding would give on the rows the table counts (>= 8, asserted at its import)"""
    case = next(c for c in UC.CASES if c.name == "contraction")
    inp, ref = UC.inputs(case), UC.reference(case)
    rows = UC.contraction_rows(case)
    assert sum(len(r) for r in rows) >= 8
    boxes, scores, classes, params = (torch.from_numpy(np.array(inp[k])).to(dev) for k in ("boxes", "scores", "classes", "params"))
    ob, _, oc, counts = ops.postprocess_affine(boxes, scores, classes, case.max_det, UC.THRESH, params)
    for b in range(case.B):
        p = inp["params"][b]
        n = int(counts[b])
        kept = oc[b, :n].cpu().numpy()
        _, fused = UC.two_roundings(inp["boxes"][b][kept], p[[0, 1, 0, 1]], p[[2, 3, 2, 3]])
        got = ob[b, :n].cpu().numpy()
        differing = [int(k) for k, g, f in zip(kept, got, fused) if not np.array_equal(g, f)]
        assert set(rows[b]) <= set(differing), (b, rows[b], differing)


@pytest.mark.parametrize("case", DC.POST_CASES, ids=DC.post_id)
def test_zero_translation_equals_postprocess(ops, dev, case):
    inp = DC.post_inputs(case)
    boxes, scores, classes, p4 = (inp[k].to(dev) for k in ("boxes", "scores", "classes", "img_params"))
    p6 = torch.zeros(DC.POST_B, 6, dtype=torch.float32)
    p6[:, :2], p6[:, 4:] = inp["img_params"][:, :2], inp["img_params"][:, 2:]
    wb, ws, wc, wcounts = ops.postprocess(boxes, scores, classes, case.max_det, DC.POST_THRESH, p4)
    gb, gs, gc, gcounts = ops.postprocess_affine(boxes, scores, classes, case.max_det, DC.POST_THRESH, p6.to(dev))
    assert torch.equal(gcounts, wcounts)
    ref = DC.post_reference(case)
    assert gcounts.tolist() == [len(r[1]) for r in ref]
    for b, n in enumerate(gcounts.tolist()):
        assert torch.equal(gb[b, :n], wb[b, :n]) and torch.equal(gs[b, :n], ws[b, :n]) and torch.equal(gc[b, :n], wc[b, :n]), b


def test_refusals(ops, dev):
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)      # noqa: E731
    with pytest.raises(AssertionError, match=r"\[2, 6\]"):
        ops.postprocess_affine(z(2, 3, 4), z(2, 3), z(2, 3, dt=torch.int32), 3, 0.1, z(2, 4))
    with pytest.raises(AssertionError):
        ops.postprocess_affine(z(2, 3, 4), z(2, 3), z(2, 3), 3, 0.1, z(2, 6))      # classes are int32


# ------------------------------------------------------------------------------------------------------------ end to end
SOURCES = {"a": (60, 80), "b": (70, 50), "c": (40, 90), "d": (64, 64), "e": (50, 70)}      # (h, w)
_NETS = {}


@pytest.fixture(scope="module")
def net(tmp_path_factory, dev):
    """get(precision) -> (model, cfg): built once per precision, score threshold 0, a positive wh bias (random weights leave
    the size map near 0: every box would be empty)"""
    from test_model_gpu import make_model

    def get(precision):
        if precision not in _NETS:
            model, cfg = make_model(tmp_path_factory.mktemp("unwarp_" + precision), precision, seed=4)
            model.score_threshold = 0.0
            model.wh[-1].bias.data.fill_(3.0)
            _NETS[precision] = (model, cfg)
        return _NETS[precision]
    yield get
    _NETS.clear()


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = tmp_path_factory.mktemp("unwarp_images")
    rng = np.random.RandomState(11)
    recs = {}
    for name, (h, w) in SOURCES.items():
        path = os.path.join(str(root), f"{name}.png")
        Image.fromarray(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(path)
        recs[name] = {"file_name": path, "image_id": len(recs), "height": h, "width": w}
    return recs


def _mapped(cfg, recs, mode, raw, out=(64, 64)):
    from detectron2_centernet_amd.data import TrafficLightDatasetMapper
    c = cfg.clone()
    c.INPUT.AFFINE.TEST_MODE, c.INPUT.AFFINE.OUTPUT_SIZE, c.INPUT.DEVICE_RESIZE = mode, out, raw
    mapper = TrafficLightDatasetMapper(c, is_train=False)
    return [mapper(r) for r in recs]


def _oracle(run, host_records):
    """the same warped bytes as plain records at the network's size (scale 1, the existing kernel), their rows through the numpy
    oracle.  Exact because the unwarp is monotone in f32 and the content rectangle lies inside the network frame -- asserted here
    per input -- so that clipping to the network frame first cannot change the result."""
    from detectron2_centernet_amd.data import warp as W
    plain = [{"image": r["image"], "height": r["image"].shape[1], "width": r["image"].shape[2]} for r in host_records]
    res = run(plain)
    out = []
    for r, rec in zip(res, host_records):
        inst = r["instances"]
        H, Wn = rec["image"].shape[1:]
        assert inst.image_size == (H, Wn)
        M, flip = W.unpack_warp(rec["warp"])
        p = W.unwarp_params(M, (rec["height"], rec["width"]))
        sx, sy, tx, ty, ow, oh = p
        assert not flip and tx <= 0 and ty <= 0 and np.float32(sx * np.float32(Wn)) + tx >= ow and np.float32(sy * np.float32(H)) + ty >= oh
        n = len(inst)
        out.append(W.unwarp_boxes_reference(inst.pred_boxes.tensor.cpu().numpy(), inst.scores.cpu().numpy(),
                                            inst.pred_classes.cpu().numpy(), n, 0.0, p))
    return out


def _assert_equals_oracle(results, records, oracle):
    assert len(results) == len(records) == len(oracle)
    for r, rec, (wb, ws, wc) in zip(results, records, oracle):
        inst = r["instances"]
        assert inst.image_size == (rec["height"], rec["width"])
        print(f"source {rec['width']}x{rec['height']}: {len(inst)} rows, oracle {len(ws)}")
        assert len(ws) >= MIN_ROWS, f"only {len(ws)} rows to compare"
        assert len(inst) == len(ws)
        assert np.array_equal(inst.pred_classes.cpu().numpy(), wc)
        assert np.array_equal(_bits(inst.scores.cpu().numpy()), _bits(ws))
        assert np.array_equal(_bits(inst.pred_boxes.tensor.cpu().numpy()), _bits(wb))
        assert (wb[:, [0, 2]] <= rec["width"]).all() and (wb[:, [1, 3]] <= rec["height"]).all()


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        ix, iy = x["instances"], y["instances"]
        assert ix.image_size == iy.image_size and len(ix) == len(iy)
        assert torch.equal(ix.pred_classes, iy.pred_classes) and torch.equal(ix.scores, iy.scores)
        assert torch.equal(ix.pred_boxes.tensor, iy.pred_boxes.tensor)


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_fix_res_end_to_end(net, dataset, precision):
    model, cfg = net(precision)
    recs = [dataset["a"], dataset["b"]]      # 80 x 60 and 50 x 70 (w x h) in one batch
    host, raw = _mapped(cfg, recs, "fix_res", False), _mapped(cfg, recs, "fix_res", True)
    assert all(tuple(r["image"].shape) == (3, 64, 64) for r in host) and all(tuple(r["resize_hw"]) == (64, 64) for r in raw)
    with torch.no_grad():
        got_host, got_raw = model(host), model(raw)
        oracle = _oracle(model, host)
    _same(got_host, got_raw)
    _assert_equals_oracle(got_host, host, oracle)
    _same(model.forward_async(raw).result(), got_raw)
    # the unwarp moved the boxes: image "a" (ty = -10, a = 1.25) differs from its rows in the network's frame
    plain = model([{"image": host[0]["image"], "height": 64, "width": 64}])[0]["instances"]
    assert not torch.equal(plain.pred_boxes.tensor, got_host[0]["instances"].pred_boxes.tensor)
    with pytest.raises(KeyError, match=r"warped \(INPUT\.AFFINE\.TEST_MODE\) or resized as a whole"):
        model([raw[0], {k: v for k, v in raw[1].items() if k != "warp"}])
    with pytest.raises(KeyError, match=r"warped \(INPUT\.AFFINE\.TEST_MODE\) or resized as a whole"):
        model([host[0], {k: v for k, v in host[1].items() if k != "warp"}])


def test_fix_res_takes_one_captured_engine(net, dataset, monkeypatch, ops):
    model, cfg = net("f16x3")
    model._engines = {}

    def ragged(*a, **k):
        raise AssertionError("_forward_eval_ragged entered")
    monkeypatch.setattr(model, "_forward_eval_ragged", ragged)
    first = _mapped(cfg, [dataset["a"], dataset["b"]], "fix_res", True)
    with torch.no_grad():
        res1 = model(first)
    assert len(model._engines) == 1
    (key, eng), = model._engines.items()
    assert key[-1] == "affine" and eng.affine and tuple(eng.img_params.shape) == (2, 6)
    assert eng.graph is not None or ops.RANGE_CHECK
    second = _mapped(cfg, [dataset["c"], dataset["d"]], "fix_res", True)      # other source sizes: the same engine, new parameters
    with torch.no_grad():
        res2 = model(second)
        assert len(model._engines) == 1 and next(iter(model._engines.values())) is eng
        assert [r["instances"].image_size for r in res2] == [SOURCES["c"], SOURCES["d"]]
        _same(model(first), res1)      # ... and back: the parameter buffer follows the warps
        _same(model(_mapped(cfg, [dataset["c"], dataset["d"]], "fix_res", False)), res2)      # host-mapped records: the same engine
        assert len(model._engines) == 1
        # a plain batch of the same shape builds its own engine, with the [B, 4] buffer and the existing kernel
        model([{"image": r["image"]} for r in _mapped(cfg, [dataset["a"], dataset["b"]], "fix_res", False)])
    assert len(model._engines) == 2
    plain = [e for e in model._engines.values() if e is not eng][0]
    assert not plain.affine and tuple(plain.img_params.shape) == (2, 4) and plain.key + ("affine",) == eng.key


def test_flip_test_on_affine_records(net, dataset):
    from detectron2_centernet_amd.modeling import CenterNetWithTTA
    model, cfg = net("f16x3")
    c = cfg.clone()
    c.TEST.AUG.ENABLED, c.TEST.AUG.MIN_SIZES, c.TEST.AUG.FLIP = True, (), True
    c.INPUT.AFFINE.TEST_MODE, c.INPUT.AFFINE.OUTPUT_SIZE = "fix_res", (64, 64)
    tta = CenterNetWithTTA(c, model)
    recs = [dataset["a"], dataset["b"]]
    host, raw = _mapped(cfg, recs, "fix_res", False), _mapped(cfg, recs, "fix_res", True)
    plain_cfg = c.clone()
    plain_cfg.INPUT.AFFINE.TEST_MODE = ""
    with torch.no_grad():
        got = tta(raw)
        _same(tta(host), got)
        oracle = _oracle(CenterNetWithTTA(plain_cfg, model), host)      # the plain flip path on the same warped bytes
        unflipped = model(raw)
    _assert_equals_oracle(got, host, oracle)
    assert not torch.equal(got[0]["instances"].scores, unflipped[0]["instances"].scores)      # the flip test changed the result
    assert any(k[-2:] == ("flip", "affine") for k in model._engines)


def test_keep_res_end_to_end(net, dataset):
    model, cfg = net("f16x3")
    host, raw = _mapped(cfg, [dataset["e"]], "keep_res", False), _mapped(cfg, [dataset["e"]], "keep_res", True)
    assert tuple(host[0]["image"].shape) == (3, 64, 96) and tuple(raw[0]["resize_hw"]) == (64, 96)      # a 70 x 50 source
    with torch.no_grad():
        got = model(host)
        _same(model(raw), got)
        _assert_equals_oracle(got, host, _oracle(model, host))
        # two sizes in one batch (64 x 96 and 96 x 64): one warp launch per size, then the ragged path
        recs = [dataset["e"], dataset["b"]]
        host2, raw2 = _mapped(cfg, recs, "keep_res", False), _mapped(cfg, recs, "keep_res", True)
        assert [tuple(r["resize_hw"]) for r in raw2] == [(64, 96), (96, 64)]
        got2 = model(raw2)
        _same(model(host2), got2)
        _assert_equals_oracle(got2, host2, _oracle(model, host2))
