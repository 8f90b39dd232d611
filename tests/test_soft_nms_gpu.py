"""Multi-scale test augmentation's soft-NMS merge on the device: ops.soft_nms_merge on every case of
tests/soft_nms_cases.py against the float64 restatement -- boxes and classes bit for bit, counts and order equal, every score
within its (decays + 1) * c * 2^-24 bound -- and the wrapper end to end on the small DLA-34 of the TTA tests: what the
multi-size wrapper returns is, bit for bit, the merge of what single-size wrappers return at the same sizes."""
import numpy as np
import pytest
import torch

import soft_nms_cases as S

pytestmark = pytest.mark.gpu

PRECISION = "f16"


@pytest.fixture(scope="module")
def ops():
    import detectron2_centernet_amd.ops as ops

    return ops


def _dev_passes(case, dev):
    return [tuple(torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in p) for p in case.passes]


# ------------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("case", S.CASES, ids=repr)
def test_merge_against_the_restatement(ops, dev, case):
    boxes, scores, classes, counts = ops.soft_nms_merge(_dev_passes(case, dev), case.num_classes, case.sigma, case.min_score,
                                                        case.max_det)
    B = len(case.passes[0][3])
    assert tuple(boxes.shape) == (B, case.max_det, 4) and tuple(scores.shape) == (B, case.max_det)
    assert classes.dtype == torch.int32 and counts.dtype == torch.int32 and tuple(counts.shape) == (B,)
    boxes, scores, classes, counts = boxes.cpu().numpy(), scores.cpu().numpy(), classes.cpu().numpy(), counts.cpu().numpy()
    worst = 0.0
    for b, ref in enumerate(case.reference()):
        n = ref["count"]
        assert int(counts[b]) == n, (case, b)
        if n <= 0:
            continue
        # same candidates in the same order: boxes and classes are copies
        assert np.array_equal(boxes[b, :n].view(np.uint32), ref["boxes"].view(np.uint32)), (case, b)
        assert np.array_equal(classes[b, :n], ref["classes"]), (case, b)
        rel = np.abs(scores[b, :n].astype(np.float64) - ref["scores"]) / np.abs(ref["scores"])
        worst = max(worst, float((rel / S.bound(ref["decays"], case.sigma)).max()))
        print(f"{case} image {b}: {n} kept, max score error {rel.max() / S.U:.2f} x 2^-24, "
              f"{(rel / S.U / np.maximum(ref['decays'], 1)).max():.2f} per decay, worst share of the bound {worst:.3f}")
        assert (rel <= S.bound(ref["decays"], case.sigma)).all(), (case, b)
        undecayed = ref["decays"] == 0
        assert np.array_equal(scores[b, :n][undecayed], ref["scores"][undecayed].astype(np.float32)), "undecayed scores are copies"
        assert (np.diff(scores[b, :n]) <= 0).all()


@pytest.mark.parametrize("name,cands,want", S.KNOWN, ids=[k[0] for k in S.KNOWN])
def test_kernel_gives_the_hand_derived_answers(ops, dev, name, cands, want):
    """the kernel against the hand-derived values themselves, not through the restatement: class 1 of 3, one pass"""
    boxes = torch.tensor([[c[0] for c in cands]], dtype=torch.float32, device=dev)
    scores = torch.tensor([[c[1] for c in cands]], dtype=torch.float32, device=dev)
    classes = torch.ones(1, len(cands), dtype=torch.int32, device=dev)
    counts = torch.tensor([len(cands)], dtype=torch.int32, device=dev)
    ob, os_, oc, n = ops.soft_nms_merge([(boxes, scores, classes, counts)], 3, 0.5, 0.001, 10)
    by_score = sorted(want, key=lambda w: -w[1])          # the final order; the known answers hold no ties
    assert int(n[0]) == len(want)
    assert torch.equal(ob[0, :len(want)], boxes[0, [w[0] for w in by_score]]) and oc[0, :len(want)].tolist() == [1] * len(want)
    got = os_[0, :len(want)].cpu().numpy().astype(np.float64)
    order, _, dec = S.class_soft_nms(boxes[0].cpu().numpy(), scores[0].cpu().numpy(), 0.5, 0.001)
    received = dict(zip(order.tolist(), dec.tolist()))      # only the number of decays (the bound's factor) comes from here
    for k, (i, s) in enumerate(by_score):
        value = float(scores[0, i]) * (s / cands[i][1])    # the hand-derived weight times the f32 input score
        decays = received[i]
        assert abs(got[k] - value) <= S.bound(decays, 0.5) * value, (name, k, got[k], value)
        if decays == 0:
            assert got[k] == float(scores[0, i])


def test_two_runs_are_bit_identical(ops, dev):
    for case in S.CASES:
        passes = _dev_passes(case, dev)
        a = ops.soft_nms_merge(passes, case.num_classes, case.sigma, case.min_score, case.max_det)
        b = ops.soft_nms_merge(passes, case.num_classes, case.sigma, case.min_score, case.max_det)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), case       # the whole tensors: the tail behind the count is zero
        n = int(a[3].clamp(min=0).max().item())
        assert not a[0][:, n:].any() and not a[1][:, n:].any() and not a[2][:, n:].any()


def test_refusals(ops, dev):
    p = (torch.zeros(1, 129, 4, device=dev), torch.zeros(1, 129, device=dev), torch.zeros(1, 129, dtype=torch.int32, device=dev),
         torch.zeros(1, dtype=torch.int32, device=dev))
    with pytest.raises(RuntimeError, match="17 passes"):
        ops.soft_nms_merge([p] * 17, 3, 0.5, 0.001, 10)
    with pytest.raises(RuntimeError, match="2064 candidates"):
        ops.soft_nms_merge([p] * 16, 3, 0.5, 0.001, 10)
    with pytest.raises(RuntimeError, match="max_det=0"):
        ops.soft_nms_merge([p], 3, 0.5, 0.001, 0)
    with pytest.raises(RuntimeError, match="sigma=0"):
        ops.soft_nms_merge([p], 3, 0.0, 0.001, 10)
    with pytest.raises(NotImplementedError):
        ops.soft_nms_merge([tuple(t.cpu() for t in p)], 3, 0.5, 0.001, 10)


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def net(tmp_path_factory, dev):
    from test_model_gpu import make_model
    model, cfg = make_model(tmp_path_factory.mktemp("soft_nms_net"), PRECISION, seed=4)
    model.score_threshold = 0.0
    model.wh[-1].bias.data.fill_(3.0)          # boxes of non-degenerate size
    return model, cfg


def _cfg(cfg, min_sizes, flip, soft_nms):
    cfg = cfg.clone()
    cfg.TEST.AUG.ENABLED, cfg.TEST.AUG.MIN_SIZES, cfg.TEST.AUG.FLIP = True, tuple(min_sizes), flip
    cfg.TEST.AUG.MAX_SIZE = 1333
    cfg.TEST.SOFT_NMS.ENABLED = soft_nms
    return cfg


def _raw(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3), dtype=np.uint8)


def _records(kind, raws):
    if kind == "image_raw":
        return [{"image_raw": r} for r in raws]
    return [{"image": torch.from_numpy(np.ascontiguousarray(r.transpose(2, 0, 1)))} for r in raws]


def _as_pass(results, dev):
    """a single-size wrapper's Instances as one padded pass"""
    insts = [r["instances"] for r in results]
    B, K = len(insts), max(len(i) for i in insts)
    boxes = torch.full((B, K, 4), 7.0, device=dev)
    scores = torch.full((B, K), 0.99, device=dev)
    classes = torch.zeros(B, K, dtype=torch.int32, device=dev)
    for b, i in enumerate(insts):
        n = len(i)
        boxes[b, :n], scores[b, :n], classes[b, :n] = i.pred_boxes.tensor, i.scores, i.pred_classes
    return boxes, scores, classes, torch.tensor([len(i) for i in insts], dtype=torch.int32, device=dev)


def _equal_to_merge(results, merged, sizes):
    boxes, scores, classes, counts = merged
    assert len(results) == len(counts)
    for b, r in enumerate(results):
        i, n = r["instances"], int(counts[b])
        assert i.image_size == sizes[b] and len(i) == n > 0
        assert torch.equal(i.pred_boxes.tensor, boxes[b, :n]) and torch.equal(i.scores, scores[b, :n])
        assert torch.equal(i.pred_classes, classes[b, :n])


@pytest.mark.parametrize("kind", ["image", "image_raw"])
@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
def test_multi_size_wrapper_is_the_merge_of_the_single_size_wrappers(net, ops, dev, kind, flip):
    from detectron2_centernet_amd.modeling import CenterNetWithTTA
    model, cfg = net
    sizes = (64, 96)
    raws = [_raw(48, 72, 1), _raw(48, 72, 2)]                  # -> 64 x 96 and 96 x 144
    recs = _records(kind, raws)
    singles = [CenterNetWithTTA(_cfg(cfg, (s,), flip, False), model)(recs) for s in sizes]
    assert all(r["instances"].image_size == (48, 72) for one in singles for r in one)
    assert not torch.equal(singles[0][0]["instances"].pred_boxes.tensor, singles[1][0]["instances"].pred_boxes.tensor)
    want = ops.soft_nms_merge([_as_pass(one, dev) for one in singles], model.num_classes, 0.5, 0.001, 100)
    tta = CenterNetWithTTA(_cfg(cfg, sizes, flip, True), model)
    out = tta(recs)
    _equal_to_merge(out, want, [(48, 72)] * 2)
    _equal_to_merge(tta.forward_async(recs).result(), want, [(48, 72)] * 2)
    # the merge did something: the passes hold 100 candidates each, duplicates of one another, and scores were decayed
    first = singles[0][0]["instances"]
    assert len(first) > 50 and not torch.equal(out[0]["instances"].scores, first.scores)
    # the order of TEST.AUG.MIN_SIZES is the order of the candidates
    rev = ops.soft_nms_merge([_as_pass(one, dev) for one in singles[::-1]], model.num_classes, 0.5, 0.001, 100)
    _equal_to_merge(CenterNetWithTTA(_cfg(cfg, sizes[::-1], flip, True), model)(recs), rev, [(48, 72)] * 2)


def test_one_size_with_the_switch_is_the_merge_of_that_pass(net, ops, dev):
    from detectron2_centernet_amd.modeling import CenterNetWithTTA
    model, cfg = net
    recs = _records("image", [_raw(48, 72, 3), _raw(48, 72, 4)])
    for sizes in ((64,), ()):
        single = CenterNetWithTTA(_cfg(cfg, sizes, True, False), model)(recs)
        want = ops.soft_nms_merge([_as_pass(single, dev)], model.num_classes, 0.5, 0.001, 100)
        tta = CenterNetWithTTA(_cfg(cfg, sizes, True, True), model)
        _equal_to_merge(tta(recs), want, [(48, 72)] * 2)
        _equal_to_merge(tta.forward_async(recs).result(), want, [(48, 72)] * 2)
    # SIGMA, MIN_SCORE and DETECTIONS_PER_IMAGE reach the kernel
    c = _cfg(cfg, (64,), True, True)
    c.TEST.SOFT_NMS.SIGMA, c.TEST.SOFT_NMS.MIN_SCORE, c.TEST.DETECTIONS_PER_IMAGE = 0.25, 0.01, 17
    single = CenterNetWithTTA(_cfg(cfg, (64,), True, False), model)(recs)
    want = ops.soft_nms_merge([_as_pass(single, dev)], model.num_classes, 0.25, 0.01, 17)
    out = CenterNetWithTTA(c, model)(recs)
    _equal_to_merge(out, want, [(48, 72)] * 2)
    assert len(out[0]["instances"]) == 17


@pytest.mark.parametrize("kind", ["image", "image_raw"])
def test_ragged_batch_takes_the_packed_route(net, ops, dev, kind):
    """(raw records of two sizes: the one pinned upload holds images of different lengths)"""
    from detectron2_centernet_amd.modeling import CenterNetWithTTA
    model, cfg = net
    recs = _records(kind, [_raw(48, 72, 5), _raw(40, 40, 6)])
    sizes = (64, 96)
    singles = [CenterNetWithTTA(_cfg(cfg, (s,), False, False), model)(recs) for s in sizes]
    want = ops.soft_nms_merge([_as_pass(one, dev) for one in singles], model.num_classes, 0.5, 0.001, 100)
    tta = CenterNetWithTTA(_cfg(cfg, sizes, False, True), model)
    _equal_to_merge(tta(recs), want, [(48, 72), (40, 40)])
    _equal_to_merge(tta.forward_async(recs).result(), want, [(48, 72), (40, 40)])


def test_a_non_finite_pass_raises(net, dev):
    from detectron2_centernet_amd.modeling import CenterNetWithTTA
    model, cfg = net
    recs = _records("image", [_raw(48, 72, 7), _raw(48, 72, 8)])
    tta = CenterNetWithTTA(_cfg(cfg, (64, 96), True, True), model)
    assert len(tta(recs)) == 2
    keep = model.wh[2].weight[0, 0, 0, 0].item()
    try:
        with torch.no_grad():
            model.wh[2].weight[0, 0, 0, 0] = float("inf")
        model._engines = {}                                  # (weights changed behind the engines' back)
        with pytest.raises(FloatingPointError, match="not finite"):
            tta(recs)
        with pytest.raises(FloatingPointError, match="not finite"):
            tta.forward_async(recs).result()
    finally:
        with torch.no_grad():
            model.wh[2].weight[0, 0, 0, 0] = keep
        model._engines = {}
