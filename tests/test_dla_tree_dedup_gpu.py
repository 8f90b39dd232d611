"""Tree.hip_forward without the work nothing reads (ops.TREE_DEDUP): a DLA tree of more than one level (level3 and level4 of
DLA-34) neither runs its own 1x1 projection, which its tree1 replaces by its own, nor lets tree1 pool the same input again.
The six level outputs must be bit-equal with the switch on and off, and the captured eval step loses exactly the two
projections and the two pools."""
import pytest
import torch

from test_model_gpu import images, make_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    import detectron2_centernet_amd.ops as ops

    return ops


def _kernel_nodes(model, imgs):
    model._engines = {}
    model.infer_batch_tensor(imgs)
    eng = list(model._engines.values())[-1]
    assert eng.graph is not None and set(eng.graph_nodes) <= {"kernel", "empty"}, eng.graph_nodes
    return eng.graph_nodes["kernel"], [t.clone() for t in eng.dec]


@pytest.mark.parametrize("precision", ["f16x3", "f16"])
def test_levels_equal_and_four_launches_fewer(tmp_path, dev, ops, monkeypatch, precision):
    model, cfg = make_model(tmp_path, precision, seed=4)
    model.score_threshold = 0.0
    base = model.backbone.base
    assert [getattr(base, f"level{i}").levels for i in range(2, 6)] == [1, 2, 2, 1]
    imgs = images(2, 64, 128, seed=9).to(dev)
    x = ops.preprocess(imgs, cfg.MODEL.PIXEL_MEAN, cfg.MODEL.PIXEL_STD, 64, 128, out_dtype=model._ctx.dtype)

    calls = {"pool": 0}
    real_pool = ops.maxpool2x2
    monkeypatch.setattr(ops, "maxpool2x2", lambda *a, **k: (calls.__setitem__("pool", calls["pool"] + 1), real_pool(*a, **k))[1])
    monkeypatch.setattr(ops, "TREE_DEDUP", False)
    y_off = base.hip_forward(x, model._ctx)
    pools_off, calls["pool"] = calls["pool"], 0
    n_off, dec_off = _kernel_nodes(model, imgs)
    monkeypatch.setattr(ops, "TREE_DEDUP", True)
    calls["pool"] = 0
    y_on = base.hip_forward(x, model._ctx)
    pools_on = calls["pool"]
    n_on, dec_on = _kernel_nodes(model, imgs)

    assert len(y_on) == len(y_off) == 6
    for lvl, (a, b) in enumerate(zip(y_on, y_off)):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), lvl
    assert (pools_off, pools_on) == (6, 4)           # level2 .. level5, twice in level3 and level4
    assert n_on == n_off - 4, (n_off, n_on)          # two pools and two projections
    for a, b in zip(dec_on, dec_off):
        assert torch.equal(a, b)
