"""The device colour jitter on the GPU (csrc/jitter.hip through ops.colour_jitter_u8) against what the host mapper produces
today -- the chain of BlendTransforms -- byte for byte: zero mismatches, no tolerance, on every case of tests/jitter_cases.py,
on a contiguous CHW tensor and on a window of a sentinel-filled batch; the 64-bit byte sum; one batched launch against the
per-image launches.  Then end to end: raw training records (INPUT.DEVICE_AUGMENT) through CenterNet give the image bytes, the
targets and the losses of host-mapped records made from the same seed, and SimpleTrainer.run_step trains on them.

Losses are compared with torch.equal when two runs of the host path are themselves bit-identical at that shape (checked
first, printed); otherwise with the bound test_train_gpu.py uses between two paths of the same step (four times the measured
run-to-run noise plus 1e-5, relative)."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import jitter_cases as JC

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
PRECISION = "f16"


@pytest.fixture(scope="module")
def cases():
    """(id, image HWC, spec, the host chain's result HWC), computed once; read only"""
    out = []
    for cid, img, params in JC.all_cases():
        ref = JC.host_chain(img, params)
        img.setflags(write=False)
        ref.setflags(write=False)
        out.append((cid, img, JC.spec_of(params), ref))
    return out


@pytest.fixture(scope="module")
def ops(dev):
    import detectron2_centernet_amd.ops as ops
    return ops


def _chw(img, dev):
    return torch.from_numpy(np.array(img.transpose(2, 0, 1), order="C")).to(dev)      # a writable copy


def _mismatches(got_chw, ref_hwc):
    got = got_chw.permute(1, 2, 0).cpu().numpy()
    assert got.shape == ref_hwc.shape, (got.shape, ref_hwc.shape)
    return int((got != ref_hwc).sum())


def _form_chw(ops, dev, img, spec, ref):
    t = _chw(img, dev)
    out = ops.colour_jitter_u8([t], [torch.from_numpy(spec)])[0]
    assert out.data_ptr() == t.data_ptr()                        # in place
    return _mismatches(t, ref)


def _form_window(ops, dev, img, spec, ref):
    """the image as a window of a sentinel-filled batch, planar (a staging batch) and interleaved: the window holds the host's
    bytes, every byte outside it stays the sentinel"""
    bad = 0
    h, w = img.shape[:2]
    for planar in (True, False):
        if planar:
            buf = torch.full((2, 3, h + 5, w + 7), SENTINEL, dtype=torch.uint8, device=dev)
            win = buf[1, :, 2:2 + h, 3:3 + w]
        else:
            buf = torch.full((h + 5, w + 7, 3), SENTINEL, dtype=torch.uint8, device=dev)
            win = buf[2:2 + h, 3:3 + w].permute(2, 0, 1)
        win.copy_(_chw(img, dev))
        ops.colour_jitter_u8([win], [spec])
        bad += _mismatches(win, ref)
        win.fill_(SENTINEL)
        bad += int((buf != SENTINEL).sum().item())
    return bad


FORMS = {"chw": _form_chw, "window": _form_window}


@pytest.mark.parametrize("form", list(FORMS))
def test_kernel_equals_the_host_chain_byte_for_byte(ops, dev, cases, form):
    bad = {}
    for cid, img, spec, ref in cases:
        n = FORMS[form](ops, dev, img, spec, ref)
        if n:
            bad[cid] = n
    assert len(cases) == 240
    assert not bad, f"{form}: mismatching bytes per case {bad}"


def test_byte_sum_does_not_wrap(ops, dev):
    """2400 x 2400 x 3 bytes of 255 exceed 2**32; a random image and a one-pixel window ride in the same launch"""
    h, w = JC.SUM_SIZE
    white = torch.full((3, h, w), 255, dtype=torch.uint8, device=dev)
    rnd = JC.make_image("random", 37, 53, seed=9)
    buf = torch.full((3, 9, 9), 200, dtype=torch.uint8, device=dev)
    buf[:, 4, 5] = torch.tensor([1, 2, 3], dtype=torch.uint8, device=dev)
    sums = ops.byte_sum_u8([white, _chw(rnd, dev), buf[:, 4:5, 5:6]])
    assert sums.dtype == torch.int64
    want = [3 * h * w * 255, int(rnd.sum(dtype=np.uint64)), 6]
    assert sums.tolist() == want and want[0] > 2 ** 32
    # and the contrast transform reads that sum: white stays white under any weight (mean 255 exactly)
    ops.colour_jitter_u8([white], [JC.spec_of(JC.PARAMS["contrast_0.8"])])
    assert int((white != 255).sum().item()) == 0


def test_one_batched_launch_equals_the_per_image_launches(ops, dev, cases):
    """all 240 images -- every size, every transform set, contrast drawn for some and not for others -- in ONE call against
    the per-image calls and the host; then a batch in which nothing was drawn"""
    single = [ops.colour_jitter_u8([_chw(img, dev)], [spec])[0] for _, img, spec, _ in cases]
    batch = [_chw(img, dev) for _, img, _, _ in cases]
    prep = ops.colour_jitter_u8_prepare(batch, [spec for _, _, spec, _ in cases])
    n_drawn = sum(1 for _, _, spec, _ in cases if spec[:, 0].any())
    n_contrast = sum(1 for _, _, spec, _ in cases if spec[0, 0])
    assert prep.n == n_drawn < len(cases) and prep.sums.numel() == n_contrast      # no descriptor for an image that drew nothing
    prep.launch()
    bad = {}
    for (cid, img, spec, ref), one, many in zip(cases, single, batch):
        n = int((one != many).sum().item()) + _mismatches(many, ref)
        if n:
            bad[cid] = n
    assert not bad, bad
    untouched = [_chw(img, dev) for _, img, _, _ in cases[:8]]
    prep = ops.colour_jitter_u8_prepare(untouched, [None, JC.spec_of(JC.PARAMS["none"])] * 4)
    assert prep.n == 0 and prep.blocks == 0 and prep.dev is None
    assert prep.launch() is untouched
    assert all(torch.equal(t.cpu(), _chw(img, torch.device("cpu"))) for t, (_, img, _, _) in zip(untouched, cases))


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def net(tmp_path_factory, dev):
    from test_model_gpu import make_model
    model, cfg = make_model(tmp_path_factory.mktemp("jitter_net"), PRECISION, seed=4)
    return model, cfg


def _dataset(root):
    rng = np.random.RandomState(11)
    recs = []
    for i, (h, w) in enumerate(((60, 90), (70, 50))):
        path = os.path.join(str(root), f"im{i}.png")
        Image.fromarray(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(path)
        recs.append({"file_name": path, "image_id": i, "height": h, "width": w,
                     "annotations": [{"bbox": [3, 4, 20, 15], "bbox_mode": 1, "category_id": 1, "iscrowd": 0},
                                     {"bbox": [22, 30, 18, 22], "bbox_mode": 1, "category_id": 5, "iscrowd": 0}]})
    return recs


def _mapped(cfg, recs, sizes, seed, prob, monkeypatch):
    """(raw records, host records) of the same dataset dicts from the same seed"""
    from detectron2_centernet_amd.data import TrafficLightDatasetMapper, dataset_mapper
    if prob is not None:
        monkeypatch.setattr(dataset_mapper, "_JITTER_PROB", prob)
    out = []
    for augment in (True, False):
        c = cfg.clone()
        c.INPUT.MIN_SIZE_TRAIN, c.INPUT.MIN_SIZE_TRAIN_SAMPLING, c.INPUT.MAX_SIZE_TRAIN = sizes, "choice", 1333
        c.INPUT.DEVICE_AUGMENT = augment
        mapper = TrafficLightDatasetMapper(c, is_train=True)
        np.random.seed(seed)
        out.append([mapper(r) for r in recs])
    return out


@pytest.mark.parametrize("sizes", [(64,), (48, 64)])
@pytest.mark.parametrize("prob", [1.0, None], ids=["all_on", "p0.15"])
def test_staged_images_and_targets_equal_the_host_mappers(net, dev, tmp_path, monkeypatch, sizes, prob):
    model, cfg = net
    recs = _dataset(tmp_path) * (1 if prob else 8)      # at 0.15: enough records for some transform to be drawn
    raw, host = _mapped(cfg, recs, sizes, 21, prob, monkeypatch)
    drawn = sum(int(r["jitter"][:, 0].sum()) for r in raw)
    print(f"MIN_SIZE_TRAIN {sizes}: {drawn} transforms drawn over {len(raw)} records")
    assert drawn == 4 * len(raw) if prob else 0 < drawn < 4 * len(raw)
    staged = model.stage_raw_train(raw)
    for s, r, h in zip(staged, raw, host):
        assert s.is_cuda and s.dtype == torch.uint8 and tuple(s.shape) == (3,) + tuple(r["resize_hw"])
        assert torch.equal(s.cpu(), h["image"]), f"{int((s.cpu() != h['image']).sum())} bytes differ"
    model.train()
    try:
        _, t_host = model.preprocess_image(host[:2])
        _, t_raw = model.preprocess_image([dict(r, image=s) for r, s in zip(raw[:2], staged[:2])])
    finally:
        model.eval()
    assert set(t_host) == set(t_raw) and t_host["reg_mask"].sum().item() == 4
    for k in t_host:
        assert torch.equal(t_host[k], t_raw[k]), k


def test_training_losses_of_raw_records_equal_host_records(net, dev, tmp_path, monkeypatch):
    model, cfg = net
    raw, host = _mapped(cfg, _dataset(tmp_path), (64,), 33, 1.0, monkeypatch)
    model.train()
    try:
        def run(records):
            return {k: v.detach().double().cpu() for k, v in model(records).items()}
        h1, h2, r = run(host), run(host), run(raw)
        with pytest.raises(KeyError, match="raw or host-mapped as a whole"):
            model([raw[0], host[1]])
    finally:
        model.eval()
    exact = all(torch.equal(h1[k], h2[k]) for k in h1)
    print(f"two runs of the host path bit-identical: {exact}; branch: {'torch.equal' if exact else 'noise bound'}")
    assert set(r) == set(h1) == {"hm_loss", "wh_loss", "off_loss"} and all(torch.isfinite(v) for v in r.values())
    for k in h1:
        print(f"{k}: host {h1[k].item():.9g} host again {h2[k].item():.9g} raw {r[k].item():.9g}")
        if exact:
            assert torch.equal(r[k], h1[k]), k
        else:
            noise = (h2[k] - h1[k]).abs().item() / abs(h1[k].item())
            assert (r[k] - h1[k]).abs().item() / abs(h1[k].item()) <= 4 * noise + 1e-5, k


def test_trainer_runs_on_raw_records(dev, tmp_path, monkeypatch):
    from test_model_gpu import make_model
    from detectron2_centernet_amd.engine.train_loop import SimpleTrainer
    model, cfg = make_model(tmp_path, PRECISION, seed=6)
    cfg.SOLVER.IMS_PER_BATCH = 2
    raw, _ = _mapped(cfg, _dataset(tmp_path), (48, 64), 5, 1.0, monkeypatch)
    tr = SimpleTrainer(model, None, cfg)
    p0 = tr.optimizer.flat_param.clone()
    for _ in range(2):
        losses = tr.run_step(raw)
        assert set(losses) == {"hm_loss", "wh_loss", "off_loss"}
        assert all(torch.isfinite(torch.as_tensor(float(v))) for v in losses.values())
    assert torch.isfinite(tr.optimizer.flat_param).all() and (tr.optimizer.flat_param - p0).abs().max() > 0
