"""The device affine warp on the GPU (csrc/warp.hip through ops.warp_affine_u8) against data.warp.warp_affine_u8_reference,
byte for byte: zero mismatches, no tolerance, on every case of tests/warp_cases.py, from HWC and CHW sources, host and
device resident, with the channel order reversed, into fresh tensors and into windows of sentinel-filled buffers whose
other bytes must survive; one batched launch against per-image launches; a stale table.  Then end to end: raw training
records (INPUT.AFFINE with INPUT.DEVICE_AUGMENT) through CenterNet give the image bytes of host-mapped records made from the
same seed, qualify for the captured training step, and SimpleTrainer.run_step trains on them."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import warp_cases as WC

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
PRECISION = "f16"


@pytest.fixture(scope="module")
def ops(dev):
    import detectron2_centernet_amd.ops as ops
    return ops


@pytest.fixture(scope="module")
def cases():
    """(name, image HWC, M, flip, (out_h, out_w), reference HWC), computed once; read only"""
    from detectron2_centernet_amd.data.warp import warp_affine_u8_reference
    out = []
    for name, img, M, flip, (oh, ow) in WC.case_inputs():
        ref = warp_affine_u8_reference(img, M, oh, ow, flip)
        img.setflags(write=False)
        ref.setflags(write=False)
        out.append((name, img, M, flip, (oh, ow), ref))
    return out


def _mismatches(got_chw, ref_hwc):
    got = got_chw.permute(1, 2, 0).cpu().numpy()
    assert got.shape == ref_hwc.shape, (got.shape, ref_hwc.shape)
    return int((got != ref_hwc).sum())


def _src_hwc_host(img, dev):
    return img.transpose(2, 0, 1)                                        # numpy HWC view: travels in the call's upload


def _src_hwc_device(img, dev):
    return torch.from_numpy(np.array(img)).to(dev).permute(2, 0, 1)      # interleaved on the device: lanes run along channels


def _src_chw_device(img, dev):
    return torch.from_numpy(np.array(img.transpose(2, 0, 1), order="C")).to(dev)      # planes: lanes run along columns


def _src_chw_host(img, dev):
    return torch.from_numpy(np.array(img.transpose(2, 0, 1), order="C"))      # a CPU tensor


SOURCES = {"hwc_host": _src_hwc_host, "hwc_device": _src_hwc_device, "chw_device": _src_chw_device, "chw_host": _src_chw_host}


@pytest.mark.parametrize("source", list(SOURCES))
def test_kernel_equals_the_reference_byte_for_byte(ops, dev, cases, source):
    bad = {}
    for name, img, M, flip, out_hw, ref in cases:
        out = ops.warp_affine_u8([SOURCES[source](img, dev)], [(M, flip)], out_hw, device=dev)[0]
        assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (3,) + tuple(out_hw) and out.is_contiguous()
        n = _mismatches(out, ref)
        if n:
            bad[name] = n
    assert len(cases) == len(WC.CASES) >= 10
    assert not bad, f"{source}: mismatching bytes per case {bad}"


def test_reversed_channel_order(ops, dev, cases):
    """the source read with channel stride -1 from channel 2, on the host (numpy view) and on the device (flipped plane order
    is a copy there: the reversed view is given as a host array and as device planes of the reversed image)"""
    bad = {}
    for name, img, M, flip, out_hw, ref in cases:
        rev = np.ascontiguousarray(img[:, :, ::-1])
        view = rev.transpose(2, 0, 1)[::-1]            # logical channels back in img's order, stride -1
        assert view.strides[0] == -1 and np.array_equal(view.transpose(1, 2, 0), img)
        n = _mismatches(ops.warp_affine_u8([view], [(M, flip)], out_hw, device=dev)[0], ref)
        planes = np.array(rev.transpose(2, 0, 1), order="C")[::-1]      # CHW planes, channel stride -H*W
        assert planes.strides[0] < 0
        n += _mismatches(ops.warp_affine_u8([planes], [(M, flip)], out_hw, device=dev)[0], ref)
        if n:
            bad[name] = n
    assert not bad, bad


def test_destination_window_inside_a_wider_buffer(ops, dev, cases):
    """planar (a staging batch) and interleaved destinations: the window holds the reference's bytes, every byte outside it
    stays the sentinel"""
    bad = {}
    for name, img, M, flip, (oh, ow), ref in cases:
        n = 0
        for planar in (True, False):
            if planar:
                buf = torch.full((2, 3, oh + 5, ow + 7), SENTINEL, dtype=torch.uint8, device=dev)
                win = buf[1, :, 2:2 + oh, 3:3 + ow]
            else:
                buf = torch.full((oh + 5, ow + 7, 3), SENTINEL, dtype=torch.uint8, device=dev)
                win = buf[2:2 + oh, 3:3 + ow].permute(2, 0, 1)
            got = ops.warp_affine_u8([_src_hwc_host(img, dev)], [(M, flip)], (oh, ow), outs=[win])[0]
            assert got.data_ptr() == win.data_ptr()
            n += _mismatches(win, ref)
            win.fill_(SENTINEL)
            n += int((buf != SENTINEL).sum().item())
        if n:
            bad[name] = n
    assert not bad, bad


def test_one_batched_launch_equals_the_per_image_launches(ops, dev):
    """three sources of different sizes (one flipped, one a device tensor) in ONE launch into windows of one sentinel-filled
    batch; then the same descriptors with n = 1"""
    from detectron2_centernet_amd.data.warp import pack_warp, warp_affine_u8_reference
    oh, ow = WC.BATCH_OUT
    imgs = [WC.make_image(h, w, seed=40 + i) for i, ((h, w), _, _) in enumerate(WC.BATCH)]
    warps = [torch.from_numpy(pack_warp(np.array(M, dtype=np.float64), flip)) for _, M, flip in WC.BATCH]
    refs = [warp_affine_u8_reference(im, M, oh, ow, flip) for im, (_, M, flip) in zip(imgs, WC.BATCH)]
    srcs = [_src_hwc_host(imgs[0], dev), _src_hwc_host(imgs[1], dev), _src_chw_device(imgs[2], dev)]
    buf = torch.full((3, 3, oh + 2, ow + 3), SENTINEL, dtype=torch.uint8, device=dev)
    wins = [buf[b, :, 1:1 + oh, 2:2 + ow] for b in range(3)]
    prep = ops.warp_affine_u8_prepare(srcs, warps, (oh, ow), outs=wins)
    assert len(prep.desc) == 3 and prep.blocks == 3 * 2 * 2 and prep.desc["blk0"].tolist() == [0, 4, 8]
    prep.launch()
    first = buf.clone()
    prep.launch()                                             # a second identical launch changes nothing
    assert torch.equal(buf, first)
    assert [_mismatches(w, r) for w, r in zip(wins, refs)] == [0, 0, 0]
    for w in wins:
        w.fill_(SENTINEL)
    assert int((buf != SENTINEL).sum().item()) == 0
    for src, warp, ref in zip(srcs, warps, refs):             # n = 1 through the same entry point
        one = ops.warp_affine_u8_prepare([src], [warp], (oh, ow), device=dev)
        assert len(one.desc) == 1 and one.blocks == 4
        assert _mismatches(one.launch()[0], ref) == 0


def test_stale_table_returns_without_a_fault(ops, dev):
    """a valid table of a LARGER source launched on a small one: entries point far beyond it.  Every tap is clamped into the
    source it is launched on, so the call returns; its bytes are those of the same table on the small source (the taps
    beyond it contribute 0), which the reference gives too"""
    from detectron2_centernet_amd.data.warp import warp_affine_u8_reference
    small = WC.make_image(6, 9, seed=70)
    M = np.array([[7.5, 0.3, 100.0], [-0.2, 9.0, 50.0]])      # a walk over most of a 600 x 800 source
    big = WC.make_image(600, 800, seed=71)
    oh, ow = 64, 96
    assert _mismatches(ops.warp_affine_u8([big.transpose(2, 0, 1)], [(M, False)], (oh, ow), device=dev)[0],
                       warp_affine_u8_reference(big, M, oh, ow)) == 0
    out = torch.full((3, oh, ow), SENTINEL, dtype=torch.uint8, device=dev)
    ops.warp_affine_u8([small.transpose(2, 0, 1)], [(M, False)], (oh, ow), outs=[out])
    torch.cuda.synchronize()
    assert _mismatches(out, warp_affine_u8_reference(small, M, oh, ow)) == 0
    M0 = np.array([[7.5, 0.3, -20.0], [-0.2, 9.0, -16.0]])     # the same walk crossing the small source: some taps inside
    ref = warp_affine_u8_reference(small, M0, oh, ow)
    assert ref.any() and _mismatches(ops.warp_affine_u8([small.transpose(2, 0, 1)], [(M0, False)], (oh, ow), device=dev)[0], ref) == 0


def test_refusals(ops, dev):
    img = torch.zeros(3, 4, 4, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="int32"):
        ops.warp_affine_u8([img], [([[1, 0, 2.2e6], [0, 1, 0]], False)], (4, 4))
    with pytest.raises(ValueError, match="16384"):
        ops.warp_affine_u8([torch.zeros(3, 1, 16385, dtype=torch.uint8, device=dev)], [([[1, 0, 0], [0, 1, 0]], False)], (4, 4))
    with pytest.raises(NotImplementedError, match="no CPU implementation"):
        ops.warp_affine_u8([img.cpu()], [([[1, 0, 0], [0, 1, 0]], False)], (4, 4), device=torch.device("cpu"))


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def net(tmp_path_factory, dev):
    from test_model_gpu import make_model
    model, cfg = make_model(tmp_path_factory.mktemp("warp_net"), PRECISION, seed=4)
    return model, cfg


def _dataset(root):
    rng = np.random.RandomState(11)
    recs = []
    for i, (h, w) in enumerate(((48, 80), (100, 60))):
        path = os.path.join(str(root), f"im{i}.png")
        Image.fromarray(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(path)
        recs.append({"file_name": path, "image_id": i, "height": h, "width": w,
                     "annotations": [{"bbox": [w // 4, h // 4, w // 3, h // 3], "bbox_mode": 1, "category_id": 1, "iscrowd": 0},
                                     {"bbox": [w // 2, h // 2, w // 4, h // 5], "bbox_mode": 1, "category_id": 5, "iscrowd": 0}]})
    return recs


def _mapped(cfg, recs, seed, monkeypatch):
    """(raw records, host records) of the same dataset dicts from the same seed, every jitter drawn"""
    from detectron2_centernet_amd.data import TrafficLightDatasetMapper, dataset_mapper
    monkeypatch.setattr(dataset_mapper, "_JITTER_PROB", 1.0)
    out = []
    for augment in (True, False):
        c = cfg.clone()
        c.INPUT.AFFINE.ENABLED, c.INPUT.AFFINE.OUTPUT_SIZE = True, (64, 64)
        c.INPUT.DEVICE_AUGMENT = augment
        mapper = TrafficLightDatasetMapper(c, is_train=True)
        np.random.seed(seed)
        out.append([mapper(r) for r in recs])
    return out


def test_staged_images_equal_the_host_mappers(net, dev, tmp_path, monkeypatch):
    model, cfg = net
    raw, host = _mapped(cfg, _dataset(tmp_path) * 4, 21, monkeypatch)      # 8 records: both flip states are drawn
    assert all(int(r["jitter"][:, 0].sum()) == 4 and tuple(r["resize_hw"]) == (64, 64) for r in raw)
    assert {bool(r["warp"][0, 3]) for r in raw} == {True, False}
    staged = model.stage_raw_train(raw)
    for s, r, h in zip(staged, raw, host):
        assert s.is_cuda and s.dtype == torch.uint8 and tuple(s.shape) == (3, 64, 64)
        assert torch.equal(s.cpu(), h["image"]), f"{int((s.cpu() != h['image']).sum())} bytes differ"
        assert torch.equal(r["instances"].gt_boxes.tensor, h["instances"].gt_boxes.tensor)
    plain = {k: v for k, v in raw[1].items() if k != "warp"}
    with pytest.raises(KeyError, match="warped .* or resized as a whole"):
        model.stage_raw_train([raw[0], plain])


def test_trainer_takes_warp_records_on_the_captured_path(dev, tmp_path, monkeypatch):
    from test_model_gpu import make_model
    from detectron2_centernet_amd.engine.train_loop import SimpleTrainer
    model, cfg = make_model(tmp_path, PRECISION, seed=6)
    cfg.SOLVER.IMS_PER_BATCH = 2
    raw, _ = _mapped(cfg, _dataset(tmp_path), 5, monkeypatch)
    tr = SimpleTrainer(model, None, cfg)
    tensors = tr._record_tensors(raw)
    assert tensors is not None and tuple(tensors[0].shape) == (2, 3, 64, 64) and tensors[0].dtype == torch.uint8
    p0 = tr.optimizer.flat_param.clone()
    losses = tr.run_step(raw)
    assert set(losses) == {"hm_loss", "wh_loss", "off_loss"}
    assert all(torch.isfinite(torch.as_tensor(float(v))) for v in losses.values())
    assert torch.isfinite(tr.optimizer.flat_param).all() and (tr.optimizer.flat_param - p0).abs().max() > 0
