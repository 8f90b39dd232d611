"""The device resize on the GPU (csrc/resize.hip through ops.resize_u8) against what the host mapper produces today --
`ResizeTransform.apply_image`, i.e. Pillow -- byte for byte: zero mismatches, no tolerance, on every case of
tests/resize_cases.py in every addressing form, and one batched launch against the per-image launches.  Then end to end:
raw records (INPUT.DEVICE_RESIZE) through CenterNet, the ragged path, CenterNetWithTTA and DefaultPredictor give the staging
bytes and the detections of host-resized records.

Detections are compared with torch.equal when two runs of the host path are themselves bit-identical at that shape (checked
first, printed); otherwise with the bound test_model_gpu.py uses against the oracle (classes equal, scores within the mode's
heat-map tolerance, boxes within 1e-4)."""
import numpy as np
import pytest
import torch
from PIL import Image

import resize_cases as RC
from detectron2_centernet_amd.data import transforms as T

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
PRECISION = "f16"


def _pil(img, new):
    img = np.ascontiguousarray(img)
    return T.ResizeTransform(img.shape[0], img.shape[1], new[0], new[1]).apply_image(img)


@pytest.fixture(scope="module")
def inputs():
    """(id, image HWC, (new_h, new_w), Pillow's result HWC), computed once; read only"""
    out = []
    for cid, img, new in RC.all_inputs():
        ref = _pil(img, new)
        img.setflags(write=False)
        ref.setflags(write=False)
        out.append((cid, img, new, ref))
    return out


@pytest.fixture(scope="module")
def ops(dev):
    import detectron2_centernet_amd.ops as ops
    return ops


def _mismatches(got_hwc, ref):
    assert got_hwc.shape == ref.shape, (got_hwc.shape, ref.shape)      # none left out
    return int((got_hwc != ref).sum())


def _form_hwc(ops, dev, img, new, ref):
    src = torch.from_numpy(np.array(img)).to(dev)                        # [H, W, 3], what a decoder gives
    out = ops.resize_u8([src.permute(2, 0, 1)], [new])[0]
    assert out.is_contiguous() and tuple(out.shape) == (3,) + tuple(new)
    return _mismatches(out.permute(1, 2, 0).cpu().numpy(), ref)


def _form_chw(ops, dev, img, new, ref):
    src = torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))).to(dev)      # planes, what TTA holds
    out = ops.resize_u8([src], [new])[0]
    return _mismatches(out.permute(1, 2, 0).cpu().numpy(), ref)


def _form_reversed(ops, dev, img, new, ref):
    """RGB <-> BGR as a channel stride of -1 (a host view: the upload keeps the image's own byte order), against Pillow on
    img[:, :, ::-1]"""
    view = img[:, :, ::-1]
    assert view.strides[2] == -1
    out = ops.resize_u8([view.transpose(2, 0, 1)], [new], device=dev)[0]
    return _mismatches(out.permute(1, 2, 0).cpu().numpy(), _pil(view, new))


def _form_window(ops, dev, img, new, ref):
    """destination = a window of a sentinel-filled buffer, planar and interleaved: every byte outside stays the sentinel"""
    bad = 0
    src = torch.from_numpy(np.array(img)).to(dev).permute(2, 0, 1)
    nh, nw = new
    for planar in (True, False):
        if planar:
            buf = torch.full((3, nh + 5, nw + 7), SENTINEL, dtype=torch.uint8, device=dev)
            win = buf[:, 2:2 + nh, 3:3 + nw]
        else:
            buf = torch.full((nh + 5, nw + 7, 3), SENTINEL, dtype=torch.uint8, device=dev)
            win = buf[2:2 + nh, 3:3 + nw].permute(2, 0, 1)
        got = ops.resize_u8([src], [new], outs=[win])[0]
        assert got.data_ptr() == win.data_ptr()
        bad += _mismatches(win.permute(1, 2, 0).cpu().numpy(), ref)
        win.fill_(SENTINEL)
        bad += int((buf != SENTINEL).sum().item())
    return bad


FORMS = {"hwc": _form_hwc, "chw": _form_chw, "reversed": _form_reversed, "window": _form_window}


@pytest.mark.parametrize("form", list(FORMS))
def test_kernel_equals_pillow_byte_for_byte(ops, dev, inputs, form):
    bad = {}
    for cid, img, new, ref in inputs:
        n = FORMS[form](ops, dev, img, new, ref)
        if n:
            bad[cid] = n
    assert not bad, f"{form}: mismatching bytes per case {bad}"


def test_one_batched_launch_equals_the_per_image_launches(ops, dev, inputs):
    """all 27 images of every size in ONE launch -- device and host sources mixed, interleaved and planar -- against the
    per-image launches (the one-image entry point) and against Pillow"""
    srcs = []
    for i, (cid, img, new, ref) in enumerate(inputs):
        if i % 3 == 0:
            srcs.append(torch.from_numpy(np.array(img)).to(dev).permute(2, 0, 1))
        elif i % 3 == 1:
            srcs.append(img.transpose(2, 0, 1))                                    # host, HWC memory
        else:
            srcs.append(torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))))      # host tensor, planes
    sizes = [new for _, _, new, _ in inputs]
    single = [ops.resize_u8([s], [n], device=dev)[0] for s, n in zip(srcs, sizes)]
    batched = ops.resize_u8(srcs, sizes, device=dev)
    bad = {}
    for (cid, img, new, ref), one, many in zip(inputs, single, batched):
        n = int((one != many).sum().item()) + _mismatches(many.permute(1, 2, 0).cpu().numpy(), ref)
        if n:
            bad[cid] = n
    assert not bad, bad
    # a second call re-uses the pinned upload buffer: the first call's images are not disturbed
    again = ops.resize_u8(srcs[::-1], sizes[::-1], device=dev)[::-1]
    assert all(torch.equal(a, b) for a, b in zip(again, batched))


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def net(tmp_path_factory, dev):
    from test_model_gpu import make_model
    model, cfg = make_model(tmp_path_factory.mktemp("resize_net"), PRECISION, seed=4)
    model.score_threshold = 0.0
    model.wh[-1].bias.data.fill_(3.0)          # boxes of non-degenerate size
    return model, cfg


def _raw(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3), dtype=np.uint8)


def _records(raws, size, max_size=1333):
    """(raw records, host-resized records) of the same images, as the two mappers emit them"""
    raw_recs, host_recs = [], []
    for raw in raws:
        h, w = raw.shape[:2]
        new = T.ResizeShortestEdge.output_size(h, w, size, max_size)
        raw_recs.append({"image_raw": raw, "resize_hw": new, "height": h, "width": w})
        host_recs.append({"image": torch.from_numpy(np.ascontiguousarray(_pil(raw, new).transpose(2, 0, 1))), "height": h, "width": w})
    return raw_recs, host_recs


def _equal(a, b):
    return all(x["instances"].image_size == y["instances"].image_size and len(x["instances"]) == len(y["instances"])
               and torch.equal(x["instances"].pred_boxes.tensor, y["instances"].pred_boxes.tensor)
               and torch.equal(x["instances"].scores, y["instances"].scores)
               and torch.equal(x["instances"].pred_classes, y["instances"].pred_classes) for x, y in zip(a, b))


def _same_detections(raw_out, host_fn, what):
    from test_model_gpu import HM_TOL
    host, host2 = host_fn(), host_fn()
    exact = _equal(host, host2)
    print(f"{what}: two runs of the host path bit-identical: {exact}")
    assert len(raw_out) == len(host)
    for r, h in zip(raw_out, host):
        ri, hi = r["instances"], h["instances"]
        assert ri.image_size == hi.image_size and len(ri) == len(hi) > 0
        if exact:
            assert torch.equal(ri.pred_boxes.tensor, hi.pred_boxes.tensor)
            assert torch.equal(ri.scores, hi.scores) and torch.equal(ri.pred_classes, hi.pred_classes)
        else:
            assert torch.equal(ri.pred_classes, hi.pred_classes)
            assert (ri.scores - hi.scores).abs().max().item() <= HM_TOL[PRECISION]
            assert torch.allclose(ri.pred_boxes.tensor, hi.pred_boxes.tensor, atol=1e-4, rtol=1e-6)


def test_raw_records_give_the_staging_bytes_and_detections_of_host_records(net, dev):
    """96 x 128, the size of test_model_gpu.py's eval forward, from raw images a few pixels off (two raw sizes with one
    target: both passes run, two table sets in one launch)"""
    model, cfg = net
    raw_recs, host_recs = _records([_raw(90, 120, 1), _raw(93, 124, 2), _raw(90, 120, 3)], 96)
    assert all(r["resize_hw"] == (96, 128) for r in raw_recs)
    out = model(raw_recs)
    eng = list(model._engines.values())[-1]
    want = torch.stack([h["image"] for h in host_recs])
    assert torch.equal(eng.images.cpu(), want)                       # the staged uint8 batch: what the host mapper produces
    assert out[0]["instances"].image_size == (90, 120) and out[1]["instances"].image_size == (93, 124)
    n_engines = len(model._engines)
    _same_detections(out, lambda: model(host_recs), "same-size batch")
    assert len(model._engines) == n_engines                          # raw and host records share the captured engine
    _same_detections(model.forward_async(raw_recs).result(), lambda: model(host_recs), "forward_async")
    assert torch.equal(eng.images.cpu(), want)
    with pytest.raises(KeyError, match="raw or resized as a whole"):
        model([raw_recs[0], host_recs[1]])


def test_raw_ragged_batch(net, dev):
    model, cfg = net
    raw_recs, host_recs = _records([_raw(90, 120, 4), _raw(60, 50, 5)], 96)
    assert [r["resize_hw"] for r in raw_recs] == [(96, 128), (115, 96)]
    _same_detections(model(raw_recs), lambda: model(host_recs), "ragged batch")
    _same_detections(model.forward_async(raw_recs).result(), lambda: model(host_recs), "ragged forward_async")


def test_tta_resizes_raw_records_on_the_device(net, dev):
    from detectron2_centernet_amd.modeling import CenterNetWithTTA
    from test_tta_gpu import _tta_cfg
    model, cfg = net
    tta = CenterNetWithTTA(_tta_cfg(cfg, min_sizes=(96,), flip=True), model)
    raws = [_raw(90, 120, 6), _raw(90, 120, 7)]
    raw_recs = [{"image_raw": r} for r in raws]
    host_recs = [{"image": torch.from_numpy(np.ascontiguousarray(r.transpose(2, 0, 1)))} for r in raws]
    staged = tta._inputs(raw_recs)
    assert all(s["resize_hw"] == (96, 128) and (s["height"], s["width"]) == (90, 120) and "image" not in s for s in staged)
    out = tta(raw_recs)
    assert out[0]["instances"].image_size == (90, 120)
    _same_detections(out, lambda: tta(host_recs), "TTA, one MIN_SIZES entry, flip")
    _same_detections(tta.forward_async(raw_recs).result(), lambda: tta(host_recs), "TTA forward_async")
    assert not _equal(out, model(staged))                            # the flip test took part


@pytest.mark.parametrize("fmt", ["BGR", "RGB"])
def test_default_predictor(net, dev, tmp_path, fmt):
    from detectron2_centernet_amd.checkpoint import DetectionCheckpointer
    from detectron2_centernet_amd.data import TrafficLightDatasetMapper
    from detectron2_centernet_amd.engine import DefaultPredictor
    model, cfg = net
    cfg = cfg.clone()
    cfg.MODEL.WEIGHTS = DetectionCheckpointer(model, str(tmp_path), save_to_disk=True).save("net")
    cfg.MODEL.CENTERNET.SCORE_THRESH_TEST = 0.0
    cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST, cfg.INPUT.FORMAT = 96, 1333, fmt
    pred = DefaultPredictor(cfg)
    assert not pred.model.training
    for k, v in model.state_dict().items():
        assert torch.equal(pred.model.state_dict()[k], v), k           # MODEL.WEIGHTS went through the checkpointer
    rgb = _raw(90, 120, 8)
    path = str(tmp_path / "frame.png")
    Image.fromarray(rgb).save(path)
    record = TrafficLightDatasetMapper(cfg, is_train=False)({"file_name": path, "height": 90, "width": 120})
    assert tuple(record["image"].shape) == (3, 96, 128)
    bgr = np.ascontiguousarray(rgb[:, :, ::-1])                      # what cv2.imread gives
    out = pred(bgr)
    assert set(out) == {"instances"} and out["instances"].image_size == (90, 120)
    eng = list(pred.model._engines.values())[-1]
    assert torch.equal(eng.images[0].cpu(), record["image"])         # channel order INPUT.FORMAT, resized bytes of the mapper
    _same_detections([out], lambda: pred.model([record]), f"DefaultPredictor {fmt}")
    with pytest.raises(TypeError):
        pred(bgr.astype(np.float32))
