"""G22: the reference's native COCO scorer (detectron2/layers/csrc/cocoeval/cocoeval.cpp: EvaluateImages + Accumulate) on a
seeded synthetic dataset (run with the reference checkout at make_golden.REF, on the CPU; needs g++ and pybind11).

The reference source is compiled into a temporary directory OUTSIDE the repository, together with the small binding stub
below (this project's own text: one `run(params, ious, gts, dts)` that builds the annotation lists from tuples).  Only data is
written: g22_cocoeval.npz holds

  inputs      boxes f32 [N,4] XYXY (the f32 values the device sees), scores f32 [N] (two decimals: ties are the rule),
              classes / image i32 [N] (contiguous indices, in shuffled order), image_ids i64 [I] (sorted),
              gt_boxes f64 [NG,4] XYWH, gt_area f64 [NG] (drawn independently of the box area), gt_crowd u8, gt_image /
              gt_classes i32 [NG], gt_ids i64 [NG] (>= 1), and the parameters iou_thrs, rec_thrs, max_dets, area_rngs;
  ious        the IoUs that were fed (numpy f64, the formula of DESIGN.md 7.7; pycocotools, which computes them for the
              reference, is absent): iou_cells i32 [C,2] = (image, category) of every cell with detections and ground truth,
              iou_off i64 [C+1] into iou_flat, each block [nd, G] over the cell's detections / ground truths in input order;
  outputs     precision [T,R,K,A,M], recall [T,K,A,M], scores_out [T,R,K,A,M] as the reference returned them.

Conditions on the inputs, asserted below from the reference's own output: see main()."""
import os
import subprocess
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import cocoeval_ref as CR  # noqa: E402
import make_golden as G  # noqa: E402

STUB = r"""
#include "cocoeval.h"
#include <tuple>
namespace ce = detectron2::COCOeval;
using Row = std::tuple<uint64_t, double, double, bool, bool>;   // id, score, area, is_crowd, ignore
using Rows = std::vector<std::vector<std::vector<Row>>>;

static ce::ImageCategoryInstances<ce::InstanceAnnotation> annotations(const Rows& rows) {
  ce::ImageCategoryInstances<ce::InstanceAnnotation> out(rows.size());
  for (size_t i = 0; i < rows.size(); ++i) {
    out[i].resize(rows[i].size());
    for (size_t c = 0; c < rows[i].size(); ++c)
      for (const Row& r : rows[i][c])
        out[i][c].emplace_back(std::get<0>(r), std::get<1>(r), std::get<2>(r), std::get<3>(r), std::get<4>(r));
  }
  return out;
}

static py::dict run(const py::object& params, const ce::ImageCategoryInstances<std::vector<double>>& ious, const Rows& gts,
                    const Rows& dts) {
  const auto area = params.attr("areaRng").cast<std::vector<std::array<double, 2>>>();
  const auto thrs = params.attr("iouThrs").cast<std::vector<double>>();
  const int top = params.attr("maxDets").cast<std::vector<int>>().back();
  return ce::Accumulate(params, ce::EvaluateImages(area, top, thrs, ious, annotations(gts), annotations(dts)));
}

PYBIND11_MODULE(g22_scorer, m) { m.def("run", &run); }
"""

I, K, W, H = 48, 6, 640.0, 480.0


def build_scorer(tmp):
    src = os.path.join(G.REF, "detectron2", "layers", "csrc", "cocoeval")
    stub = os.path.join(tmp, "g22_stub.cpp")
    with open(stub, "w") as f:
        f.write(STUB)
    inc = subprocess.check_output([sys.executable, "-m", "pybind11", "--includes"], text=True).split()
    out = os.path.join(tmp, "g22_scorer.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", *inc, "-I", src, os.path.join(src, "cocoeval.cpp"),
                           stub, "-o", out])
    sys.path.insert(0, tmp)
    import g22_scorer
    return g22_scorer


def make_inputs():
    rng = np.random.default_rng(22)
    gt_rows, dt_rows = [], []
    for i in range(I):
        has_gt, has_dt = i % 12 not in (5, 11), i % 12 not in (7, 11)
        gts = []
        if has_gt:
            for _ in range(int(rng.integers(2, 21))):
                side = float(np.exp(rng.uniform(np.log(10.0), np.log(300.0))))
                w, h = side * rng.uniform(0.6, 1.6), side * rng.uniform(0.6, 1.6)
                x, y = rng.uniform(0, max(1.0, W - w)), rng.uniform(0, max(1.0, H - h))
                box = np.round([x, y, w, h], 2)
                k = int(rng.integers(0, K - 1))                     # category K-1 has no ground truth at all
                gts.append((box, k))
                gt_rows.append((i, k, box, float(box[2] * box[3] * rng.uniform(0.4, 1.0)), int(rng.random() < 0.14)))
        if not has_dt:
            continue
        for box, k in gts:
            for _ in range(int(rng.integers(1, 3))):
                j = rng.normal(0, 0.08, 4)
                w, h = box[2] * (1 + j[2]), box[3] * (1 + j[3])
                x, y = box[0] + j[0] * box[2], box[1] + j[1] * box[3]
                kk = k if rng.random() < 0.9 else int(rng.integers(0, K))
                dt_rows.append((i, kk, x, y, w, h, float(np.round(rng.uniform(0.3, 1.0), 2))))
        nrand = 128 if i == 3 else int(rng.integers(20, 61))
        for _ in range(nrand):
            side = float(np.exp(rng.uniform(np.log(10.0), np.log(300.0))))
            w, h = side * rng.uniform(0.6, 1.6), side * rng.uniform(0.6, 1.6)
            x, y = rng.uniform(0, max(1.0, W - w)), rng.uniform(0, max(1.0, H - h))
            kk = 0 if i == 3 else int(rng.integers(0, K))
            dt_rows.append((i, kk, x, y, w, h, float(np.round(rng.uniform(0.01, 0.6), 2))))
    perm = rng.permutation(len(dt_rows))
    dt_rows = [dt_rows[p] for p in perm]
    d = np.array([r[2:6] for r in dt_rows], dtype=np.float64)
    x1, y1 = d[:, 0].astype(np.float32), d[:, 1].astype(np.float32)
    boxes = np.stack([x1, y1, (d[:, 0] + d[:, 2]).astype(np.float32), (d[:, 1] + d[:, 3]).astype(np.float32)], 1)
    return dict(
        boxes=boxes, scores=np.array([r[6] for r in dt_rows], dtype=np.float32),
        classes=np.array([r[1] for r in dt_rows], dtype=np.int32), image=np.array([r[0] for r in dt_rows], dtype=np.int32),
        image_ids=np.array([100 + 7 * i for i in range(I)], dtype=np.int64),
        gt_boxes=np.array([r[2] for r in gt_rows], dtype=np.float64), gt_area=np.array([r[3] for r in gt_rows], dtype=np.float64),
        gt_crowd=np.array([r[4] for r in gt_rows], dtype=np.uint8), gt_image=np.array([r[0] for r in gt_rows], dtype=np.int32),
        gt_classes=np.array([r[1] for r in gt_rows], dtype=np.int32), gt_ids=np.arange(1, len(gt_rows) + 1, dtype=np.int64))


def main():
    a = make_inputs()
    dxywh = CR.det_xywh(a["boxes"])
    darea = dxywh[:, 2] * dxywh[:, 3]
    dts = [[[] for _ in range(K)] for _ in range(I)]
    gts = [[[] for _ in range(K)] for _ in range(I)]
    dsel = [[[] for _ in range(K)] for _ in range(I)]
    gsel = [[[] for _ in range(K)] for _ in range(I)]
    for n in range(len(a["scores"])):
        i, k = int(a["image"][n]), int(a["classes"][n])
        dts[i][k].append((n + 1, float(a["scores"][n]), float(darea[n]), False, False))
        dsel[i][k].append(n)
    for n in range(len(a["gt_ids"])):
        i, k = int(a["gt_image"][n]), int(a["gt_classes"][n])
        c = bool(a["gt_crowd"][n])
        gts[i][k].append((int(a["gt_ids"][n]), 0.0, float(a["gt_area"][n]), c, c))
        gsel[i][k].append(n)
    ious = [[[] for _ in range(K)] for _ in range(I)]
    cells, off, flat = [], [0], []
    for i in range(I):
        for k in range(K):
            if dsel[i][k] and gsel[i][k]:
                m = CR.iou(dxywh[dsel[i][k]], a["gt_boxes"][gsel[i][k]], a["gt_crowd"][gsel[i][k]])
                # the reference indexes the rows by position in score order (pycocotools' computeIoU sorts the detections with
                # a stable argsort of -score before it computes them); the fixture keeps the block in input order
                ious[i][k] = m[np.argsort(-a["scores"][dsel[i][k]].astype(np.float64), kind="stable")].tolist()
                cells.append((i, k))
                flat.append(m.reshape(-1))
                off.append(off[-1] + m.size)
    params = types.SimpleNamespace(iouThrs=CR.IOU_THRS.tolist(), recThrs=CR.REC_THRS.tolist(), maxDets=list(CR.MAX_DETS),
                                   areaRng=[list(map(float, r)) for r in CR.AREA_RNGS], useCats=1, catIds=list(range(K)),
                                   imgIds=a["image_ids"].tolist())
    with tempfile.TemporaryDirectory() as tmp:
        assert not os.path.abspath(tmp).startswith(os.path.dirname(os.path.dirname(HERE)) + os.sep)
        res = build_scorer(tmp).run(params, ious, gts, dts)
    T, R, A, M = len(params.iouThrs), len(params.recThrs), len(params.areaRng), len(params.maxDets)
    assert list(res["counts"]) == [T, R, K, A, M]
    precision = np.array(res["precision"], dtype=np.float64).reshape(T, R, K, A, M)
    recall = np.array(res["recall"], dtype=np.float64).reshape(T, K, A, M)
    scores_out = np.array(res["scores"], dtype=np.float64).reshape(T, R, K, A, M)

    # ---- the conditions on the inputs, from the reference's own output
    stats = CR.summarize(precision, recall)
    print("AP, AP50, AP75, APs, APm, APl =", np.round(stats[:6], 4))
    assert all(0.05 <= s <= 0.95 for s in stats[:6]), stats
    assert (precision[:, :, K - 1] == -1).all() and (precision[:, :, :K - 1] > -1).all()      # one category without ground truth,
    assert np.isclose((precision == -1).mean(), 1.0 / K)                                     # every area range valid elsewhere
    ncrowd = int(a["gt_crowd"].sum())
    assert ncrowd >= 50, ncrowd
    ratio = a["gt_area"] / (a["gt_boxes"][:, 2] * a["gt_boxes"][:, 3])
    assert ratio.min() >= 0.4 - 1e-9 and ratio.max() <= 1.0 + 1e-9 and ratio.std() > 0.1
    counts = np.array([[len(dsel[i][k]) for k in range(K)] for i in range(I)])
    assert counts.max() > 100 and (counts > 10).sum() >= 20, (counts.max(), (counts > 10).sum())
    distinct = len(np.unique(a["scores"]))
    assert distinct <= 100 and np.array_equal(np.round(a["scores"].astype(np.float64), 2).astype(np.float32), a["scores"])
    ties_in_cell = sum(len(set(a["scores"][s].tolist())) < len(s) for row in dsel for s in row if s)
    assert ties_in_cell >= 20
    per_img_d, per_img_g = counts.sum(1), np.bincount(a["gt_image"], minlength=I)
    assert ((per_img_d == 0) & (per_img_g > 0)).any() and ((per_img_d > 0) & (per_img_g == 0)).any()
    assert ((per_img_d == 0) & (per_img_g == 0)).any()
    assert a["boxes"].dtype == np.float32 and (a["gt_ids"] >= 1).all()
    # the maxDets cut: the three columns differ
    assert not np.array_equal(recall[..., 0], recall[..., 1]) and not np.array_equal(recall[..., 1], recall[..., 2])
    print(f"{len(a['scores'])} detections ({distinct} distinct scores), {len(a['gt_ids'])} ground truths ({ncrowd} crowd), "
          f"largest cell {counts.max()}, {(counts > 10).sum()} cells > 10, {ties_in_cell} cells with tied scores")
    np.savez_compressed(
        os.path.join(HERE, "g22_cocoeval.npz"), **a, iou_thrs=CR.IOU_THRS, rec_thrs=CR.REC_THRS,
        max_dets=np.array(CR.MAX_DETS, dtype=np.int32), area_rngs=np.array(CR.AREA_RNGS, dtype=np.float64),
        iou_cells=np.array(cells, dtype=np.int32), iou_off=np.array(off, dtype=np.int64), iou_flat=np.concatenate(flat),
        precision=precision, recall=recall, scores_out=scores_out)
    print("G22 written to", HERE)


if __name__ == "__main__":
    main()
