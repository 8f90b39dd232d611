"""COCO box-AP scoring in plain numpy / Python loops, written from the definition in DESIGN.md 7.7 (the reference's native
scorer: precision = tp / (tp + fp), lower-bound sampling of the recall thresholds).  The CPU oracle of the HIP scorer for
inputs the G22 fixture does not cover; test_cocoeval_host.py pins it to the fixture with np.array_equal."""
import numpy as np

IOU_THRS = np.linspace(0.5, 0.95, int(np.round((0.95 - 0.5) / 0.05)) + 1, endpoint=True)
REC_THRS = np.linspace(0.0, 1.00, int(np.round((1.00 - 0.0) / 0.01)) + 1, endpoint=True)
MAX_DETS = [1, 10, 100]
AREA_RNGS = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]


def det_xywh(boxes_xyxy_f32):
    """XYXY f32 -> XYWH f64, width and height taken in f32 (what the reference pipeline does before it leaves the tensor)"""
    b = np.asarray(boxes_xyxy_f32, dtype=np.float32).reshape(-1, 4)
    out = np.empty(b.shape, dtype=np.float64)
    out[:, 0], out[:, 1] = b[:, 0], b[:, 1]
    out[:, 2], out[:, 3] = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    return out


def iou(dt, gt, crowd):
    """dt [D,4], gt [G,4] XYWH f64, crowd [G] -> [D,G] f64"""
    dt, gt = np.asarray(dt, dtype=np.float64).reshape(-1, 4), np.asarray(gt, dtype=np.float64).reshape(-1, 4)
    crowd = np.asarray(crowd).astype(bool)
    out = np.zeros((len(dt), len(gt)), dtype=np.float64)
    for d in range(len(dt)):
        dx, dy, dw, dh = dt[d]
        w = np.minimum(dx + dw, gt[:, 0] + gt[:, 2]) - np.maximum(dx, gt[:, 0])
        h = np.minimum(dy + dh, gt[:, 1] + gt[:, 3]) - np.maximum(dy, gt[:, 1])
        inter = w * h
        da, ga = dw * dh, gt[:, 2] * gt[:, 3]
        union = np.where(crowd, da, da + ga - inter)
        ok = (w > 0) & (h > 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            out[d] = np.where(ok, inter / union, 0.0)
    return out


def match_cell(ious, dt_area, gt_area, gt_crowd, iou_thrs, area_rng):
    """one (image, category) cell, one area range; detections in score order (already truncated).  Returns
    (matched [T,D] bool, ignored [T,D] bool, number of non-ignored ground truths)"""
    D, G = len(dt_area), len(gt_area)
    lo, hi = area_rng
    gt_ign = np.array([bool(gt_crowd[g]) or gt_area[g] < lo or gt_area[g] > hi for g in range(G)], dtype=bool)
    order = [g for g in range(G) if not gt_ign[g]] + [g for g in range(G) if gt_ign[g]]     # stable partition
    T = len(iou_thrs)
    matched, ignored = np.zeros((T, D), dtype=bool), np.zeros((T, D), dtype=bool)
    for t in range(T):
        taken = np.zeros(G, dtype=bool)
        for d in range(D):
            best, m = min(iou_thrs[t], 1 - 1e-10), -1
            for g in order:
                if taken[g] and not gt_crowd[g]:
                    continue
                if m >= 0 and not gt_ign[m] and gt_ign[g]:
                    break
                if ious[d, g] >= best:
                    best, m = ious[d, g], g
            if m >= 0:
                taken[m] = True
                matched[t, d], ignored[t, d] = True, gt_ign[m]
            else:
                ignored[t, d] = dt_area[d] < lo or dt_area[d] > hi
    return matched, ignored, int((~gt_ign).sum())


def evaluate(boxes, scores, classes, image, gt_boxes, gt_area, gt_crowd, gt_image, gt_classes, I, K, iou_thrs=IOU_THRS,
             rec_thrs=REC_THRS, max_dets=MAX_DETS, area_rngs=AREA_RNGS, ious=None):
    """Detections: boxes f32 [N,4] XYXY, scores f32 [N], classes / image [N] (contiguous indices).  Ground truth: gt_boxes f64
    [NG,4] XYWH, gt_area, gt_crowd, gt_image, gt_classes [NG].  `ious` (optional): {(i, k): [nd, G]} over the cell's detections
    in INPUT order, used instead of computing them.  Returns precision [T,R,K,A,M], recall [T,K,A,M], scores [T,R,K,A,M]."""
    scores = np.asarray(scores, dtype=np.float32)
    classes, image = np.asarray(classes).astype(np.int64), np.asarray(image).astype(np.int64)
    gt_image, gt_classes = np.asarray(gt_image).astype(np.int64), np.asarray(gt_classes).astype(np.int64)
    gt_boxes = np.asarray(gt_boxes, dtype=np.float64).reshape(-1, 4)
    gt_area, gt_crowd = np.asarray(gt_area, dtype=np.float64), np.asarray(gt_crowd).astype(bool)
    if len(classes) and (image.min() < 0 or image.max() >= I or classes.min() < 0 or classes.max() >= K):
        raise ValueError("detection with an image or class index out of range")
    dxywh = det_xywh(boxes)
    T, R, A, M = len(iou_thrs), len(rec_thrs), len(area_rngs), len(max_dets)
    top = max_dets[-1]
    dcell, gcell = {}, {}
    for n in np.argsort(image * K + classes, kind="stable"):
        dcell.setdefault((int(image[n]), int(classes[n])), []).append(int(n))
    for n in np.argsort(gt_image * K + gt_classes, kind="stable"):
        gcell.setdefault((int(gt_image[n]), int(gt_classes[n])), []).append(int(n))
    # per cell: score order, matches per area range
    cells = {}
    for key in sorted(set(dcell) | set(gcell)):
        di, gi = np.array(dcell.get(key, []), dtype=np.int64), np.array(gcell.get(key, []), dtype=np.int64)
        srt = np.argsort(-scores[di].astype(np.float64), kind="stable")[:top]
        dsel = di[srt]
        if ious is not None and len(di) and len(gi):
            io = np.asarray(ious[key], dtype=np.float64).reshape(len(di), len(gi))[srt]
        else:
            io = iou(dxywh[dsel], gt_boxes[gi], gt_crowd[gi])
        darea = dxywh[dsel, 2] * dxywh[dsel, 3]
        per_a = [match_cell(io, darea, gt_area[gi], gt_crowd[gi], iou_thrs, area_rngs[a]) for a in range(A)]
        cells[key] = (scores[dsel].astype(np.float64), per_a)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    scores_out = -np.ones((T, R, K, A, M))
    for k in range(K):
        keys = [key for key in cells if key[1] == k]          # sorted by image already
        for a in range(A):
            npig = sum(cells[key][1][a][2] for key in keys)
            if npig == 0:
                continue
            for mi, m in enumerate(max_dets):
                sc = np.concatenate([cells[key][0][:m] for key in keys]) if keys else np.zeros(0)
                mt = np.concatenate([cells[key][1][a][0][:, :m] for key in keys], axis=1) if keys else np.zeros((T, 0), bool)
                ig = np.concatenate([cells[key][1][a][1][:, :m] for key in keys], axis=1) if keys else np.zeros((T, 0), bool)
                srt = np.argsort(-sc, kind="stable")
                sc, mt, ig = sc[srt], mt[:, srt], ig[:, srt]
                for t in range(T):
                    tp = np.cumsum(mt[t] & ~ig[t]).astype(np.int64)
                    fp = np.cumsum(~mt[t] & ~ig[t]).astype(np.int64)
                    n = len(tp)
                    rc = tp.astype(np.float64) / float(npig)
                    den = (tp + fp).astype(np.float64)
                    pr = np.where(den > 0, tp.astype(np.float64) / np.where(den > 0, den, 1.0), 0.0)
                    recall[t, k, a, mi] = rc[-1] if n else 0.0
                    for i in range(n - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    idx = np.searchsorted(rc, rec_thrs, side="left")
                    for r, pi in enumerate(idx):
                        if pi < n:
                            precision[t, r, k, a, mi], scores_out[t, r, k, a, mi] = pr[pi], sc[pi]
                        else:
                            precision[t, r, k, a, mi], scores_out[t, r, k, a, mi] = 0.0, 0.0
    return precision, recall, scores_out


def summarize(precision, recall, iou_thrs=IOU_THRS, max_dets=MAX_DETS):
    """the twelve COCO stats; area ranges in the order all / small / medium / large"""
    iou_thrs = np.asarray(iou_thrs)

    def one(ap, thr=None, a=0, m=len(max_dets) - 1):
        s = precision if ap else recall
        if thr is not None:
            s = s[np.where(thr == iou_thrs)[0]]
        s = s[:, :, :, a, m] if ap else s[:, :, a, m]
        return float(np.mean(s[s > -1])) if (s > -1).any() else -1.0

    last = len(max_dets) - 1
    return np.array([one(1), one(1, .5), one(1, .75), one(1, a=1), one(1, a=2), one(1, a=3),
                     one(0, m=0), one(0, m=min(1, last)), one(0, m=min(2, last)), one(0, a=1), one(0, a=2), one(0, a=3)])


def coco_scale_inputs(I=5000, K=80, per_image=100, seed=3):
    """COCO-val scale, synthetic: ~7.4 annotations per image (areas x0.4-1 of the box, 2 % crowds), `per_image` detections per
    image, half of them jittered ground truths with the higher scores.  Returns (COCO annotation dicts, boxes f32 [N,4] XYXY,
    scores f32, classes i32, image i32, I, K); shared by the GPU test at this scale and tools/bench_cocoeval.py."""
    rng = np.random.default_rng(seed)
    ng = rng.poisson(7.4, I)
    gi = np.repeat(np.arange(I), ng)
    NG = len(gi)
    side = np.exp(rng.uniform(np.log(8), np.log(300), NG))
    wh = np.stack([side * rng.uniform(0.6, 1.6, NG), side * rng.uniform(0.6, 1.6, NG)], 1)
    xy = rng.uniform(0, 400, (NG, 2))
    gb = np.round(np.concatenate([xy, wh], 1), 2)
    gk = rng.integers(0, K, NG)
    anns = [{"id": n + 1, "image_id": int(gi[n]), "category_id": int(gk[n]), "bbox": gb[n].tolist(),
             "area": float(gb[n, 2] * gb[n, 3] * rng.uniform(0.4, 1.0)), "iscrowd": int(rng.random() < 0.02)} for n in range(NG)]
    N = I * per_image
    image = np.repeat(np.arange(I), per_image)
    start = np.concatenate([[0], np.cumsum(ng)])
    pick = (start[image] + (rng.random(N) * np.maximum(ng[image], 1)).astype(np.int64)).clip(0, NG - 1)
    from_gt = (rng.random(N) < 0.5) & (ng[image] > 0)
    jit = gb[pick] * (1 + rng.normal(0, 0.08, (N, 4)))
    rnd = np.concatenate([rng.uniform(0, 400, (N, 2)), np.exp(rng.uniform(np.log(8), np.log(300), (N, 2)))], 1)
    b = np.where(from_gt[:, None], jit, rnd)
    cls = np.where(from_gt & (rng.random(N) < 0.9), gk[pick], rng.integers(0, K, N))
    sc = np.round(np.where(from_gt, rng.uniform(0.3, 1, N), rng.uniform(0.01, 0.6, N)), 3)
    boxes = np.stack([b[:, 0], b[:, 1], b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]], 1).astype(np.float32)
    return anns, boxes, sc.astype(np.float32), cls.astype(np.int32), image.astype(np.int32), I, K
