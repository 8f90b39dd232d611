"""The Pascal VOC scoring rule of DESIGN.md 7.16 restated in numpy f64 (the oracle of the HIP scorer's tests and the host
alternative of tools/bench_voceval.py), and the table of cases the GPU tests run.

Nothing here imports the package under test: the restatement is checked on its own against the reference's recorded
results (tests/golden/g23_voceval.npz) in tests/test_voc_host.py."""
import math

import numpy as np

EPS = float(np.finfo(np.float64).eps)
THRESHOLDS = [t / 100.0 for t in range(50, 100, 5)]
POINTS_07 = np.arange(0.0, 1.1, 0.1)


# ---- quantisation: the reference's "{score:.3f} {x:.1f}" text round trip, in f64
def quantise_scores(scores):
    return np.rint(np.asarray(scores, dtype=np.float32).astype(np.float64) * 1000.0) / 1000.0


def quantise_boxes(boxes):
    """f32 [N,4] XYXY, 0-based -> f64 [N,4]: x1 / y1 plus one IN F32 (one rounding), then every coordinate to one decimal"""
    b = np.array(boxes, dtype=np.float32).reshape(-1, 4)
    b[:, 0] = b[:, 0] + np.float32(1.0)
    b[:, 1] = b[:, 1] + np.float32(1.0)
    return np.rint(b.astype(np.float64) * 10.0) / 10.0


def total_order(classes, qscores):
    """class ascending, quantised score descending, input index ascending"""
    n = len(classes)
    return np.lexsort((np.arange(n), -np.asarray(qscores), np.asarray(classes)))


def make_gt(I, K, objects):
    """objects: (image, class, difficult, [xmin, ymin, xmax, ymax]) -> arrays sorted (stably) by cell, CSR offsets [I*K+1]"""
    n = len(objects)
    cell = np.array([o[0] * K + o[1] for o in objects], dtype=np.int64).reshape(n)
    order = np.argsort(cell, kind="stable")
    off = np.zeros(I * K + 1, dtype=np.int32)
    np.cumsum(np.bincount(cell, minlength=I * K), out=off[1:])
    return {"I": I, "K": K, "boxes": np.array([objects[j][3] for j in order], dtype=np.float64).reshape(n, 4),
            "difficult": np.array([1 if objects[j][2] else 0 for j in order], dtype=np.uint8).reshape(n), "off": off}


def ap_11_point(rec, prec):
    ap = 0.0
    for x in POINTS_07:
        sel = rec >= x
        p = prec[sel].max() if sel.any() else 0.0
        ap = ap + p / 11.0
    return float(ap)


def ap_area_terms(rec, prec):
    """the terms (recall step) * (precision envelope) of the area form, by position"""
    mrec = np.concatenate([[0.0], rec, [1.0]])
    mpre = np.concatenate([[0.0], prec, [0.0]])
    env = np.maximum.accumulate(mpre[::-1])[::-1]
    pos = np.flatnonzero(mrec[1:] != mrec[:-1])
    with np.errstate(invalid="ignore"):
        return (mrec[pos + 1] - mrec[pos]) * env[pos + 1]


def ap_area(rec, prec):
    ap = 0.0
    for term in ap_area_terms(rec, prec):      # in position order
        ap = ap + term
    return float(ap)


def voc_score(gt, boxes, scores, classes, image, thresholds=THRESHOLDS):
    """-> order [N], cls_off [K+1], flags u8 [N,T] at the input index (0 neither, 1 TP, 2 FP), npos [K], rec / prec [T,N] by
    position of the order, ap07 / ap12 [K,T] (fractions), terms [K][T] (number of terms of the area sum)"""
    I, K, T = gt["I"], gt["K"], len(thresholds)
    classes, image = np.asarray(classes, dtype=np.int64), np.asarray(image, dtype=np.int64)
    N = len(classes)
    q, bq = quantise_scores(scores), quantise_boxes(boxes)
    order = total_order(classes, q)
    cls_off = np.searchsorted(classes[order], np.arange(K + 1)).astype(np.int32)
    thr = np.asarray(thresholds, dtype=np.float64)
    flags = np.zeros((N, T), dtype=np.uint8)
    taken = np.zeros((len(gt["difficult"]), T), dtype=bool)
    for o in order:
        cell = image[o] * K + classes[o]
        g0, g1 = gt["off"][cell], gt["off"][cell + 1]
        ovmax, jmax = -np.inf, -1
        if g1 > g0:
            g, bb = gt["boxes"][g0:g1], bq[o]
            iw = np.maximum(np.minimum(g[:, 2], bb[2]) - np.maximum(g[:, 0], bb[0]) + 1.0, 0.0)
            ih = np.maximum(np.minimum(g[:, 3], bb[3]) - np.maximum(g[:, 1], bb[1]) + 1.0, 0.0)
            inter = iw * ih
            uni = (bb[2] - bb[0] + 1.0) * (bb[3] - bb[1] + 1.0) + (g[:, 2] - g[:, 0] + 1.0) * (g[:, 3] - g[:, 1] + 1.0) - inter
            ov = inter / uni
            jmax = int(np.argmax(ov))
            ovmax = ov[jmax]
        for t in range(T):
            if ovmax > thr[t]:
                if gt["difficult"][g0 + jmax]:
                    flags[o, t] = 0
                elif taken[g0 + jmax, t]:
                    flags[o, t] = 2
                else:
                    flags[o, t] = 1
                    taken[g0 + jmax, t] = True
            else:
                flags[o, t] = 2
    gt_class = np.repeat(np.arange(I * K) % K, np.diff(gt["off"]))
    npos = np.bincount(gt_class[gt["difficult"] == 0], minlength=K).astype(np.int32)
    rec, prec = np.zeros((T, N)), np.zeros((T, N))
    ap07, ap12 = np.zeros((K, T)), np.zeros((K, T))
    terms = np.zeros((K, T), dtype=np.int64)
    for k in range(K):
        seg = order[cls_off[k]:cls_off[k + 1]]
        for t in range(T):
            tp = np.cumsum(flags[seg, t] == 1).astype(np.float64)
            fp = np.cumsum(flags[seg, t] == 2).astype(np.float64)
            with np.errstate(invalid="ignore", divide="ignore"):
                r = tp / float(npos[k])
            p = tp / np.maximum(tp + fp, EPS)
            rec[t, cls_off[k]:cls_off[k + 1]], prec[t, cls_off[k]:cls_off[k + 1]] = r, p
            ap07[k, t], ap12[k, t] = ap_11_point(r, p), ap_area(r, p)
            terms[k, t] = len(ap_area_terms(r, p))
    return {"order": order.astype(np.int32), "cls_off": cls_off, "flags": flags, "npos": npos, "rec": rec, "prec": prec,
            "ap07": ap07, "ap12": ap12, "terms": terms}


def area_bound(terms):
    """two sums of the same `terms` non-negative values of total <= 1 in different orders differ by at most this"""
    return (np.asarray(terms, dtype=np.float64) + 2.0) * 2.0 ** -52


def fsum_area(rec, prec):
    return math.fsum(ap_area_terms(rec, prec))


# ---- cases of the GPU tests: name -> (gt, boxes f32 [N,4], scores f32 [N], classes i32 [N], image i32 [N], thresholds)
def _grid_boxes(rng, n, size=24, per_row=16):
    """n ground-truth boxes (1-based, int) on a grid of cells `size` apart: neighbours do not overlap, so a jittered copy of
    one has that one as its best match"""
    out = []
    for j in range(n):
        x0, y0 = 1 + (j % per_row) * size, 1 + (j // per_row) * size
        w, h = int(rng.integers(8, size - 4)), int(rng.integers(8, size - 4))
        out.append([x0, y0, x0 + w, y0 + h])
    return out


def _cells_case(seed, I, K, gts, dets, difficult_share=0.2):
    """gts / dets: {(image, class): count}.  Detections of a cell are jittered copies of its ground truths (several per
    ground truth once there are more detections than ground truths: duplicates) mixed with boxes that match nothing."""
    rng = np.random.default_rng(seed)
    objects, cell_boxes = [], {}
    for (i, k), n in sorted(gts.items()):
        bs = _grid_boxes(rng, n)
        cell_boxes[(i, k)] = bs
        objects += [(i, k, bool(rng.random() < difficult_share), b) for b in bs]
    boxes, classes, image = [], [], []
    for (i, k), n in sorted(dets.items()):
        bs = cell_boxes.get((i, k), [])
        for d in range(n):
            if bs and rng.random() < 0.8:
                b = np.array(bs[int(rng.integers(len(bs)))], dtype=np.float64)
                b = b + rng.uniform(-2.5, 2.5, 4)
                b[:2] -= 1.0           # the model's boxes are 0-based
            else:
                x, y = rng.uniform(0, 300, 2)
                b = np.array([x, y, x + rng.uniform(4, 40), y + rng.uniform(4, 40)])
            boxes.append(b)
            classes.append(k)
            image.append(i)
    n = len(boxes)
    perm = rng.permutation(n)
    # scores on a coarse grid: ties within a class are the rule, so the input index decides often
    scores = (rng.integers(1, 400, n) / 400.0 + rng.integers(0, 3, n) * 0.0004).astype(np.float32)
    return (make_gt(I, K, objects), np.array(boxes, dtype=np.float32).reshape(n, 4)[perm], scores,
            np.array(classes, dtype=np.int32)[perm], np.array(image, dtype=np.int32)[perm])


def _first_wins_case():
    """65 ground truths in one cell, numbers 0 and 64 the same box (two lanes' strides apart: lane 0 sees both, in two rounds);
    two detections on it: the first takes ground truth 0, the second finds 0 again -- taken -- and is a false positive"""
    rng = np.random.default_rng(64)
    bs = _grid_boxes(rng, 64)
    bs.append(list(bs[0]))
    objects = [(0, 0, False, b) for b in bs]
    b0 = np.array(bs[0], dtype=np.float32)
    b0[:2] -= 1.0
    boxes = np.stack([b0, b0, np.array(bs[5], dtype=np.float32) - np.array([1, 1, 0, 0], dtype=np.float32)])
    return (make_gt(1, 1, objects), boxes, np.array([0.9, 0.8, 0.7], dtype=np.float32), np.zeros(3, dtype=np.int32),
            np.zeros(3, dtype=np.int32))


def _perfect_case():
    """every ground truth (none difficult) detected exactly once, nothing else"""
    rng = np.random.default_rng(7)
    I, K = 3, 4
    objects, boxes, classes, image = [], [], [], []
    for i in range(I):
        for k in range(K):
            for b in _grid_boxes(rng, int(rng.integers(1, 6))):
                objects.append((i, k, False, b))
                boxes.append([b[0] - 1.0, b[1] - 1.0, b[2], b[3]])
                classes.append(k)
                image.append(i)
    n = len(boxes)
    return (make_gt(I, K, objects), np.array(boxes, dtype=np.float32), rng.uniform(0.1, 0.9, n).astype(np.float32),
            np.array(classes, dtype=np.int32), np.array(image, dtype=np.int32))


GT_COUNTS = (0, 1, 63, 64, 65, 130)
DET_COUNTS = (1, 64, 65, 130)


def build_case(name):
    if name == "gt_seams":          # one image per ground-truth count; a handful of detections each, class 1 without ground truth
        gts = {(i, 0): n for i, n in enumerate(GT_COUNTS)}
        dets = {(i, 0): 9 for i in range(len(GT_COUNTS))}
        dets[(2, 1)] = 3
        return _cells_case(1, len(GT_COUNTS), 2, gts, dets) + (THRESHOLDS,)
    if name == "gt_130_many_dets":  # taken words in the workspace, with duplicates on them
        return _cells_case(2, 1, 1, {(0, 0): 130}, {(0, 0): 300}) + (THRESHOLDS,)
    if name == "det_seams":         # one image per detection count over 20 ground truths: more than one AP chunk in class 0
        gts = {(i, 0): 20 for i in range(len(DET_COUNTS))}
        dets = {(i, 0): n for i, n in enumerate(DET_COUNTS)}
        return _cells_case(3, len(DET_COUNTS), 1, gts, dets) + (THRESHOLDS,)
    if name == "first_wins":
        return _first_wins_case() + ([0.5, 0.7],)
    if name == "t1":
        return _cells_case(4, 3, 2, {(i, k): 5 for i in range(3) for k in range(2)},
                           {(i, k): 12 for i in range(3) for k in range(2)}) + ([0.5],)
    if name == "k20":               # K = 20, T = 10: every class has cells with and without ground truth
        gts = {(i, k): (i + k) % 4 for i in range(4) for k in range(20)}
        dets = {(i, k): (3 * i + k) % 7 for i in range(4) for k in range(20)}
        return _cells_case(5, 4, 20, gts, dets) + (THRESHOLDS,)
    if name == "i1":
        return _cells_case(6, 1, 3, {(0, 0): 4, (0, 1): 7}, {(0, 0): 10, (0, 1): 5, (0, 2): 2}) + (THRESHOLDS,)
    if name == "chunks":            # a class segment of several 256-element chunks, true positives in every one
        gts = {(i, 0): 30 for i in range(24)}
        dets = {(i, 0): 40 for i in range(24)}
        return _cells_case(8, 24, 1, gts, dets, difficult_share=0.1) + (THRESHOLDS,)
    if name == "perfect":
        return _perfect_case() + (THRESHOLDS,)
    raise KeyError(name)


CASES = ("gt_seams", "gt_130_many_dets", "det_seams", "first_wins", "t1", "k20", "i1", "chunks", "perfect")


def voc_scale_inputs(I=4952, K=20, per_image=100, seed=7):
    """VOC2007-test scale, synthetic: ~3 objects per image (a fifth of them difficult), `per_image` detections per image, half
    of them jittered ground truths with the higher scores.  Returns (gt, boxes f32 [N,4], scores f32, classes i32, image i32);
    shared by tools/bench_voceval.py and its host alternative."""
    rng = np.random.default_rng(seed)
    ng = rng.poisson(3.0, I)
    gi = np.repeat(np.arange(I), ng)
    NG = len(gi)
    wh = np.exp(rng.uniform(np.log(16), np.log(300), (NG, 2)))
    xy = rng.uniform(1, 200, (NG, 2))
    gb = np.rint(np.concatenate([xy, xy + wh], 1)).astype(np.int64)
    gk = rng.integers(0, K, NG)
    gd = rng.random(NG) < 0.2
    gt = make_gt(I, K, [(int(gi[n]), int(gk[n]), bool(gd[n]), gb[n].tolist()) for n in range(NG)])
    N = I * per_image
    image = np.repeat(np.arange(I), per_image)
    start = np.concatenate([[0], np.cumsum(ng)])
    pick = (start[image] + (rng.random(N) * np.maximum(ng[image], 1)).astype(np.int64)).clip(0, max(NG - 1, 0))
    from_gt = (rng.random(N) < 0.5) & (ng[image] > 0)
    size = (gb[pick, 2:] - gb[pick, :2]).astype(np.float64)
    jit = gb[pick] + rng.normal(0, 0.08, (N, 4)) * np.concatenate([size, size], 1) - np.array([1.0, 1.0, 0.0, 0.0])
    x = rng.uniform(0, 300, (N, 2))
    rnd = np.concatenate([x, x + np.exp(rng.uniform(np.log(16), np.log(300), (N, 2)))], 1)
    boxes = np.where(from_gt[:, None], jit, rnd).astype(np.float32)
    cls = np.where(from_gt & (rng.random(N) < 0.9), gk[pick], rng.integers(0, K, N))
    sc = np.where(from_gt, rng.uniform(0.3, 1, N), rng.uniform(0.01, 0.6, N))
    return gt, boxes, sc.astype(np.float32), cls.astype(np.int32), image.astype(np.int32)
