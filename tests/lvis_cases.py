"""The LVIS box-AP rule in plain numpy / Python loops, written from its statement in DESIGN.md 7.17, and the case tables of
the LVIS tests.  It is the contract of the HIP scorer (csrc/lviseval.hip), which is held to it bit for bit; test_lvis_host.py
ties it to tests/cocoeval_ref.py (itself pinned to fixture G22) where LVIS coincides with COCO, and to hand-derived answers.

Every operation below is one f64 operation of numpy or of Python's float: each rounds once."""
import numpy as np

IOU_THRS = np.linspace(0.5, 0.95, 10)
REC_THRS = np.linspace(0.0, 1.0, 101)
AREA_RNGS = [[0.0, 1e10], [0.0, 1024.0], [1024.0, 9216.0], [9216.0, 1e10]]
MAX_DETS = 300
NEG, NEL = 1, 2          # bits of gt["lists"]
EPS = 2.0 ** -52


def make_gt(I, K, objects, neg=(), nel=()):
    """objects: (image, class, [x, y, w, h], area or None, ignore) in file order; neg / nel: (image, class) pairs -> the arrays the
    matcher takes: stable-sorted by (image, class) cell with CSR offsets [I*K+1]; area None = w * h"""
    n = len(objects)
    cell = np.array([o[0] * K + o[1] for o in objects], dtype=np.int64).reshape(n)
    order = np.argsort(cell, kind="stable")
    off = np.zeros(I * K + 1, dtype=np.int32)
    off[1:] = np.cumsum(np.bincount(cell, minlength=I * K))
    boxes = np.array([objects[j][2] for j in order], dtype=np.float64).reshape(n, 4)
    area = np.array([objects[j][3] if objects[j][3] is not None else objects[j][2][2] * objects[j][2][3] for j in order],
                    dtype=np.float64).reshape(n)
    ignore = np.array([1 if objects[j][4] else 0 for j in order], dtype=np.uint8).reshape(n)
    lists = np.zeros((I, K), dtype=np.uint8)
    for i, c in neg:
        lists[i, c] |= NEG
    for i, c in nel:
        lists[i, c] |= NEL
    return {"I": I, "K": K, "boxes": boxes, "area": area, "ignore": ignore, "off": off, "lists": lists,
            "image": (cell[order] // K).astype(np.int32), "classes": (cell[order] % K).astype(np.int32)}


def det_xywh(boxes):
    """XYXY f32 -> XYWH f64, width and height taken in f32, then widened"""
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    out = np.empty(b.shape, dtype=np.float64)
    out[:, 0], out[:, 1] = b[:, 0], b[:, 1]
    out[:, 2], out[:, 3] = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    return out


def iou_row(d, g):
    """one detection XYWH against ground truths [G,4] XYWH: ctdet_cocoeval_iou's formula with no crowd"""
    w = np.minimum(d[0] + d[2], g[:, 0] + g[:, 2]) - np.maximum(d[0], g[:, 0])
    h = np.minimum(d[1] + d[3], g[:, 1] + g[:, 3]) - np.maximum(d[1], g[:, 1])
    inter = w * h
    union = d[2] * d[3] + g[:, 2] * g[:, 3] - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((w > 0) & (h > 0), inter / union, 0.0)


def lvis_score(gt, boxes, scores, classes, image, iou_thrs=IOU_THRS, area_rngs=AREA_RNGS, rec_thrs=REC_THRS, max_dets=MAX_DETS):
    """-> {"precision" [T,R,K,A], "recall" [T,K,A], "npig" [K,A], "order", "cls_off", "flags" [N, A*T] (bit 0 matched, bit 1
    ignored; 255 where the detection takes no part), "first_tp" [T,K,A]: the first non-ignored detection of the order is a true
    positive (where the precision differs from tp / (tp + fp))}"""
    I, K = gt["I"], gt["K"]
    scores = np.asarray(scores, dtype=np.float32)
    classes, image = np.asarray(classes).astype(np.int64), np.asarray(image).astype(np.int64)
    N, T, A, R = len(scores), len(iou_thrs), len(area_rngs), len(rec_thrs)
    d = det_xywh(boxes)
    darea = d[:, 2] * d[:, 3]
    off, lists = gt["off"], gt["lists"]
    # the per-image cut: the max_dets detections of highest score, ties to the lower input index
    part = np.zeros(N, dtype=bool)
    by_image = {}
    for n in range(N):
        by_image.setdefault(int(image[n]), []).append(n)
    for mine in by_image.values():
        mine.sort(key=lambda n: (-float(scores[n]), n))
        part[mine[:max_dets]] = True
    # the drop: a class that is neither positive nor negative in its image
    for n in range(N):
        cell = image[n] * K + classes[n]
        if part[n] and not (off[cell + 1] > off[cell] or lists[image[n], classes[n]] & NEG):
            part[n] = False
    matched = np.zeros((N, A, T), dtype=bool)
    ignored = np.zeros((N, A, T), dtype=bool)
    npig = np.zeros((K, A), dtype=np.int32)
    by_cell = {}
    for n in range(N):
        if part[n]:
            by_cell.setdefault(int(image[n] * K + classes[n]), []).append(n)
    for cell in sorted(set(by_cell) | {int(c) for c in np.flatnonzero(np.diff(off))}):       # the cells that hold anything
        i, c = cell // K, cell % K
        g0, g1 = int(off[cell]), int(off[cell + 1])
        dets = by_cell.get(cell, [])
        dets.sort(key=lambda n: (-float(scores[n]), n))
        gb, garea, gign = gt["boxes"][g0:g1], gt["area"][g0:g1], gt["ignore"][g0:g1]
        ious = [iou_row(d[n], gb) for n in dets]
        nel = bool(lists[i, c] & NEL)
        for a, (lo, hi) in enumerate(area_rngs):
            ign = [bool(gign[g]) or garea[g] < lo or garea[g] > hi for g in range(g1 - g0)]
            npig[c, a] += sum(1 for v in ign if not v)
            walk = [g for g in range(g1 - g0) if not ign[g]] + [g for g in range(g1 - g0) if ign[g]]
            for t in range(T):
                taken = [False] * (g1 - g0)
                for j, n in enumerate(dets):
                    best, m = min(iou_thrs[t], 1 - 1e-10), None
                    for g in walk:
                        if taken[g]:
                            continue
                        if m is not None and not ign[m] and ign[g]:
                            break
                        if ious[j][g] < best:
                            continue
                        best, m = ious[j][g], g
                    if m is not None:
                        taken[m] = True
                        matched[n, a, t], ignored[n, a, t] = True, ign[m]
                    else:
                        ignored[n, a, t] = bool(darea[n] < lo or darea[n] > hi or nel)
    # the total order: class ascending, score descending, image ascending, input index
    order = [n for n in range(N) if part[n]]
    order.sort(key=lambda n: (classes[n], -float(scores[n]), image[n], n))
    cls_off = np.zeros(K + 1, dtype=np.int32)
    for n in order:
        cls_off[classes[n] + 1:] += 1
    precision, recall = -np.ones((T, R, K, A)), -np.ones((T, K, A))
    first_tp = np.zeros((T, K, A), dtype=bool)
    for c in range(K):
        seg = order[cls_off[c]:cls_off[c + 1]]
        for a in range(A):
            if npig[c, a] == 0:
                continue
            for t in range(T):
                tp = np.cumsum([matched[n, a, t] and not ignored[n, a, t] for n in seg]).astype(np.int64)
                fp = np.cumsum([not matched[n, a, t] and not ignored[n, a, t] for n in seg]).astype(np.int64)
                rc = tp.astype(np.float64) / float(npig[c, a])
                pr = tp.astype(np.float64) / ((fp + tp).astype(np.float64) + EPS)
                recall[t, c, a] = rc[-1] if len(seg) else 0.0
                counted = [j for j in range(len(seg)) if tp[j] + fp[j] > 0]
                first_tp[t, c, a] = bool(counted) and tp[counted[0]] == 1
                for j in range(len(seg) - 1, 0, -1):
                    if pr[j] > pr[j - 1]:
                        pr[j - 1] = pr[j]
                for r, x in enumerate(rec_thrs):
                    at = [j for j in range(len(seg)) if rc[j] >= x]
                    precision[t, r, c, a] = pr[at[0]] if at else 0.0
    flags = np.full((N, A * T), 255, dtype=np.uint8)
    for n in order:
        flags[n] = (matched[n].astype(np.uint8) | (ignored[n].astype(np.uint8) << 1)).reshape(A * T)
    rest = [n for n in range(N) if not part[n]]
    return {"precision": precision, "recall": recall, "npig": npig, "order": np.array(order + rest, dtype=np.int32),
            "cls_off": cls_off, "flags": flags, "first_tp": first_tp, "part": part}


def mean_valid(s):
    """mean over the entries > -1; -1 when there is none"""
    s = np.asarray(s)
    return float(np.mean(s[s > -1])) if (s > -1).any() else -1.0


def summarize(precision, recall, frequency):
    """the summaries of the rule, with LVIS's own ten thresholds and four area ranges"""
    res = {"AP": mean_valid(precision[:, :, :, 0]), "AP50": mean_valid(precision[0, :, :, 0]),
           "AP75": mean_valid(precision[5, :, :, 0]), "APs": mean_valid(precision[:, :, :, 1]),
           "APm": mean_valid(precision[:, :, :, 2]), "APl": mean_valid(precision[:, :, :, 3])}
    for f in "rcf":
        res["AP" + f] = mean_valid(precision[:, :, [k for k, v in enumerate(frequency) if v == f], 0])
    for a, lbl in enumerate(("", "s", "m", "l")):
        res[f"AR{lbl}@300"] = mean_valid(recall[:, :, a])
    return res


# ---- hand-derived cases: name -> (gt, boxes f32 [N,4] XYXY, scores f32 [N], classes i32 [N], image i32 [N])
ONE = 1.0 / (1.0 + EPS)        # the precision of a lone first true positive
FAR = [500.0, 500.0, 510.0, 510.0]


def _case(gt, dets):
    """dets: (box XYXY, score, class, image)"""
    n = len(dets)
    return (gt, np.array([x[0] for x in dets], dtype=np.float32).reshape(n, 4), np.array([x[1] for x in dets], dtype=np.float32),
            np.array([x[2] for x in dets], dtype=np.int32), np.array([x[3] for x in dets], dtype=np.int32))


def hand_case(name):
    box = [0.0, 0.0, 10.0, 10.0]
    if name in ("nel_on", "nel_off"):
        # one ground truth; a stray detection (0.95) ahead of the exact one (0.9).  Not exhaustive: the stray is ignored, tp = [0, 1],
        # fp = [0, 0], pr = [0 / 2^-52, 1 / (1 + 2^-52)] -> envelope ONE everywhere.  Exhaustive: fp = [1, 1], pr = [0, 1/2] -> 0.5.
        gt = make_gt(1, 1, [(0, 0, box, None, 0)], nel=[(0, 0)] if name == "nel_on" else [])
        return _case(gt, [(FAR, 0.95, 0, 0), (box, 0.9, 0, 0)])
    if name in ("drop_with", "drop_without"):
        # class 1 is neither positive nor negative in image 0: its detection, the best-scored of all, changes nothing -- class 1
        # has a ground truth in image 1, so a counted false positive would show in its tables
        gt = make_gt(2, 2, [(0, 0, box, None, 0), (1, 1, box, None, 0)])
        dets = [(box, 0.9, 0, 0), (box, 0.8, 1, 1)]
        return _case(gt, ([(box, 0.99, 1, 0)] if name == "drop_with" else []) + dets)
    if name in ("neg_on", "neg_off"):
        # class 0 has no ground truth in image 0 and one in image 1.  Negative in image 0: its detection there (0.9) is a false
        # positive ahead of the true positive (0.8): pr = [0, 1/2] -> 0.5.  Not negative: dropped, the true positive stands alone: ONE.
        gt = make_gt(2, 1, [(1, 0, box, None, 0)], neg=[(0, 0)] if name == "neg_on" else [])
        return _case(gt, [(box, 0.9, 0, 0), (box, 0.8, 0, 1)])
    if name == "area_1024":
        # a 32 x 32 ground truth of area exactly 1024, detected exactly: both ends of a range are inclusive, so it counts (and its
        # detection, of area 1024, is in range) in small [0, 1024] and in medium [1024, 9216]; in large it is ignored: -1
        return _case(make_gt(1, 1, [(0, 0, [0.0, 0.0, 32.0, 32.0], 1024.0, 0)]), [([0.0, 0.0, 32.0, 32.0], 0.9, 0, 0)])
    if name == "prefers_non_ignored":
        # the detection is 10 x 10; ground truth 0 (10 x 6.2, inside it: IoU 0.62) is non-ignored, ground truth 1 (10 x 9.2: IoU 0.92)
        # has `ignore`.  At 0.5 .. 0.6 it takes ground truth 0 and the walk stops at the first ignored one: a true positive.
        # At 0.65 .. 0.9 ground truth 0 is below the threshold and ground truth 1 matches: the detection is ignored, nothing is
        # counted, precision 0 / 2^-52 = 0 at recall 0.  At 0.95 it matches nothing: a false positive.
        gt = make_gt(1, 1, [(0, 0, [0.0, 0.0, 10.0, 6.2], None, 0), (0, 0, [0.0, 0.0, 10.0, 9.2], None, 1)])
        return _case(gt, [(box, 0.9, 0, 0)])
    if name == "iou_half":
        # detection 1 x 1 inside a 2 x 1 ground truth: intersection 1, union 1 + 2 - 1 = 2, IoU exactly 0.5: `iou < best` is false at
        # the threshold 0.5, so it matches there and at no other threshold
        return _case(make_gt(1, 1, [(0, 0, [0.0, 0.0, 2.0, 1.0], None, 0)]), [([0.0, 0.0, 1.0, 1.0], 0.9, 0, 0)])
    if name == "tie_in_cell":
        # two exact detections of one ground truth with equal scores: the lower input index takes it, the other is a false
        # positive behind it: pr = [ONE, 1/2], recall 1 at position 0 -> ONE everywhere
        return _case(make_gt(1, 1, [(0, 0, box, None, 0)]), [(box, 0.5, 0, 0), (box, 0.5, 0, 0)])
    if name == "tie_across_images":
        # equal scores in two images: input index 0 is image 1's false positive (negative class there), input index 1 is image 0's
        # true positive.  The order goes by image index before input index: the true positive leads, pr = [ONE, 1/2] -> ONE;
        # by input index it would be [0, 1/2] -> 0.5
        gt = make_gt(2, 1, [(0, 0, box, None, 0)], neg=[(1, 0)])
        return _case(gt, [(box, 0.5, 0, 1), (box, 0.5, 0, 0)])
    if name in ("cut_301", "cut_300"):
        # 299 strays (0.9), then two detections at 0.5: the lower input index a stray, the higher one exact.  With 301 detections
        # the cut keeps the lower index of the tie and the true positive is lost: recall 0, precision 0.  With one stray fewer
        # (300 detections) it stays: tp at position 299, pr = 1 / (300 + 2^-52) = 1/300, recall 1.
        strays = 299 if name == "cut_301" else 298
        dets = [(FAR, 0.9, 0, 0)] * strays + [(FAR, 0.5, 0, 0), (box, 0.5, 0, 0)]
        return _case(make_gt(1, 1, [(0, 0, box, None, 0)]), dets)
    raise KeyError(name)


# ---- seam cases of the GPU tests: name -> (gt, boxes, scores, classes, image, {parameter overrides})
def _grid_boxes(rng, n, size=40, per_row=16):
    """n ground-truth boxes XYWH on a grid of cells `size` apart: neighbours do not overlap, so a jittered copy of one has that
    one as its best match; sides 12 .. 36 put the areas (144 .. 1296) on both sides of 1024"""
    out = []
    for j in range(n):
        x0, y0 = (j % per_row) * size, (j // per_row) * size
        out.append([float(x0), float(y0), float(rng.integers(12, size - 3)), float(rng.integers(12, size - 3))])
    return out


def cells_case(seed, I, K, gts, dets, ignore_share=0.15, neg_share=0.5, nel_share=0.3):
    """gts / dets: {(image, class): count}.  Detections of a cell are jittered copies of its ground truths (several per ground
    truth once there are more detections than ground truths: duplicates) mixed with boxes that match nothing; `area` is a
    share of the box (as a segment's is), a sixth of the ground truths carry `ignore`; half of the cells without ground truth are
    negative (the detections of the others are dropped), a third of all cells are not exhaustive; scores on a coarse grid."""
    rng = np.random.default_rng(seed)
    objects, cell_boxes = [], {}
    for (i, k), n in sorted(gts.items()):
        bs = _grid_boxes(rng, n)
        cell_boxes[(i, k)] = bs
        objects += [(i, k, b, float(b[2] * b[3] * rng.uniform(0.5, 1.0)), bool(rng.random() < ignore_share)) for b in bs]
    neg = [(i, k) for i in range(I) for k in range(K) if gts.get((i, k), 0) == 0 and rng.random() < neg_share]
    nel = [(i, k) for i in range(I) for k in range(K) if rng.random() < nel_share]
    boxes, classes, image = [], [], []
    for (i, k), n in sorted(dets.items()):
        bs = cell_boxes.get((i, k), [])
        for _ in range(n):
            if bs and rng.random() < 0.8:
                b = np.array(bs[int(rng.integers(len(bs)))], dtype=np.float64)
                b = np.array([b[0], b[1], b[0] + b[2], b[1] + b[3]]) + rng.uniform(-2.5, 2.5, 4)
            else:
                x, y = rng.uniform(0, 600, 2)
                b = np.array([x, y, x + rng.uniform(4, 120), y + rng.uniform(4, 120)])
            boxes.append(b)
            classes.append(k)
            image.append(i)
    n = len(boxes)
    perm = rng.permutation(n)
    scores = (rng.integers(1, 400, n) / 400.0).astype(np.float32)       # ties are the rule: image and input index decide often
    return (make_gt(I, K, objects, neg, nel), np.array(boxes, dtype=np.float32).reshape(n, 4)[perm], scores,
            np.array(classes, dtype=np.int32)[perm], np.array(image, dtype=np.int32)[perm])


GT_COUNTS = (0, 1, 63, 64, 65, 130)
DET_COUNTS = (1, 64, 65, 130)
IMAGE_COUNTS = (299, 300, 301)


def build_case(name):
    if name == "gt_seams":          # one image per ground-truth count, a handful of detections each; class 1 without ground truth
        gts = {(i, 0): n for i, n in enumerate(GT_COUNTS)}
        dets = {(i, 0): 9 for i in range(len(GT_COUNTS))}
        dets.update({(i, 1): 3 for i in range(len(GT_COUNTS))})
        return cells_case(1, len(GT_COUNTS), 2, gts, dets, neg_share=0.6) + ({},)
    if name == "gt_130_many_dets":  # more than 128 ground truths: taken flags in the workspace, with duplicates on them
        return cells_case(2, 1, 1, {(0, 0): 130}, {(0, 0): 300}) + ({},)
    if name == "det_seams":         # one image per detection count over 20 ground truths
        gts = {(i, 0): 20 for i in range(len(DET_COUNTS))}
        dets = {(i, 0): n for i, n in enumerate(DET_COUNTS)}
        return cells_case(3, len(DET_COUNTS), 1, gts, dets) + ({},)
    if name == "image_cut":         # images of 299, 300 and 301 detections over three classes, at max_dets = 300
        gts = {(i, k): 6 for i in range(3) for k in range(3)}
        dets = {}
        for i, n in enumerate(IMAGE_COUNTS):
            dets.update({(i, 0): 100, (i, 1): 100, (i, 2): n - 200})
        return cells_case(4, 3, 3, gts, dets) + ({},)
    if name == "cut_small":         # the same seam at max_dets = 7: images of 6, 7, 8 and 20 detections
        gts = {(i, k): 3 for i in range(4) for k in range(2)}
        dets = {(0, 0): 3, (0, 1): 3, (1, 0): 4, (1, 1): 3, (2, 0): 4, (2, 1): 4, (3, 0): 12, (3, 1): 8}
        return cells_case(5, 4, 2, gts, dets) + ({"max_dets": 7},)
    if name == "t1":
        return cells_case(6, 3, 2, {(i, k): 5 for i in range(3) for k in range(2)},
                          {(i, k): 12 for i in range(3) for k in range(2)}) + ({"iou_thrs": np.array([0.5])},)
    if name == "a1":
        return cells_case(7, 3, 2, {(i, k): 5 for i in range(3) for k in range(2)},
                          {(i, k): 12 for i in range(3) for k in range(2)}) + ({"area_rngs": [[0.0, 1e10]]},)
    if name == "k20":               # K = 20: every class has cells with and without ground truth, negatives and drops
        gts = {(i, k): (i + k) % 4 for i in range(4) for k in range(20)}
        dets = {(i, k): (3 * i + k) % 7 for i in range(4) for k in range(20)}
        return cells_case(8, 4, 20, gts, dets) + ({},)
    if name == "i1":
        return cells_case(9, 1, 3, {(0, 0): 4, (0, 1): 7}, {(0, 0): 10, (0, 1): 5, (0, 2): 2}, neg_share=1.0) + ({},)
    if name == "chunks":            # a class segment of four 256-element chunks, true positives in every one
        gts = {(i, 0): 30 for i in range(24)}
        dets = {(i, 0): 40 for i in range(24)}
        return cells_case(10, 24, 1, gts, dets, ignore_share=0.1) + ({},)
    raise KeyError(name)


CASES = ("gt_seams", "gt_130_many_dets", "det_seams", "image_cut", "cut_small", "t1", "a1", "k20", "i1", "chunks")
HAND_CASES = ("nel_on", "nel_off", "drop_with", "drop_without", "neg_on", "neg_off", "area_1024", "prefers_non_ignored", "iou_half",
              "tie_in_cell", "tie_across_images", "cut_301", "cut_300")


def lvis_scale_inputs(I=19809, K=1203, per_image=300, objects=244000, seed=17):
    """LVIS-val scale, synthetic: `objects` annotations over I images with a long-tailed class distribution, ~5 negative and ~1
    not-exhaustive classes per image, `per_image` detections per image, a third of them jittered ground truths with the
    higher scores.  Returns (gt, boxes f32 [N,4], scores f32, classes i32, image i32, frequency); shared by
    tools/bench_lviseval.py and its host alternative.  Built with numpy throughout: make_gt's loops are for small cases."""
    rng = np.random.default_rng(seed)
    weight = 1.0 / (1.0 + np.arange(K)) ** 1.3
    weight /= weight.sum()
    NG = int(objects)
    gi = np.sort(rng.integers(0, I, NG))
    gk = rng.choice(K, NG, p=weight)
    wh = np.exp(rng.uniform(np.log(8), np.log(300), (NG, 2)))
    xy = rng.uniform(0, 400, (NG, 2))
    gb = np.round(np.concatenate([xy, wh], 1), 2)
    cell = gi.astype(np.int64) * K + gk
    order = np.argsort(cell, kind="stable")
    off = np.zeros(I * K + 1, dtype=np.int32)
    off[1:] = np.cumsum(np.bincount(cell, minlength=I * K))
    lists = np.zeros((I, K), dtype=np.uint8)
    lists[np.repeat(np.arange(I), 5), rng.integers(0, K, I * 5)] |= NEG
    lists[np.arange(I), rng.integers(0, K, I)] |= NEL
    gt = {"I": I, "K": K, "boxes": gb[order], "area": (gb[:, 2] * gb[:, 3] * rng.uniform(0.4, 1.0, NG))[order],
          "ignore": np.zeros(NG, dtype=np.uint8), "off": off, "lists": lists,
          "image": gi[order].astype(np.int32), "classes": gk[order].astype(np.int32)}
    N = I * per_image
    image = np.repeat(np.arange(I), per_image)
    ng = np.bincount(gi, minlength=I)
    start = np.concatenate([[0], np.cumsum(ng)])
    pick = (start[image] + (rng.random(N) * np.maximum(ng[image], 1)).astype(np.int64)).clip(0, NG - 1)
    from_gt = (rng.random(N) < 0.33) & (ng[image] > 0)
    jit = gb[pick] * (1 + rng.normal(0, 0.08, (N, 4)))
    rnd = np.concatenate([rng.uniform(0, 400, (N, 2)), np.exp(rng.uniform(np.log(8), np.log(300), (N, 2)))], 1)
    b = np.where(from_gt[:, None], jit, rnd)
    cls = np.where(from_gt & (rng.random(N) < 0.9), gk[pick], rng.choice(K, N, p=weight))
    sc = np.round(np.where(from_gt, rng.uniform(0.3, 1, N), rng.uniform(0.01, 0.6, N)), 3)
    boxes = np.stack([b[:, 0], b[:, 1], b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]], 1).astype(np.float32)
    count = np.bincount(gk, minlength=K)
    frequency = ["r" if c <= 10 else "c" if c <= 100 else "f" for c in count]
    return gt, boxes, sc.astype(np.float32), cls.astype(np.int32), image.astype(np.int32), frequency
