"""Multi-scale test augmentation's merge: the float64 restatement of the rule, the committed cases and
the margin checker.  No GPU, no project code: numpy only.

THE RULE (CenterNet's test code: `soft_nms(..., Nt=0.5, method=2)` per class, then the `max_per_image` cut).  The candidates of
one image are the detections of all passes, concatenated pass-major, each pass in the order it returned them; the candidate
index is the position in that concatenation.  Per class, with A the class's live candidates:
  1. pick m, the highest current score of A, ties to the lowest index; append (box_m, score_m, class); remove m from A;
  2. for every i still in A:  iw = min(x2_m, x2_i) - max(x1_m, x1_i) + 1,  ih likewise in y;  only when iw > 0 and ih > 0:
       ua = (x2_m-x1_m+1)(y2_m-y1_m+1) + (x2_i-x1_i+1)(y2_i-y1_i+1) - iw*ih,  ov = iw*ih / ua,
       score_i *= exp(-(ov*ov) / SIGMA);  if the new score_i < MIN_SCORE, remove i from A
     (a candidate that is never decayed is never removed);
  3. until A is empty.
Then all classes' outputs by score descending, ties to the lower class, then to the earlier selection; the first max_det.

THE PER-CANDIDATE BOUND.  The kernel evaluates the same expressions in f32, one rounding per operation (its file is compiled
with floating point contraction off), exp by the library's expf (at most 1 ulp).  With u = 2^-24 (half an ulp, the relative
error of one rounding) and first-order error counts in units of u:
  * a width / height term `x2 - x1 + 1`: two roundings                                                        -> 2
  * iw, ih: min / max are exact, then two roundings each                                                      -> 2 each
    (where `min - max` cancels, the absolute error of iw is at most u * (|min - max| + iw) <= u * (w_m + 1 + iw), and it enters
    the exponent through (ih / ua) * d(iw) <= d(iw) / w_m, w_m > 1: no more than the 2 units above, scaled by ov)
  * inter = iw * ih: 2 + 2 + 1                                                                                -> 5
  * the two areas: 2 + 2 + 1 each -> 5; their sum S: + 1 -> 6; ua = S - inter with inter <= min(area_m, area_i), so
    S <= 2 ua and inter <= ua: (6 * 2 + 5 * 1) + 1                                                            -> 18
  * ov = inter / ua: 5 + 18 + 1                                                                               -> 24
  * t = (ov * ov) / SIGMA: 2 * 24 + 2                                                                         -> 50, relative
  * the weight exp(-t) has the RELATIVE error |dt| = t * 50 u <= 50 u / SIGMA (ov <= 1, so t <= 1 / SIGMA), plus expf's 1 ulp
    (<= 2 u), and the product score * weight rounds once more                                                 -> 50 / SIGMA + 3
so one decay costs at most c = 50 / SIGMA + 3 units (103 at SIGMA = 0.5), and a candidate that received d decays is within
(d + 1) * c * 2^-24, relative, of the float64 value.  (The bound is a worst case, not a fit: a trial with numpy f32 against f64
on 200 clustered random cases saw at most 8.2 units per decay, the f32 evaluation of this file's restatement on the committed
cases at most 11.)

THE MARGIN CONDITION every committed case meets (check_margins, asserted on the CPU by tests/test_soft_nms_host.py) makes the
f32 kernel's DECISIONS those of the restatement: at every selection step the picked score and every other live score are exactly
tied, or both never decayed (f32 inputs: compared exactly in both arithmetics), or apart by more than twice the sum of their
bounds; every decayed score is that far from MIN_SCORE; so are neighbours in the final order (which covers the max_det cut);
and no evaluated pair has an iw / ih whose sign differs between f32 and f64.
"""
import numpy as np

U = 2.0 ** -24
SIGMA, MIN_SCORE = 0.5, 0.001


def c_units(sigma):
    """units of 2^-24 one decay may cost (derivation: the module docstring)"""
    return 50.0 / float(np.float32(sigma)) + 3.0


def bound(decays, sigma):
    """relative bound of a candidate's f32 score after `decays` decays"""
    return (np.asarray(decays, dtype=np.float64) + 1.0) * c_units(sigma) * U


def _apart(s1, d1, s2, d2, sigma):
    """the margin condition for two scores whose order (or equality) the f32 kernel must reproduce (arrays broadcast)"""
    s1, s2, d1, d2 = np.asarray(s1, np.float64), np.asarray(s2, np.float64), np.asarray(d1), np.asarray(d2)
    far = np.abs(s1 - s2) > 2.0 * (bound(d1, sigma) * np.abs(s1) + bound(d2, sigma) * np.abs(s2))
    return (s1 == s2) | ((d1 == 0) & (d2 == 0)) | far


def class_soft_nms(boxes, scores, sigma, min_score, dtype=np.float64, trace=None):
    """one class.  boxes [n,4], scores [n] in candidate order.  Returns (order, out_scores, decays): the candidates in
    selection order, the scores they were selected with and the number of decays each had received.  dtype=np.float32
    evaluates every operation in f32 (what the kernel does); trace (a list) receives the failed margin conditions."""
    f = dtype
    bx = np.asarray(boxes).astype(f)
    s = np.asarray(scores).astype(f).copy()
    sig, mn, one = f(np.float32(sigma)), f(np.float32(min_score)), f(1)
    n = len(s)
    live = np.ones(n, dtype=bool)
    dec = np.zeros(n, dtype=np.int64)
    order, out_s, out_d = [], [], []
    b32 = np.asarray(boxes).astype(np.float32)
    while live.any():
        idx = np.flatnonzero(live)
        m = idx[np.argmax(s[idx])]                      # first maximum: ties to the lowest index
        if trace is not None:
            for i in idx[~_apart(s[m], dec[m], s[idx], dec[idx], sigma)]:
                trace.append(f"selection {len(order)}: picked {m} ({s[m]!r}, {dec[m]} decays) vs live {i} ({s[i]!r}, {dec[i]} decays)")
        order.append(int(m)); out_s.append(s[m]); out_d.append(int(dec[m]))
        live[m] = False
        idx = np.flatnonzero(live)
        if len(idx) == 0:
            break
        iw = np.minimum(bx[m, 2], bx[idx, 2]) - np.maximum(bx[m, 0], bx[idx, 0]) + one
        ih = np.minimum(bx[m, 3], bx[idx, 3]) - np.maximum(bx[m, 1], bx[idx, 1]) + one
        if trace is not None:
            one32 = np.float32(1)
            iw32 = np.minimum(b32[m, 2], b32[idx, 2]) - np.maximum(b32[m, 0], b32[idx, 0]) + one32
            ih32 = np.minimum(b32[m, 3], b32[idx, 3]) - np.maximum(b32[m, 1], b32[idx, 1]) + one32
            if not (np.array_equal(iw > 0, iw32 > 0) and np.array_equal(ih > 0, ih32 > 0)):
                trace.append(f"selection {len(order) - 1}: an overlap's sign differs between f32 and f64")
        hit = (iw > 0) & (ih > 0)
        j = idx[hit]
        if len(j) == 0:
            continue
        iw, ih = iw[hit], ih[hit]
        am = (bx[m, 2] - bx[m, 0] + one) * (bx[m, 3] - bx[m, 1] + one)
        ai = (bx[j, 2] - bx[j, 0] + one) * (bx[j, 3] - bx[j, 1] + one)
        inter = iw * ih
        ua = am + ai - inter
        ov = inter / ua
        s[j] = s[j] * np.exp(-(ov * ov) / sig)
        dec[j] += 1
        if trace is not None:
            for i in j[~(np.abs(s[j] - mn) > 2.0 * bound(dec[j], sigma) * np.abs(s[j]))]:
                trace.append(f"candidate {i}: decayed score {s[i]!r} ({dec[i]} decays) too close to MIN_SCORE")
        live[j[s[j] < mn]] = False
    return np.asarray(order, dtype=np.int64), np.asarray(out_s, dtype=f), np.asarray(out_d, dtype=np.int64)


def merge_reference(passes, num_classes, sigma=SIGMA, min_score=MIN_SCORE, max_det=100, dtype=np.float64, trace=None):
    """the whole rule for a batch.  passes: [(boxes [B,K,4] f32, scores [B,K] f32, classes [B,K] i32, counts [B] i32)].
    Returns one dict per image: count (-1: a pass flagged the image), boxes f32 [count,4] and classes i32 [count] copied bit
    for bit, scores [count] in `dtype`, decays [count], survivors (before the cut)."""
    B = len(passes[0][3])
    out = []
    for b in range(B):
        cnts = [int(p[3][b]) for p in passes]
        if any(c < 0 for c in cnts):
            out.append({"count": -1})
            continue
        cnts = [min(c, p[1].shape[1]) for c, p in zip(cnts, passes)]
        boxes = np.concatenate([p[0][b, :c] for p, c in zip(passes, cnts)]).astype(np.float32).reshape(-1, 4)
        scores = np.concatenate([p[1][b, :c] for p, c in zip(passes, cnts)]).astype(np.float32)
        classes = np.concatenate([p[2][b, :c] for p, c in zip(passes, cnts)]).astype(np.int32)
        rows = []                                   # (score, class, selection order, candidate, decays)
        for c in range(num_classes):
            cand = np.flatnonzero(classes == c)
            if len(cand) == 0:
                continue
            sub = []
            order, s, d = class_soft_nms(boxes[cand], scores[cand], sigma, min_score, dtype, None if trace is None else sub)
            if trace is not None:
                trace.extend(f"image {b} class {c}: {t}" for t in sub)
            rows.extend((s[k], c, k, int(cand[order[k]]), int(d[k])) for k in range(len(order)))
        rows.sort(key=lambda r: (-float(r[0]), r[1], r[2]))
        if trace is not None:
            for r0, r1 in zip(rows, rows[1:]):
                if not bool(_apart(float(r0[0]), r0[4], float(r1[0]), r1[4], sigma)):
                    trace.append(f"image {b}: final neighbours {r0[0]!r} ({r0[4]} decays) and {r1[0]!r} ({r1[4]} decays)")
        keep = rows[:max_det]
        cand = np.asarray([r[3] for r in keep], dtype=np.int64)
        out.append({"count": len(keep), "survivors": len(rows), "boxes": boxes[cand].reshape(-1, 4), "classes": classes[cand],
                    "scores": np.asarray([r[0] for r in keep], dtype=dtype), "decays": np.asarray([r[4] for r in keep], dtype=np.int64)})
    return out


class Case:
    def __init__(self, name, passes, num_classes, max_det=100, sigma=SIGMA, min_score=MIN_SCORE):
        self.name, self.passes, self.num_classes = name, passes, num_classes
        self.max_det, self.sigma, self.min_score = max_det, sigma, min_score
        self._ref = None

    def reference(self):
        """computed once, shared by every test that needs it"""
        if self._ref is None:
            self._ref = merge_reference(self.passes, self.num_classes, self.sigma, self.min_score, self.max_det)
        return self._ref

    def __repr__(self):
        return self.name


def check_margins(case):
    """the failed conditions of the module docstring (empty: the case may be committed)"""
    trace = []
    merge_reference(case.passes, case.num_classes, case.sigma, case.min_score, case.max_det, trace=trace)
    return trace


def to_passes(images, widths):
    """images: per image a list of (x1, y1, x2, y2, score, class) in candidate order, dealt into passes of the given widths
    (image b fills pass 0 first, then pass 1, ...); what does not fit is an error.  Padding rows hold garbage on purpose."""
    B = len(images)
    passes = []
    for s, K in enumerate(widths):
        g = np.random.default_rng(1000 + s)
        boxes = (g.random((B, K, 4)) * 50).astype(np.float32)          # behind the counts: never to be read as candidates
        scores = g.random((B, K)).astype(np.float32)
        classes = np.zeros((B, K), dtype=np.int32)
        passes.append([boxes, scores, classes, np.zeros(B, dtype=np.int32)])
    for b, cands in enumerate(images):
        s, k = 0, 0
        for cand in cands:
            while s < len(widths) and k == widths[s]:
                s, k = s + 1, 0
            assert s < len(widths), "more candidates than the passes hold"
            passes[s][0][b, k] = cand[:4]
            passes[s][1][b, k] = cand[4]
            passes[s][2][b, k] = cand[5]
            k += 1
            passes[s][3][b] = k
    return [tuple(p) for p in passes]


def clustered(seed, n, classes, origin=0.0, extent=400.0, size=(20.0, 120.0)):
    """n candidates of a few objects x 2..12 near-copies each: (x1, y1, x2, y2, score, class) in a random order"""
    g = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        w, h = g.uniform(size[0], size[1], 2)
        x, y = origin + g.uniform(0, extent, 2)
        c = int(classes[g.integers(len(classes))])
        base = g.uniform(0.05, 0.95)
        for _ in range(int(g.integers(2, 13))):
            if len(out) == n:
                break
            dx, dy, dw, dh = g.normal(0, 0.06, 4) * (w, h, w, h)
            out.append((x + dx, y + dy, x + dx + w + dw, y + dy + h + dh, base * g.uniform(0.3, 1.0), c))
    perm = g.permutation(len(out))
    return [out[i] for i in perm]


def _cell(n, seed):
    """n candidates in the cell (image 0, class 1) of a 3-class problem, a handful in the neighbouring classes"""
    img = clustered(seed, n, [1]) + clustered(seed + 1, 7, [0, 2])
    g = np.random.default_rng(seed + 2)
    return [img[i] for i in g.permutation(len(img))]


def _ties():
    """exact ties of disjoint boxes: within a class, across classes, and a duplicate (same box, same score) in two passes"""
    return [
        (0, 0, 9, 9, 0.5, 2), (100, 0, 109, 9, 0.5, 2), (200, 0, 209, 9, 0.5, 0), (300, 0, 309, 9, 0.5, 1),
        (0, 100, 9, 109, 0.25, 1), (100, 100, 109, 109, 0.25, 1), (200, 100, 209, 109, 0.75, 2),
        (0, 200, 19, 219, 0.625, 0), (300, 300, 319, 319, 0.625, 0), (0, 200, 19, 219, 0.375, 0), (300, 300, 319, 319, 0.375, 0),
    ]


def _full(seed):
    """the capacity: 2048 candidates of one class in 16 passes of 128 (every lane of the wave holds 32 slots).  2000 boxes on
    a disjoint grid -- never decayed, scores on multiples of 1/64: ties by the hundred -- and 8 clusters of 6 near-copies"""
    g = np.random.default_rng(seed)
    img = [(40.0 * (i % 50), 40.0 * (i // 50), 40.0 * (i % 50) + 20, 40.0 * (i // 50) + 20, int(g.integers(1, 64)) / 64.0, 1)
           for i in range(2000)]
    img += clustered(seed + 1, 48, [1], origin=3000.0)
    return [img[i] for i in g.permutation(len(img))]


def _survivors(images, widths, num_classes):
    return max(r["survivors"] for r in merge_reference(to_passes(images, widths), num_classes, max_det=1 << 20))


def build_cases():
    cases = []
    # candidates in one cell: 0, 1, 63, 64, 65, 128, 129 (the wave's slot boundaries)
    for n, seed in ((0, 10), (1, 10), (63, 11), (64, 10), (65, 12), (128, 10), (129, 13)):
        img = _cell(n, seed)
        cases.append(Case(f"cell{n}", to_passes([img], (50, 50, 50)), 3, max_det=200))
    # an image with no candidate among three; passes of different widths; B = 3
    imgs = [clustered(20, 90, range(5)), [], clustered(21, 40, range(5))]
    cases.append(Case("empty_image_B3_widths", to_passes(imgs, (100, 37, 64, 1)), 5))
    # every pass empty
    cases.append(Case("all_passes_empty", to_passes([[], []], (10, 0, 5)), 4))
    # all candidates in one class (the deepest sequential chain), 5 passes
    cases.append(Case("one_class", to_passes([clustered(33, 300, [0])], (60,) * 5), 1, max_det=100))
    cases.append(Case("full2048", to_passes([_full(35)], (128,) * 16), 2, max_det=2048))
    # 80 classes: class C-1 present, many absent
    cls80 = [0, 3, 17, 42, 63, 78, 79]
    cases.append(Case("classes80", to_passes([clustered(42, 120, cls80), clustered(43, 60, [79, 5])], (100, 100)), 80))
    # exact ties
    cases.append(Case("ties", to_passes([_ties()], (6, 5)), 3))
    # survivors fewer than, equal to and more than max_det
    imgs = [clustered(50, 70, range(4))]
    ns = _survivors(imgs, (40, 40), 4)
    for name, md in (("fewer", ns + 5), ("equal", ns), ("more", ns - 9), ("cut_to_1", 1)):
        cases.append(Case(f"survivors_{name}_max_det", to_passes(imgs, (40, 40)), 4, max_det=md))
    # coordinates near 4000
    cases.append(Case("near4000", to_passes([clustered(60, 80, range(3), origin=3600.0, extent=380.0)], (100,)), 3))
    # boxes narrower than a pixel
    cases.append(Case("subpixel", to_passes([clustered(70, 60, range(2), extent=6.0, size=(0.1, 0.9))], (30, 30)), 2))
    # a -1 count in one pass
    imgs = [clustered(81, 30, range(3)), clustered(81, 30, range(3)), clustered(82, 25, range(3))]
    p = to_passes(imgs, (20, 20))
    p[1][3][1] = -1
    cases.append(Case("nonfinite_flag", p, 3))
    # clustered random
    for seed in (91, 93, 94):
        cases.append(Case(f"clustered{seed}", to_passes([clustered(seed, 150, range(6)), clustered(seed + 100, 110, range(6))],
                                                        (100, 100)), 6))
    return cases


CASES = build_cases()

# hand-derived known answers: ([(box, score)], expected [(candidate, score)] in output order), one class
E = np.exp
KNOWN = [
    ("identical pair", [((0, 0, 9, 9), 0.9), ((0, 0, 9, 9), 0.8)], [(0, 0.9), (1, 0.8 * E(-2.0))]),
    # 10 x 10 boxes shifted by 5: iw = 9 - 5 + 1 = 5, inter = 50, ua = 100 + 100 - 50 = 150, ov = 1/3, weight exp(-(1/9)/0.5)
    ("overlap one third", [((0, 0, 9, 9), 0.9), ((5, 0, 14, 9), 0.8)], [(0, 0.9), (1, 0.8 * E(-2.0 / 9.0))]),
    # iw = 9 - 10 + 1 = 0: not > 0, no decay
    ("touching: no decay", [((0, 0, 9, 9), 0.9), ((10, 0, 19, 9), 0.8)], [(0, 0.9), (1, 0.8)]),
    # iw = 9 - 9.5 + 1 = 0.5 (the +1 convention): inter = 5, ua = 100 + 10.5 * 10 - 5 = 200, ov = 1/40
    ("half a pixel: decays", [((0, 0, 9, 9), 0.9), ((9.5, 0, 19, 9), 0.8)], [(0, 0.9), (1, 0.8 * E(-(1.0 / 1600.0) / 0.5))]),
    # chained: 0.8 decays once (by 0.9), 0.5 twice (by 0.9, then by the decayed 0.8); identical boxes: weight exp(-2) each
    ("chained", [((0, 0, 9, 9), 0.9), ((0, 0, 9, 9), 0.8), ((0, 0, 9, 9), 0.5)],
     [(0, 0.9), (1, 0.8 * E(-2.0)), (2, 0.5 * E(-4.0))]),
    # the fourth, 0.006 * exp(-2) = 0.00081 < 0.001, is removed at its first decay
    ("removed", [((0, 0, 9, 9), 0.9), ((0, 0, 9, 9), 0.8), ((0, 0, 9, 9), 0.5), ((0, 0, 9, 9), 0.006)],
     [(0, 0.9), (1, 0.8 * E(-2.0)), (2, 0.5 * E(-4.0))]),
    # 0.85 decays to 0.115 and the disjoint 0.3 overtakes it
    ("re-ordering", [((0, 0, 9, 9), 0.9), ((0, 0, 9, 9), 0.85), ((50, 50, 59, 59), 0.3)],
     [(0, 0.9), (2, 0.3), (1, 0.85 * E(-2.0))]),
    # never decayed, never removed -- whatever its score
    ("undecayed below the floor", [((0, 0, 9, 9), 0.9), ((50, 50, 59, 59), 0.0005)], [(0, 0.9), (1, 0.0005)]),
]
