"""G23: the reference's Pascal VOC scorer (detectron2/evaluation/pascal_voc_evaluation.py: PascalVOCDetectionEvaluator and
voc_eval) on a seeded synthetic VOC tree (run with the reference checkout at make_golden.REF, on the CPU; needs torch).

The reference module is loaded from the checkout with stand-in modules for what it imports (fvcore.common.file_io,
detectron2.data, detectron2.utils.comm, .evaluator) and the alias np.bool = bool; the VOC tree (ImageSets, Annotations) and the
per-class detection files are written into a temporary directory OUTSIDE the repository.  f32 detections go through the
reference's own process() / evaluate() (both years) and, per class and threshold, through voc_eval (both AP forms).  Only
data is written: g23_voceval.npz holds

  inputs    boxes f32 [N,4] XYXY (0-based, as a model gives them), scores f32 [N], classes / image i32 [N] in process()
            order, image_ids [I] (strings, split order), class_names [K], and the objects of the XML files in file order:
            gt_image / gt_classes i32 [NG], gt_difficult u8 [NG], gt_boxes i64 [NG,4] (1-based, as written)
  outputs   rec / prec f64 [T,N]: voc_eval's arrays of class k in columns cls_off[k]:cls_off[k+1] (classes ascending; within a
            class the reference's order, which is unambiguous: see the first condition), cls_off i64 [K+1];
            ap07 / ap12 f64 [K,T] (fractions); res07_* / res12_*: the evaluator's result dicts (bbox [3] = AP, AP50, AP75;
            bbox_AP / bbox_AP50 / bbox_AP75 [K])

Conditions on the inputs are asserted in main(), from the reference's output where it shows them."""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as G  # noqa: E402

I, K, T = 24, 5, 10
CLASS_NAMES = ["aeroplane", "bicycle", "bird", "boat", "bottle"]
# classes 0..2 are scored; 3 has ground truth and no detection; 4 has detections and only difficult ground truth
NO_DET_CLASS, ONLY_DIFFICULT_CLASS = 3, 4
W, H = 500, 375
XML = "<annotation><size><width>{w}</width><height>{h}</height><depth>3</depth></size>{objects}</annotation>"
OBJ = ("<object><name>{name}</name><pose>Unspecified</pose><truncated>0</truncated><difficult>{d}</difficult>"
       "<bndbox><xmin>{b[0]}</xmin><ymin>{b[1]}</ymin><xmax>{b[2]}</xmax><ymax>{b[3]}</ymax></bndbox></object>")


def load_reference(meta):
    """the reference module, with stand-ins for its imports"""
    np.bool = bool      # numpy >= 1.24 dropped the alias the reference uses

    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    class PathManager:
        open = staticmethod(open)

    class DatasetEvaluator:
        pass

    module("fvcore"), module("fvcore.common"), module("fvcore.common.file_io", PathManager=PathManager)
    module("detectron2", __path__=[]), module("detectron2.utils", __path__=[])
    module("detectron2.data", MetadataCatalog=types.SimpleNamespace(get=lambda name: meta[name]))
    comm = module("detectron2.utils.comm", gather=lambda x, dst=0: [x], is_main_process=lambda: True)
    sys.modules["detectron2.utils"].comm = comm
    module("detectron2.evaluation", __path__=[]), module("detectron2.evaluation.evaluator", DatasetEvaluator=DatasetEvaluator)
    path = os.path.join(G.REF, "detectron2", "evaluation", "pascal_voc_evaluation.py")
    spec = importlib.util.spec_from_file_location("detectron2.evaluation.pascal_voc_evaluation", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


class Instances:
    """what process() reads of an Instances"""

    def __init__(self, boxes, scores, classes):
        self.pred_boxes = types.SimpleNamespace(tensor=torch.from_numpy(boxes))
        self.scores, self.pred_classes = torch.from_numpy(scores), torch.from_numpy(classes)

    def to(self, device):
        return self


def overlap(b, g):
    """the VOC overlap of a quantised 1-based detection box with integer ground-truth boxes (for the conditions only)"""
    iw = np.maximum(np.minimum(g[:, 2], b[2]) - np.maximum(g[:, 0], b[0]) + 1.0, 0.0)
    ih = np.maximum(np.minimum(g[:, 3], b[3]) - np.maximum(g[:, 1], b[1]) + 1.0, 0.0)
    return iw * ih / ((b[2] - b[0] + 1.0) * (b[3] - b[1] + 1.0) + (g[:, 2] - g[:, 0] + 1.0) * (g[:, 3] - g[:, 1] + 1.0) - iw * ih)


def make_inputs():
    rng = np.random.default_rng(23)
    gt = []                                            # (image, class, difficult, box)
    for i in range(I):
        if i % 8 == 7:                                 # images without ground truth
            continue
        for _ in range(int(rng.integers(3, 10))):
            k = int(rng.integers(0, K))
            w, h = int(rng.integers(20, 160)), int(rng.integers(20, 160))
            x, y = int(rng.integers(1, W - w)), int(rng.integers(1, H - h))
            d = 1 if k == ONLY_DIFFICULT_CLASS else int(rng.random() < 0.22)
            gt.append((i, k, d, [x, y, x + w, y + h]))
    boxes, classes, image = [], [], []
    for i in range(I):
        if i % 6 == 5:                                 # images without detections
            continue
        mine = [g for g in gt if g[0] == i and g[1] != NO_DET_CLASS]
        for g in mine:
            for _ in range(int(rng.integers(0, 4))):   # 0..3 detections near every ground truth: misses and duplicates
                s = rng.choice([1.0, 3.0, 12.0, 30.0])
                b = np.array(g[3], dtype=np.float64) + rng.normal(0, s, 4)
                b[:2] -= 1.0
                boxes.append(b), classes.append(g[1]), image.append(i)
        for _ in range(int(rng.integers(1, 5))):       # boxes that are near nothing in particular
            k = int(rng.choice([0, 1, 2, ONLY_DIFFICULT_CLASS]))
            x, y = rng.uniform(0, W - 60), rng.uniform(0, H - 60)
            boxes.append(np.array([x, y, x + rng.uniform(10, 60), y + rng.uniform(10, 60)])), classes.append(k), image.append(i)
    n = len(boxes)
    boxes = np.array(boxes, dtype=np.float64)
    boxes[:, 2:] = np.maximum(boxes[:, 2:], boxes[:, :2] + 2.0)
    q = rng.random(n) < 0.3                             # many coordinates on quarters: x.25 / x.75 are exact ties of "%.1f"
    boxes[q] = np.round(boxes[q] * 4.0) / 4.0
    boxes = boxes.astype(np.float32)
    # scores: distinct thousandths (a permutation of 1 .. 999 needs n <= 999), moved by less than half a thousandth
    assert n <= 999, n
    scores = (rng.permutation(999)[:n] + 1) / 1000.0 + rng.uniform(-0.0004, 0.0004, n)
    return gt, boxes, scores.astype(np.float32), np.array(classes, dtype=np.int32), np.array(image, dtype=np.int32)


def main():
    gt, boxes, scores, classes, image = make_inputs()
    ids = ["%06d" % (i + 1) for i in range(I)]
    N = len(scores)
    with tempfile.TemporaryDirectory(prefix="g23_voc_") as tmp:
        os.makedirs(os.path.join(tmp, "ImageSets", "Main")), os.makedirs(os.path.join(tmp, "Annotations"))
        with open(os.path.join(tmp, "ImageSets", "Main", "test.txt"), "w") as f:
            f.write("".join(i + "\n" for i in ids))
        for i, fileid in enumerate(ids):
            objects = "".join(OBJ.format(name=CLASS_NAMES[g[1]], d=g[2], b=g[3]) for g in gt if g[0] == i)
            with open(os.path.join(tmp, "Annotations", fileid + ".xml"), "w") as f:
                f.write(XML.format(w=W, h=H, objects=objects))
        meta = {f"g23_{year}": types.SimpleNamespace(dirname=tmp, split="test", thing_classes=CLASS_NAMES, year=year)
                for year in (2007, 2012)}
        ref = load_reference(meta)
        results, evaluator = {}, None
        for year in (2007, 2012):
            evaluator = ref.PascalVOCDetectionEvaluator(f"g23_{year}")
            evaluator.reset()
            for i in range(I):       # one process() call per image that has detections, in input order
                sel = np.flatnonzero(image == i)
                if sel.size:
                    assert np.all(np.diff(sel) == 1)
                    evaluator.process([{"image_id": ids[i]}], [{"instances": Instances(boxes[sel], scores[sel], classes[sel])}])
            results[year] = evaluator.evaluate()
        # voc_eval per class and threshold over the files the evaluator would write
        det_dir = os.path.join(tmp, "dets")
        os.makedirs(det_dir)
        template = os.path.join(det_dir, "{}.txt")
        for k, name in enumerate(CLASS_NAMES):
            with open(template.format(name), "w") as f:
                f.write("\n".join(evaluator._predictions.get(k, [""])))
        counts = np.bincount(classes, minlength=K)
        cls_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        rec, prec = np.zeros((T, N)), np.zeros((T, N))
        ap07, ap12 = np.zeros((K, T)), np.zeros((K, T))
        anno = os.path.join(tmp, "Annotations", "{}.xml")
        imageset = os.path.join(tmp, "ImageSets", "Main", "test.txt")
        with np.errstate(invalid="ignore", divide="ignore"):
            for k, name in enumerate(CLASS_NAMES):
                for t, thresh in enumerate(range(50, 100, 5)):
                    r, p, a07 = ref.voc_eval(template, anno, imageset, name, ovthresh=thresh / 100.0, use_07_metric=True)
                    r2, p2, a12 = ref.voc_eval(template, anno, imageset, name, ovthresh=thresh / 100.0, use_07_metric=False)
                    assert np.array_equal(r, r2, equal_nan=True) and np.array_equal(p, p2) and len(r) == counts[k]
                    rec[t, cls_off[k]:cls_off[k + 1]], prec[t, cls_off[k]:cls_off[k + 1]] = r, p
                    ap07[k, t], ap12[k, t] = a07, a12

    # ---- conditions
    qs = np.array([float(f"{s:.3f}") for s in scores.tolist()])
    for k in range(K):       # quantised scores distinct within each class: the reference's unstable sort cannot matter
        assert len(set(qs[classes == k])) == counts[k]
    gt_cls, gt_diff = np.array([g[1] for g in gt]), np.array([g[2] for g in gt])
    share = gt_diff[gt_cls != ONLY_DIFFICULT_CLASS].mean()
    assert 0.1 < share < 0.4, share                                   # a share of difficult ground truths
    assert counts[NO_DET_CLASS] == 0 and (gt_cls == NO_DET_CLASS).any()                 # a class without detections
    assert counts[ONLY_DIFFICULT_CLASS] > 0 and gt_diff[gt_cls == ONLY_DIFFICULT_CLASS].all()
    assert np.all(ap07[NO_DET_CLASS] == 0) and np.all(ap12[NO_DET_CLASS] == 0)
    assert np.all(ap07[ONLY_DIFFICULT_CLASS] == 0) and np.all(np.isnan(ap12[ONLY_DIFFICULT_CLASS]))    # the NaN case
    gt_images, det_images = {g[0] for g in gt}, set(image.tolist())
    assert len(gt_images) < I and len(det_images) < I and (det_images - gt_images) and (gt_images - det_images)
    for k in (0, 1, 2):      # the scored classes: APs inside 0.05 .. 0.95 at the loosest threshold, for both forms
        assert 0.05 < ap07[k, 0] < 0.95 and 0.05 < ap12[k, 0] < 0.95, (k, ap07[k, 0], ap12[k, 0])
    # from the reference's output at 0.5: tp + fp at the end of a class is tp / prec; what is missing of the class's detections
    # matched a difficult ground truth
    neither = 0
    for k in (0, 1, 2):
        last = cls_off[k + 1] - 1
        npos = int(((gt_cls == k) & (gt_diff == 0)).sum())
        tp = int(np.rint(rec[0, last] * npos))
        assert tp > 0
        neither += counts[k] - int(np.rint(tp / prec[0, last]))
    assert neither >= 1, neither                                       # detections whose best match is difficult
    # duplicates on one ground truth (by construction, with the rule's own overlap): two detections of an image and class whose
    # best match above 0.5 is the same non-difficult ground truth
    bq = boxes.copy()
    bq[:, :2] = bq[:, :2] + np.float32(1)
    bq = np.array([[float(f"{c:.1f}") for c in row] for row in bq.tolist()])
    dup = 0
    for i in range(I):
        for k in (0, 1, 2):
            g = [x for x in gt if x[0] == i and x[1] == k]
            if not g:
                continue
            gb, hits = np.array([x[3] for x in g], dtype=np.float64), {}
            for o in np.flatnonzero((image == i) & (classes == k)):
                ov = overlap(bq[o], gb)
                j = int(np.argmax(ov))
                if ov[j] > 0.5 and not g[j][2]:
                    hits[j] = hits.get(j, 0) + 1
            dup += sum(1 for v in hits.values() if v > 1)
    assert dup >= 3, dup

    def pack(res):
        return {"bbox": np.array([res["bbox"][m] for m in ("AP", "AP50", "AP75")], dtype=np.float64),
                **{key: np.array([res[key][n] for n in CLASS_NAMES], dtype=np.float64) for key in ("bbox_AP", "bbox_AP50", "bbox_AP75")}}

    out = {"boxes": boxes, "scores": scores, "classes": classes, "image": image, "image_ids": np.array(ids),
           "class_names": np.array(CLASS_NAMES), "gt_image": np.array([g[0] for g in gt], dtype=np.int32),
           "gt_classes": gt_cls.astype(np.int32), "gt_difficult": gt_diff.astype(np.uint8),
           "gt_boxes": np.array([g[3] for g in gt], dtype=np.int64), "cls_off": cls_off, "rec": rec, "prec": prec,
           "ap07": ap07, "ap12": ap12}
    for year in (2007, 2012):
        assert list(results[year]) == ["bbox", "bbox_AP", "bbox_AP50", "bbox_AP75"]
        out.update({f"res{year % 100:02d}_{key}": v for key, v in pack(results[year]).items()})
    path = os.path.join(HERE, "g23_voceval.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: N={N} detections, NG={len(gt)} ground truths ({int(gt_diff.sum())} difficult), "
          f"{neither} on difficult, {dup} duplicated; AP50 07 {ap07[:, 0].round(3)} 12 {ap12[:, 0].round(3)}")


if __name__ == "__main__":
    main()
