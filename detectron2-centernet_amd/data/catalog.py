"""Dataset / metadata catalogs (detectron2/data/catalog.py:13-236) plus a synthetic COCO-shaped source.

`CenterNet.__init__` requires `DatasetCatalog.get(cfg.DATASETS.TRAIN[0])` and takes the class count from
`MetadataCatalog.get(...).thing_classes` (centernet.py:59-63).  The reference yaml names `bulb_train`, a private
dataset (detectron2/data/datasets/builtin.py:251-279) that is not available; `register_synthetic` registers
any such name with generated 512x512 samples so the yaml loads unchanged."""
import types

import torch


class _DatasetCatalog:
    def __init__(self):
        self._registered = {}

    def register(self, name, func):
        assert callable(func), "You must register a function with `DatasetCatalog.register`!"
        assert name not in self._registered, f"Dataset '{name}' is already registered!"
        self._registered[name] = func

    def get(self, name):
        try:
            f = self._registered[name]
        except KeyError:
            raise KeyError(f"Dataset '{name}' is not registered! Available datasets are: {', '.join(self._registered)}")
        return f()

    def list(self):
        return list(self._registered.keys())

    def remove(self, name):
        self._registered.pop(name)

    def clear(self):
        self._registered.clear()

    def __contains__(self, name):
        return name in self._registered


class Metadata(types.SimpleNamespace):
    name: str = "N/A"

    def as_dict(self):
        return dict(self.__dict__)

    def set(self, **kwargs):
        for k, v in kwargs.items():
            setattr(self, k, v)
        return self

    def get(self, key, default=None):
        return getattr(self, key, default)


class _MetadataCatalog:
    def __init__(self):
        self._name_to_meta = {}

    def get(self, name):
        assert len(name)
        if name not in self._name_to_meta:
            self._name_to_meta[name] = Metadata(name=name)
        return self._name_to_meta[name]

    def list(self):
        return list(self._name_to_meta.keys())

    def remove(self, name):
        self._name_to_meta.pop(name)


DatasetCatalog = _DatasetCatalog()
MetadataCatalog = _MetadataCatalog()


def synthetic_sample(index, size=512, num_classes=80, max_boxes=32, seed=1234):
    """One COCO-shaped synthetic sample: uint8 image, 1..max_boxes boxes with
    w,h ~ U[8,256] inside the image, class ~ U{0..C-1}.  Deterministic in (seed, index)."""
    g = torch.Generator().manual_seed(seed * 100003 + index)
    image = torch.randint(0, 256, (3, size, size), generator=g, dtype=torch.uint8)
    n = int(torch.randint(1, max_boxes + 1, (1,), generator=g))
    wh = torch.rand(n, 2, generator=g) * min(248, size - 8) + 8
    ctr = torch.rand(n, 2, generator=g) * (size - wh) + wh / 2
    boxes = torch.cat([ctr - wh / 2, ctr + wh / 2], dim=1)
    classes = torch.randint(0, num_classes, (n,), generator=g)
    return {"image": image, "boxes": boxes, "classes": classes, "height": size, "width": size}


def register_synthetic(name, num_classes=80, length=1000, size=512):
    """Registers `name` (e.g. the yaml's "bulb_train") as a synthetic COCO-shaped dataset."""
    if name in DatasetCatalog:
        return

    def _load():
        return [{"file_name": f"synthetic://{name}/{i}", "image_id": i, "height": size, "width": size}
                for i in range(length)]

    DatasetCatalog.register(name, _load)
    MetadataCatalog.get(name).set(thing_classes=[f"class_{i}" for i in range(num_classes)], synthetic=True)


def register_synthetic_files(name, root, length=64, size=512, num_classes=80, max_boxes=8, replace=False):
    """Registers `name` as a synthetic dataset a loader can read: the images of `synthetic_sample` are written as PNG files
    under `root` (once; PNG is lossless, so a mapper decodes the sample's bytes) and the records carry their boxes as
    annotations -- what `tools/train_net.py` trains on when the config's datasets are not registered, and what the trainer's
    tests use.  A name that is registered already is an error unless `replace` is set."""
    import os

    from PIL import Image

    from ..structures import BoxMode
    if name in DatasetCatalog and not replace:
        raise ValueError(f"Dataset '{name}' is already registered (replace=True replaces the registration)")
    os.makedirs(root, exist_ok=True)
    records = []
    for i in range(length):
        s = synthetic_sample(i, size=size, num_classes=num_classes, max_boxes=max_boxes)
        path = os.path.join(root, f"{name}_{size}_{i:06d}.png")
        if not os.path.exists(path):
            Image.fromarray(s["image"].permute(1, 2, 0).contiguous().numpy()).save(path)
        records.append({"file_name": path, "image_id": i, "height": size, "width": size, "annotations": [
            {"bbox": b.tolist(), "bbox_mode": BoxMode.XYXY_ABS, "category_id": int(c), "iscrowd": 0}
            for b, c in zip(s["boxes"], s["classes"])]})
    if name in DatasetCatalog:
        DatasetCatalog.remove(name)
    DatasetCatalog.register(name, lambda: records)
    MetadataCatalog.get(name).set(thing_classes=[f"class_{i}" for i in range(num_classes)], synthetic=True)
    return records
