"""RepeatFactorTrainingSampler against the reference's own (fixture G24, tests/golden/make_g24.py): the repeat factors at two
thresholds and the first three epochs' index streams for two seeds and two ranks, exactly; and DATALOADER.SAMPLER_TRAIN in
`build_detection_train_loader`: honoured, refused by name, and the default path's index stream unchanged."""
import itertools
import os

import numpy as np
import pytest
import torch

from detectron2_centernet_amd.config import get_cfg
from detectron2_centernet_amd.data import (DatasetCatalog, MetadataCatalog, RepeatFactorTrainingSampler, TrainingSampler,
                                           build_detection_train_loader, repeat_factors_from_category_frequency)

HERE = os.path.dirname(os.path.abspath(__file__))
G24 = os.path.join(HERE, "golden", "g24_repeat_factor.npz")


@pytest.fixture(scope="module")
def g24():
    g = np.load(G24)
    dicts = [{"image_id": i, "annotations": []} for i in range(int(g["num_images"]))]
    for i, c in zip(g["ann_image"].tolist(), g["ann_class"].tolist()):
        dicts[i]["annotations"].append({"category_id": c})
    return g, dicts


def test_repeat_factors_equal_the_reference(g24):
    g, dicts = g24
    for t, want in zip(g["thresholds"].tolist(), g["factors"]):
        got = repeat_factors_from_category_frequency(dicts, t)
        assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want), t
    assert (g["factors"] > 1).any() and (g["factors"] == 1).any()


def test_image_without_annotations_gets_one(g24):
    """the reference raises there (max of an empty set); it can only occur with FILTER_EMPTY_ANNOTATIONS off"""
    g, dicts = g24
    got = repeat_factors_from_category_frequency(dicts + [{"image_id": -1, "annotations": []}, {"image_id": -2}], 0.6)
    assert got[-2:].tolist() == [1.0, 1.0] and got.shape == (len(dicts) + 2,)
    # the two empty images count in the number of images: every class is rarer by 62 / 60, so no factor is smaller than before
    assert torch.all(got[:-2] >= torch.as_tensor(g["factors"][1]))


def test_index_streams_equal_the_reference(g24):
    g, _ = g24
    factors, world = torch.as_tensor(g["factors"][0]), int(g["world"])
    for s, seed in enumerate(g["seeds"].tolist()):
        total = int(g["epoch_len"][s].sum())
        for rank in range(world):
            want = g[f"stream_s{seed}_r{rank}"].tolist()
            assert len(want) == len(range(rank, total, world))
            sampler = RepeatFactorTrainingSampler(factors, seed=seed, rank=rank, world_size=world)
            assert list(itertools.islice(iter(sampler), len(want))) == want, (seed, rank)
        # the ranks' streams interleave to one stream whose epochs are multisets with int or int + 1 copies of every index
        whole = list(itertools.islice(iter(RepeatFactorTrainingSampler(factors, seed=seed)), total))
        assert whole[0::world] == g[f"stream_s{seed}_r0"].tolist() and whole[1::world] == g[f"stream_s{seed}_r1"].tolist()
        start = 0
        for n in g["epoch_len"][s].tolist():
            count = np.bincount(whole[start:start + n], minlength=len(factors))
            assert np.all((count == np.floor(g["factors"][0])) | (count == np.floor(g["factors"][0]) + 1))
            start += n
    assert g["stream_s0_r0"].tolist() != g["stream_s7_r0"].tolist()


def test_without_shuffle_the_indices_ascend_within_an_epoch():
    s = RepeatFactorTrainingSampler(torch.tensor([1.0, 3.0, 2.0]), shuffle=False, seed=3)
    assert list(itertools.islice(iter(s), 12)) == [0, 1, 1, 1, 2, 2] * 2


def test_factors_all_one_give_the_training_samplers_multiset_per_epoch():
    n = 17
    s = iter(RepeatFactorTrainingSampler(torch.ones(n), seed=5))
    t = iter(TrainingSampler(n, seed=5))
    for _ in range(3):
        a, b = list(itertools.islice(s, n)), list(itertools.islice(t, n))
        assert sorted(a) == sorted(b) == list(range(n))


# ---- DATALOADER.SAMPLER_TRAIN
@pytest.fixture
def tail_set(g24):
    _, dicts = g24
    name = f"repeat_factor_host_{os.getpid()}"
    DatasetCatalog.register(name, lambda: dicts)
    MetadataCatalog.get(name).set(thing_classes=[f"c{k}" for k in range(9)])
    yield name, dicts
    DatasetCatalog.remove(name)
    MetadataCatalog.remove(name)


def _cfg(name, sampler, threshold=None):
    cfg = get_cfg()
    cfg.DATASETS.TRAIN = (name,)
    cfg.SOLVER.IMS_PER_BATCH = 4
    cfg.DATALOADER.SAMPLER_TRAIN = sampler
    if threshold is not None:
        cfg.DATALOADER.REPEAT_THRESHOLD = threshold
    return cfg


def _stream(cfg, n, **kw):
    """the image ids of the first n batches: the mapper hands the record's id through"""
    loader = build_detection_train_loader(cfg, mapper=lambda d: d["image_id"], num_workers=0, **kw)
    return [i for batch in itertools.islice(loader, n) for i in batch]


def test_default_sampler_path_is_unchanged(tail_set):
    name, dicts = tail_set
    assert get_cfg().DATALOADER.SAMPLER_TRAIN == "TrainingSampler" and get_cfg().DATALOADER.REPEAT_THRESHOLD == 0.0
    got = _stream(_cfg(name, "TrainingSampler"), 40, seed=11)
    assert got == list(itertools.islice(iter(TrainingSampler(len(dicts), seed=11)), 160))
    g = torch.Generator()
    g.manual_seed(11)
    assert got[:len(dicts)] == torch.randperm(len(dicts), generator=g).tolist()       # the stream itself, not the class
    both = [_stream(_cfg(name, "TrainingSampler"), 10, seed=11, rank=r, world_size=2) for r in (0, 1)]
    assert both[0] == got[0:40:2] and both[1] == got[1:40:2]


def test_repeat_factor_sampler_is_honoured(tail_set, g24):
    name, dicts = tail_set
    g, _ = g24
    t = float(g["thresholds"][0])
    got = _stream(_cfg(name, "RepeatFactorTrainingSampler", t), 30, seed=7, rank=1, world_size=2)
    assert len(got) == 60 and got == g["stream_s7_r1"][:60].tolist()
    # the threshold is read: at 0 every factor is 1 and an epoch holds every image once
    once = _stream(_cfg(name, "RepeatFactorTrainingSampler", 0.0), 15, seed=7)
    assert sorted(once) == list(range(len(dicts)))


def test_unknown_sampler_is_refused_by_name(tail_set):
    with pytest.raises(ValueError, match="Unknown training sampler: WeightedSampler"):
        build_detection_train_loader(_cfg(tail_set[0], "WeightedSampler"), mapper=lambda d: d, num_workers=0)
