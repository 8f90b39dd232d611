"""Training and inference samplers and minimal batched loaders (reference: data/samplers/distributed_sampler.py:12-55
TrainingSampler, :57-170 RepeatFactorTrainingSampler, :172-199 InferenceSampler, data/build.py:270-355 build_detection_train_loader / per-GPU batch size, :358-403
build_detection_test_loader).  The GPU path takes `list[dict]` batches of unequal image sizes as they come."""
import itertools
import math
from collections import defaultdict

import torch

from .catalog import DatasetCatalog
from .dataset_mapper import TrafficLightDatasetMapper


class TrainingSampler:
    """infinite stream of indices: every rank draws the same seeded permutations and takes elements rank, rank+W, ..."""

    def __init__(self, size, shuffle=True, seed=0, rank=0, world_size=1):
        assert size > 0
        self._size, self._shuffle, self._seed, self._rank, self._world = size, shuffle, int(seed), rank, world_size

    def __iter__(self):
        yield from itertools.islice(self._infinite_indices(), self._rank, None, self._world)

    def _infinite_indices(self):
        g = torch.Generator()
        g.manual_seed(self._seed)
        while True:
            if self._shuffle:
                yield from torch.randperm(self._size, generator=g).tolist()
            else:
                yield from range(self._size)


def repeat_factors_from_category_frequency(dataset_dicts, repeat_thresh):
    """f32 [len(dataset_dicts)]: the repeat factor of every image from the frequency of its rarest class (LVIS paper, appendix
    B.2; reference :86-130).  f(c) = share of the images that hold class c; r(c) = max(1, sqrt(repeat_thresh / f(c))); r(I) =
    the largest r(c) over the image's classes.  An image without annotations gets 1.0: the reference raises there (max of an
    empty set), which it can only meet with DATALOADER.FILTER_EMPTY_ANNOTATIONS off; repeating such an image never is this
    project's choice."""
    category_freq = defaultdict(int)
    for d in dataset_dicts:
        for c in {a["category_id"] for a in d.get("annotations", [])}:
            category_freq[c] += 1
    num_images = len(dataset_dicts)
    category_rep = {c: max(1.0, math.sqrt(repeat_thresh / (n / num_images))) for c, n in category_freq.items()}
    return torch.tensor([max({category_rep[a["category_id"]] for a in d.get("annotations", [])}, default=1.0)
                         for d in dataset_dicts], dtype=torch.float32)


class RepeatFactorTrainingSampler:
    """TrainingSampler in which index i appears repeat_factors[i] times per epoch on average (reference :57-170).  Per epoch,
    on the one seeded generator: `torch.rand(n)` rounds every fractional part up or down (stochastic rounding), the indices
    are repeated, and with `shuffle` a `randperm` over the repeated list orders them.  Every rank draws the same stream and takes
    elements rank, rank+W, ...; factors all 1 give TrainingSampler's multiset per epoch (not its order: one more draw)."""

    def __init__(self, repeat_factors, shuffle=True, seed=0, rank=0, world_size=1):
        repeat_factors = torch.as_tensor(repeat_factors, dtype=torch.float32)
        assert repeat_factors.ndim == 1 and repeat_factors.numel() > 0
        self._shuffle, self._seed, self._rank, self._world = shuffle, int(seed), rank, world_size
        self._int_part = torch.trunc(repeat_factors)
        self._frac_part = repeat_factors - self._int_part

    def __iter__(self):
        yield from itertools.islice(self._infinite_indices(), self._rank, None, self._world)

    def _epoch_indices(self, g):
        rands = torch.rand(len(self._frac_part), generator=g)
        reps = (self._int_part + (rands < self._frac_part).float()).to(torch.int64)
        return torch.repeat_interleave(torch.arange(len(reps), dtype=torch.int64), reps)

    def _infinite_indices(self):
        g = torch.Generator()
        g.manual_seed(self._seed)
        while True:
            indices = self._epoch_indices(g)
            if self._shuffle:
                indices = indices[torch.randperm(len(indices), generator=g)]
            yield from indices.tolist()


class InferenceSampler:
    """every index once, in order: rank r of W takes r, r + W, r + 2W, ... (the reference hands each rank one contiguous
    shard; a strided split keeps the ranks within one image of each other for any dataset size)"""

    def __init__(self, size, rank=0, world_size=1):
        assert size > 0 and 0 <= rank < world_size
        self._indices = range(rank, size, world_size)

    def __iter__(self):
        yield from self._indices

    def __len__(self):
        return len(self._indices)


def filter_images_with_only_crowd_annotations(dataset_dicts):
    """data/build.py:41-68"""
    def valid(anns):
        return any(a.get("iscrowd", 0) == 0 for a in anns)
    return [d for d in dataset_dicts if valid(d.get("annotations", []))]


class _MapDataset(torch.utils.data.Dataset):
    def __init__(self, dicts, mapper):
        self.dicts, self.mapper = dicts, mapper

    def __len__(self):
        return len(self.dicts)

    def __getitem__(self, i):
        return self.mapper(self.dicts[i])


def _trivial_batch_collator(batch):
    return batch


def _worker_init_reset_seed(worker_id):
    """every worker process gets its own numpy / python RNG stream (data/build.py worker_init_reset_seed)"""
    import random

    import numpy as np
    seed = (torch.initial_seed() + worker_id) % 2 ** 31
    np.random.seed(seed)
    random.seed(seed)


def build_detection_train_loader(cfg, mapper=None, rank=0, world_size=1, seed=0, num_workers=None):
    """iterator over lists of `IMS_PER_BATCH // world_size` mapped samples, forever (data/build.py:300-355): a
    torch DataLoader with worker PROCESSES (the mapper is numpy / PIL code under the GIL), infinite TrainingSampler, batches
    kept as lists -- images in a batch have different sizes"""
    names = cfg.DATASETS.TRAIN
    dicts = list(itertools.chain.from_iterable(DatasetCatalog.get(n) for n in names))
    if cfg.DATALOADER.FILTER_EMPTY_ANNOTATIONS and dicts and "annotations" in dicts[0]:
        dicts = filter_images_with_only_crowd_annotations(dicts)
    assert len(dicts), "no training images"
    total = cfg.SOLVER.IMS_PER_BATCH
    assert total % world_size == 0, f"IMS_PER_BATCH ({total}) must be divisible by the number of workers ({world_size})"
    per_gpu = total // world_size
    mapper = mapper if mapper is not None else TrafficLightDatasetMapper(cfg, True)
    name = cfg.DATALOADER.SAMPLER_TRAIN
    if name == "TrainingSampler":
        sampler = TrainingSampler(len(dicts), seed=seed, rank=rank, world_size=world_size)
    elif name == "RepeatFactorTrainingSampler":
        factors = repeat_factors_from_category_frequency(dicts, cfg.DATALOADER.REPEAT_THRESHOLD)
        sampler = RepeatFactorTrainingSampler(factors, seed=seed, rank=rank, world_size=world_size)
    else:
        raise ValueError("Unknown training sampler: {}".format(name))
    workers = cfg.DATALOADER.NUM_WORKERS if num_workers is None else num_workers
    batch_sampler = torch.utils.data.BatchSampler(sampler, per_gpu, drop_last=True)
    loader = torch.utils.data.DataLoader(_MapDataset(dicts, mapper), batch_sampler=batch_sampler, num_workers=workers,
                                         collate_fn=_trivial_batch_collator,
                                         worker_init_fn=_worker_init_reset_seed if workers > 0 else None)
    return iter(loader)


def build_detection_test_loader(cfg, dataset_name, mapper=None, rank=0, world_size=1, num_workers=None):
    """loader over `dataset_name` for inference (data/build.py:358-403): every record once and in order (InferenceSampler),
    nothing filtered, lists of TEST.BATCH_SIZE mapped samples (the last one shorter).  The default mapper is
    TrafficLightDatasetMapper(cfg, False): with INPUT.DEVICE_RESIZE its records carry the raw image and the model resizes
    the batch on the device; with INPUT.AFFINE.TEST_MODE they are CenterNet's warped test input (fix_res: one size for the
    whole set, so every full batch replays one captured engine)."""
    dicts = list(DatasetCatalog.get(dataset_name))
    assert len(dicts), f"dataset '{dataset_name}' is empty"
    mapper = mapper if mapper is not None else TrafficLightDatasetMapper(cfg, False)
    sampler = InferenceSampler(len(dicts), rank=rank, world_size=world_size)
    workers = cfg.DATALOADER.NUM_WORKERS if num_workers is None else num_workers
    batch_sampler = torch.utils.data.BatchSampler(sampler, int(cfg.TEST.BATCH_SIZE), drop_last=False)
    return torch.utils.data.DataLoader(_MapDataset(dicts, mapper), batch_sampler=batch_sampler, num_workers=workers,
                                       collate_fn=_trivial_batch_collator)
