"""G24: the reference's RepeatFactorTrainingSampler (detectron2/data/samplers/distributed_sampler.py:57-170) on a seeded
long-tailed set (run with the reference checkout at make_golden.REF, on the CPU; needs torch).

The reference module is loaded from the checkout with a stand-in for the one module it imports (detectron2.utils.comm: rank,
world size and the shared seed are set from here).  Only data is written: g24_repeat_factor.npz holds

  inputs    num_images, and the annotations of the set as two flat arrays ann_image / ann_class i32 [M] (every image has one)
            thresholds f64 [2], seeds i64 [2], world = 2
  outputs   factors f32 [2, num_images]: repeat_factors_from_category_frequency at the two thresholds
            epoch_len i64 [2, 3]: the lengths of the first three epochs of thresholds[0]'s factors, per seed
            stream_s<seed>_r<rank> i64: what rank `rank` of `world` draws of those three epochs (elements rank, rank + world, ...
            of the first sum(epoch_len) indices), with shuffle"""
import importlib.util
import itertools
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as G  # noqa: E402

NUM_IMAGES, K = 60, 9
THRESHOLDS = (0.2, 0.6)
SEEDS = (0, 7)
WORLD, EPOCHS = 2, 3


def load_reference(state):
    """the reference module, with a stand-in for detectron2.utils.comm that reads rank and world size from `state`"""
    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    module("detectron2", __path__=[])
    utils = module("detectron2.utils", __path__=[])
    utils.comm = module("detectron2.utils.comm", get_rank=lambda: state["rank"], get_world_size=lambda: state["world"],
                        shared_random_seed=lambda: 0)
    path = os.path.join(G.REF, "detectron2", "data", "samplers", "distributed_sampler.py")
    spec = importlib.util.spec_from_file_location("detectron2.data.samplers.distributed_sampler", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def make_inputs():
    """a long tail: class k is drawn with weight 1 / (1 + k)^1.5; one to four annotations per image"""
    rng = np.random.default_rng(24)
    w = 1.0 / (1.0 + np.arange(K)) ** 1.5
    w /= w.sum()
    ann_image, ann_class = [], []
    for i in range(NUM_IMAGES):
        for c in rng.choice(K, int(rng.integers(1, 5)), p=w):
            ann_image.append(i), ann_class.append(int(c))
    return np.array(ann_image, dtype=np.int32), np.array(ann_class, dtype=np.int32)


def dataset_dicts(ann_image, ann_class, num_images):
    dicts = [{"annotations": []} for _ in range(num_images)]
    for i, c in zip(ann_image.tolist(), ann_class.tolist()):
        dicts[i]["annotations"].append({"category_id": c})
    return dicts


def main():
    state = {"rank": 0, "world": 1}
    ref = load_reference(state)
    ann_image, ann_class = make_inputs()
    dicts = dataset_dicts(ann_image, ann_class, NUM_IMAGES)
    Sampler = ref.RepeatFactorTrainingSampler
    factors = [Sampler.repeat_factors_from_category_frequency(dicts, t) for t in THRESHOLDS]
    out = {"num_images": np.int64(NUM_IMAGES), "ann_image": ann_image, "ann_class": ann_class,
           "thresholds": np.array(THRESHOLDS, dtype=np.float64), "seeds": np.array(SEEDS, dtype=np.int64), "world": np.int64(WORLD),
           "factors": torch.stack(factors).numpy()}
    epoch_len = np.zeros((len(SEEDS), EPOCHS), dtype=np.int64)
    for s, seed in enumerate(SEEDS):
        probe = Sampler(factors[0], shuffle=True, seed=seed)
        g = torch.Generator()
        g.manual_seed(seed)
        for e in range(EPOCHS):       # the generator's use per epoch: the rounding draw, then the permutation
            epoch_len[s, e] = len(probe._get_epoch_indices(g))
            torch.randperm(int(epoch_len[s, e]), generator=g)
        total = int(epoch_len[s].sum())
        for rank in range(WORLD):
            state.update(rank=rank, world=WORLD)
            sampler = Sampler(factors[0], shuffle=True, seed=seed)
            n = len(range(rank, total, WORLD))
            out[f"stream_s{seed}_r{rank}"] = np.array([int(v) for v in itertools.islice(iter(sampler), n)], dtype=np.int64)
        state.update(rank=0, world=1)
    out["epoch_len"] = epoch_len
    # ---- conditions
    f = out["factors"]
    assert f.dtype == np.float32 and f.shape == (2, NUM_IMAGES)
    for row in f:      # factors of 1, fractional factors, and factors of 2 and more
        assert (row == 1).any() and ((row > 1) & (row % 1 != 0)).sum() >= 5 and (row >= 2).any(), row
    assert len(set(epoch_len.reshape(-1).tolist())) > 1          # the stochastic rounding shows: epochs of different lengths
    assert epoch_len.min() > NUM_IMAGES
    path = os.path.join(HERE, "g24_repeat_factor.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: factors {f.min():.3f} .. {f.max():.3f}, epoch lengths {epoch_len.tolist()}")


if __name__ == "__main__":
    main()
