"""GPU: TrainingFrameLoader(..., rank, world), the loader side of data-parallel training, on the fixtures of
tests/test_train_loader_gpu.py (tests/golden/train_io, four triplets of three raw sizes).  Each loader is constructed in this
process with no process group, shuffle=False: the order is the file order on every rank.

    python -m pytest tests/test_train_loader_shard_gpu.py -m gpu -q
"""
import os

import numpy as np
import pytest
import torch

import kbnet_amd as kb
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

IO = os.path.join(GOLDEN_DIR, "train_io")
IMAGES = [os.path.join(IO, f"triplet_{i}.png") for i in range(4)]
DEPTHS = [os.path.join(IO, f"depth_{i}.png") for i in range(4)]
KS = [os.path.join(IO, f"k_{i}.npy") for i in range(4)]
SIZES = [(24, 40), (26, 44), (25, 43), (24, 40)]
SHAPE = (16, 24)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need a visible MI355X (run with -m gpu on a GPU box)")
    kb._lib.load()
    return torch.device("cuda:0")


def loader(dev, batch_size, crop_type, **kw):
    return kb.loader.TrainingFrameLoader(IMAGES, DEPTHS, KS, shape=list(SHAPE), random_crop_type=crop_type, batch_size=batch_size,
                                         shuffle=False, device=dev, workers=2, prefetch=2, **kw)


def epoch(ld, seed=None):
    """One epoch's batches on the host: [[image0, image1, image2, depth, k] a batch]."""
    if seed is not None:
        np.random.seed(seed)
    out = []
    for batch in ld:
        assert len(batch) == 5 and all(t.is_cuda and t.dtype == torch.float32 for t in batch)
        out.append([t.cpu() for t in batch])
    return out


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("batch_size", [1, 3, 4])
def test_centre_crop_shards_concatenate_to_the_world_1_batch(dev, batch_size):
    """random_crop_type ['none'] draws nothing: the shards of ranks 0 and 1 are the world-1 batch cut at shard_bounds, bit for bit.
    Batch sizes 1 and 3 end in a batch of one frame: rank 1's shard of it is empty."""
    whole = epoch(loader(dev, batch_size, ["none"]))
    shards = [epoch(loader(dev, batch_size, ["none"], rank=rank, world=2)) for rank in range(2)]
    n_batch = -(-4 // batch_size)
    assert len(whole) == n_batch and all(len(s) == n_batch for s in shards)
    for b in range(n_batch):
        n = whole[b][0].shape[0]
        assert n == loader(dev, batch_size, ["none"], rank=1, world=2).global_batch_size(b) == min(batch_size, 4 - b * batch_size)
        for rank in range(2):
            lo, hi = kb.dist.shard_bounds(n, rank, 2)
            assert all(t.shape[0] == hi - lo for t in shards[rank][b]), (b, rank)
            assert [tuple(t.shape[1:]) for t in shards[rank][b]] == [(3, *SHAPE)] * 3 + [(1, *SHAPE), (3, 3)]
        for i in range(5):
            assert same_bits(torch.cat([shards[0][b][i], shards[1][b][i]], dim=0), whole[b][i]), (b, i)
    assert (batch_size in (1, 3)) == any(t[0].shape[0] == 0 for t in shards[1])


def test_the_crops_are_drawn_for_the_ranks_own_samples(dev):
    """Under np.random.seed(s) a rank draws for its own samples only, in its own order: rank 1 of world 2 at batch size 4 holds
    samples 2 and 3, and its crops are the FIRST two draws after the seed -- for those samples' raw sizes."""
    crop_type = ["horizontal", "vertical"]
    for rank, own in ((0, [0, 1]), (1, [2, 3])):
        [got] = epoch(loader(dev, 4, crop_type, rank=rank, world=2), seed=11)
        np.random.seed(11)
        starts = [kb.loader.draw_crop(*SIZES[i], SHAPE, crop_type) for i in own]
        assert got[0].shape[0] == 2
        for j, (i, (y, x)) in enumerate(zip(own, starts)):
            k = np.load(KS[i]).astype(np.float32)
            k[0, 2] -= x
            k[1, 2] -= y
            assert same_bits(got[4][j], torch.from_numpy(k)), (rank, i)
            raw = torch.from_numpy(kb.loader.decode_png(open(IMAGES[i], "rb").read()).astype(np.float32))      # H x 3 W x 3
            w = SIZES[i][1]
            centre = raw[:, w:2 * w].permute(2, 0, 1)[:, y:y + SHAPE[0], x:x + SHAPE[1]]
            assert same_bits(got[0][j], centre), (rank, i)


@pytest.mark.parametrize("crop_type", [["none"], ["horizontal", "vertical"]], ids=["none", "random"])
def test_rank_0_of_world_1_is_the_loader_without_the_arguments(dev, crop_type):
    plain = epoch(loader(dev, 3, crop_type), seed=5)
    named = epoch(loader(dev, 3, crop_type, rank=0, world=1), seed=5)
    assert len(plain) == len(named) == 2
    for a, b in zip(plain, named):
        assert all(same_bits(x, y) for x, y in zip(a, b))


def test_an_empty_shard_launches_nothing(dev):
    ld = loader(dev, 3, ["none"], rank=1, world=2)      # batches of 3 and 1 frames: rank 1 holds 1 and 0
    batches = list(ld)
    assert [b[0].shape[0] for b in batches] == [1, 0]
    assert ld._serial == 1, "only the batch with a frame went through the decode / copy / unpack pipeline"
    assert all(t.numel() == 0 and t.is_cuda for t in batches[1])
