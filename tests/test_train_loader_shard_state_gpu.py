"""GPU, one process: the state of a sharded TrainingFrameLoader (world 2, crops="global") is the GLOBAL one -- equal dicts on both
ranks -- and a fresh pair of loaders given rank 0's state continues the epoch, and runs the next, bit for bit as the uninterrupted
pair.

Rank 0 and rank 1 each get a loader of their own in this process, no process group, each run under the same np.random.seed /
torch.manual_seed (the way tests/test_augment_shard_gpu.py builds its ranks).  The samples are the two triplets of
tests/golden/train_io with room for a free 24 x 40 crop (26 x 44 and 25 x 43), batch 2: nine of them -- five global batches, the
last of one frame, of which rank 1's shard is empty -- at the (prefetch, batches taken) pairs of tests/test_train_resumable_gpu.py,
and three of them: two global batches, the state taken with the one-frame batch in flight.  Between two batches the thread draws
from np.random, as Transforms.draw does.

Proof of power: with the stored plans dropped and drawn again from the restored generator, at least one batch differs.

    python -m pytest tests/test_train_loader_shard_state_gpu.py -m gpu -q
"""
import os

import numpy as np
import pytest
import torch

import kbnet_amd as kb
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

KbnError = kb._lib.KbnError
IO = os.path.join(GOLDEN_DIR, "train_io")
ORDER = [1, 2, 2, 1, 2, 1, 1, 1, 2]
WORLD = 2
CASES = [(9, 4, 1), (9, 4, 3), (9, 2, 2), (9, 1, 4), (9, 8, 2), (3, 4, 1), (3, 1, 1)]      # samples, prefetch, batches taken


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    kb._lib.load()
    return torch.device("cuda:0")


def _seed(value):
    torch.manual_seed(value)
    np.random.seed(value)


def _loader(dev, rank, n_sample, **more):
    paths = [[os.path.join(IO, pattern.format(i)) for i in ORDER[:n_sample]] for pattern in ("triplet_{}.png", "depth_{}.png", "k_{}.npy")]
    arguments = dict(shape=(24, 40), random_crop_type=["horizontal", "vertical"], batch_size=2, shuffle=True, device=dev, workers=2,
                     rank=rank, world=WORLD, crops="global")
    arguments.update(more)
    return kb.loader.TrainingFrameLoader(*paths, **arguments)


def _take(loader, epochs, stop=None):
    """The batches of `epochs` epochs, cloned; with `stop`, those of the first epoch's first `stop` batches only."""
    out = []
    for epoch in range(epochs):
        for b, batch in enumerate(loader):
            out.append([t.clone() for t in batch])
            np.random.rand(3)
            if stop is not None and b + 1 == stop:
                return out
    return out


def _same_batches(got, want):
    return len(got) == len(want) and all(len(a) == len(b) and all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))
                                         for a, b in zip(got, want))


def _same_generators(a, b):
    return a[0][0] == b[0][0] and np.array_equal(a[0][1], b[0][1]) and a[0][2:] == b[0][2:] and torch.equal(a[1], b[1])


def _interrupted(dev, n_sample, prefetch, taken, tmp_path, harm=None):
    """-> per rank (the uninterrupted two epochs, the same in two sessions), and rank 0's state."""
    n_batch = -(-n_sample // 2)
    want, heads, states, generators = [], [], [], []
    for rank in range(WORLD):
        _seed(5)
        want.append(_take(_loader(dev, rank, n_sample, prefetch=prefetch), 2))
        _seed(5)
        first = _loader(dev, rank, n_sample, prefetch=prefetch)
        assert first.state_dict() == {}      # before the first epoch
        heads.append(_take(first, 1, stop=taken))
        states.append(first.state_dict())
        generators.append((np.random.get_state(), torch.get_rng_state()))
    assert states[0] == states[1] and _same_generators(*generators)      # ONE state: rank 0's is the file's
    state = states[0]
    assert state["next"] == taken and len(state["order"]) == n_sample and len(state["plans"]) == min(prefetch, n_batch - taken)
    for b, (frames, shape, _, _, cropped) in enumerate(state["plans"], taken):      # the plans of whole global batches
        assert [f[0] for f in frames] == state["order"][2 * b:2 * b + 2] and list(shape) == [24, 40] and cropped
    torch.save(state, str(tmp_path / "state.pth"))      # through a file, as a training state goes
    state = torch.load(str(tmp_path / "state.pth"), map_location="cpu")
    got = []
    for rank in range(WORLD):
        _seed(6 + rank)      # other seeds, and not the same on the two ranks: what follows comes from the state alone
        second = _loader(dev, rank, n_sample, prefetch=prefetch)
        second.load_state_dict(state)
        if harm is not None:
            harm(second)
        np.random.set_state(generators[0][0])      # rank 0's, set last on every rank
        torch.set_rng_state(generators[0][1])
        tail = _take(second, 1)
        assert len(tail) == n_batch - taken and second.state_dict() == {}      # after the epoch's last batch
        got.append(heads[rank] + tail + _take(second, 1))      # an ordinary epoch follows
    return want, got, state


@pytest.mark.parametrize("n_sample,prefetch,taken", CASES)
def test_both_ranks_continue_from_rank_0s_state(dev, n_sample, prefetch, taken, tmp_path):
    want, got, _ = _interrupted(dev, n_sample, prefetch, taken, tmp_path)
    n_batch = -(-n_sample // 2)
    for rank in range(WORLD):
        assert len(want[rank]) == 2 * n_batch
        assert _same_batches(got[rank], want[rank]), rank
    # the shards are what they should be: a frame each, and of the one-frame batch that ends an epoch rank 1 holds none
    assert [batch[0].shape[0] for batch in want[0]] == [1] * (2 * n_batch)
    assert [batch[0].shape[0] for batch in want[1]] == ([1] * (n_batch - 1) + [0]) * 2
    assert tuple(want[1][n_batch - 1][0].shape) == (0, 3, 24, 40) and tuple(want[1][n_batch - 1][4].shape) == (0, 3, 3)
    assert not _same_batches(want[0][:n_batch], want[0][n_batch:])      # the two epochs are not one epoch twice
    assert not _same_batches(want[0], want[1])      # nor the two ranks one rank twice


@pytest.mark.parametrize("n_sample,prefetch,taken", [(9, 4, 1), (3, 4, 1)])
def test_power_without_the_stored_plans(dev, n_sample, prefetch, taken, tmp_path):
    dropped = []

    def without_plans(loader):
        dropped.append(len(loader._resume["plans"]))
        loader._resume["plans"] = []      # the crops of the batches in flight are drawn again, from the restored generator

    want, got, _ = _interrupted(dev, n_sample, prefetch, taken, tmp_path, harm=without_plans)
    assert dropped == [min(prefetch, -(-n_sample // 2) - taken)] * WORLD
    assert not _same_batches(got[0], want[0])      # rank 0 holds a frame of every batch
    assert _same_batches(got[0][:taken], want[0][:taken])      # and what came before the state is not what differs


def test_a_rank_takes_its_own_share_of_a_stored_plan(dev, tmp_path):
    """The state does not know the rank: rank 1 given the state yields rank 1's frames, not rank 0's."""
    want, got, state = _interrupted(dev, 9, 4, 1, tmp_path)
    _seed(9)
    swapped = _loader(dev, 0, 9, prefetch=4)
    swapped.load_state_dict(state)
    first = next(iter(swapped))
    assert all(torch.equal(a, b) for a, b in zip(first, want[0][1])) and not all(torch.equal(a, b) for a, b in zip(first, want[1][1]))
    for f in swapped._pending:      # the batches left in flight own staging sets
        f.exception()


def test_own_crops_keep_raising(dev):
    own = _loader(dev, 0, 9, crops="own")
    with pytest.raises(KbnError, match="sharded.*crops='global'"):
        own.state_dict()
    with pytest.raises(KbnError, match="sharded.*crops='global'"):
        own.load_state_dict({})
