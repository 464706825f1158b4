"""GPU, one process: a rank's part of a global batch is the slice of what one process builds, bit for bit.

ops.augment(..., frame_base=first) over frames [first, first + n) against the [first:] slice of the call over the whole batch (same
seed and call; kbn_augment_forward_at, csrc/augment.hip), one global call against the NumPy oracle (tests/transforms_oracle.py), and
Transforms.transform(shard=...) behind TrainingFrameLoader(crops="global") for ranks 0 and 1 of world 2 against the world-1 batch
-- each rank a loader and a Transforms of its own in this process, no process group, under one np.random.seed / torch.manual_seed
a run.  The same comparisons with frame_base=0, shard=None and crops="own" -- the package without the feature -- must differ.

    python -m pytest tests/test_augment_shard_gpu.py -m gpu -q
"""
import numpy as np
import pytest
import torch

import kbnet_amd as kb
import run_cases as rc
import transforms_cases as tc

pytestmark = pytest.mark.gpu

FLAGS = [15, 0, 12, 15, 8 | 4 | 1]      # all four bits, none, removal + noise, all four again, removal + noise + horizontal flip
DENSITIES = [0.6123, 0.65, 0.7, 0.6789, 0.6321]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need a visible MI355X (run with -m gpu on a GPU box)")
    kb._lib.load()   # a missing extension is an error on a GPU box, never a skip
    return torch.device("cuda:0")


def _case(h, w, noise_type):
    """5 frames: three image tensors of 3 channels, one range map, two tensors in the validity-map role."""
    rng = np.random.default_rng(41)
    depth = tc._depth(rng, 5, 1, h, w, 0.4)
    return tc._case(f"shard 5x{h}x{w} {noise_type}", tc._images(rng, 5, 3, h, w, 3), [depth], [depth.copy(), (depth > 0).astype(np.float32)],
                    FLAGS, DENSITIES, normalized_image_range=[0, 1], noise_type=noise_type, noise_spread=0.5 if noise_type == "uniform" else 0.1)


def _augment(case, dev, first, last, frame_base):
    ins = [[torch.from_numpy(x).to(dev)[first:last] for x in case[key]] for key in ("images", "ranges", "validity")]
    densities = torch.from_numpy(case["densities"]).to(dev)[first:last].contiguous()
    outs = kb.ops.augment(*ins, case["flags"][first:last], densities, frame_base=frame_base, **case["options"])
    torch.cuda.synchronize()
    return [t for lst in outs for t in lst]


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("noise_type", ["uniform", "gaussian"])
@pytest.mark.parametrize("h,w", [(12, 20), (13, 19)], ids=["16-byte path", "scalar path"])
def test_a_shard_with_frame_base_is_the_slice_of_the_global_call(dev, h, w, noise_type):
    case = _case(h, w, noise_type)
    n = len(case["flags"])
    whole = _augment(case, dev, 0, n, 0)
    assert len(whole) == 6
    sparse_in, sparse_out = torch.from_numpy(case["ranges"][0]).to(dev), whole[3]
    for b in (0, 2, 3, 4):      # the call did something to every flagged frame: points removed, noise on those that stay
        kept = sparse_out[b] != 0
        removed = int((sparse_in[b] > 0).sum()) - int(kept.sum())
        assert removed == int(np.float32(DENSITIES[b]) * np.float32(int((sparse_in[b] > 0).sum()))), b
    for first, last in ((2, 5), (0, 2), (4, 5)):
        part = _augment(case, dev, first, last, first)
        for i, (p, g) in enumerate(zip(part, whole)):
            assert _same(p, g[first:last]), (first, last, i)
    # without the frame word the shard's frames draw what frames 0, 1, 2 draw: other points go, other noise
    blind = _augment(case, dev, 2, 5, 0)
    assert not _same(blind[3], whole[3][2:5])
    assert all(_same(blind[i], whole[i][2:5]) for i in (0, 1, 2, 4, 5))      # images and validity maps draw nothing


def test_the_global_call_against_the_oracle(dev):
    case = _case(12, 20, "uniform")
    got = _augment(case, dev, 0, 5, 0)
    got = [[t.cpu().numpy() for t in got[:3]], [got[3].cpu().numpy()], [t.cpu().numpy() for t in got[4:]]]
    assert tc.mismatches(case, got) == []


def test_the_frame_word_is_not_the_chunks_first_frame(dev):
    """515 frames of 1 x 4 x 8: the global call takes two launches (KBN_AUGMENT_MAX_FRAMES = 512, frame0 = 0 and 512), the shard
    [509, 515) one, with frame0 = 0 and frame_base = 509."""
    rng = np.random.default_rng(43)
    n = 515
    depth = tc._depth(rng, n, 1, 4, 8, 0.7)
    flags = [int(f) for f in rng.choice([4, 8, 12, 13, 14, 15, 0], size=n)]
    flags[509:] = [12, 15, 4, 8, 0, 13]
    case = tc._case("515 frames", [], [depth], [], flags, rng.uniform(0.6, 0.7, size=n), noise_type="uniform", noise_spread=0.5)
    [whole] = _augment(case, dev, 0, n, 0)
    for first, last in ((509, 515), (512, 515), (0, 3)):
        [part] = _augment(case, dev, first, last, first)
        assert _same(part, whole[first:last]), (first, last)
    [blind] = _augment(case, dev, 509, 515, 0)
    assert not _same(blind, whole[509:])
    last_words = kb.ops.augment([], [torch.from_numpy(depth[:2]).to(dev)], [], [12, 12], torch.full((2,), 0.65, device=dev), noise_type="uniform",
                                noise_spread=0.5, seed=1, frame_base=0xFFFFFFFD)      # frame words 2^32 - 3 and 2^32 - 2: the last allowed
    assert len(last_words[1]) == 1 and bool(torch.isfinite(last_words[1][0]).all())
    with pytest.raises(kb._lib.KbnError, match="frame_base"):
        kb.ops.augment([], [torch.from_numpy(depth[:2]).to(dev)], [], [0, 0], None, frame_base=0xFFFFFFFE)


# ------------------------------------------------------------------------------------------------ Transforms and the loader
SHAPE = (16, 24)      # smaller than the 24 x 40 frames of golden/io: every crop is drawn


def _epochs(dev, crop_type, rank, world, crops, sharded, epochs=2):
    """Two epochs of one global batch of three frames through the loader and train_inputs, under one pair of seeds -> per epoch the
    seven tensors a rank feeds its networks (six of train_inputs and the intrinsics), on the host."""
    images, depths, intrinsics, _ = rc.path_lists()
    np.random.seed(5)
    torch.manual_seed(6)
    more = {} if world == 1 else {"rank": rank, "world": world, "crops": crops}
    loader = kb.loader.TrainingFrameLoader(images, depths, intrinsics, shape=list(SHAPE), random_crop_type=crop_type, batch_size=3, shuffle=False,
                                           device=dev, workers=2, prefetch=2, **more)
    transforms = kb.transforms.Transforms(normalized_image_range=[0, 1], random_flip_type=["horizontal", "vertical"],
                                          random_remove_points=[0.6, 0.7], random_noise_type="gaussian", random_noise_spread=0.1, seed=99)
    out = []
    for _ in range(epochs):
        for b, (image0, image1, image2, sparse_depth0, k) in enumerate(loader):
            n_global = loader.global_batch_size(b)
            shard = (kb.dist.shard_bounds(n_global, rank, world)[0], n_global) if sharded else None
            got = kb.transforms.train_inputs(transforms, image0, image1, image2, sparse_depth0, 0.9, shard=shard)
            torch.cuda.synchronize()
            out.append([t.cpu() for t in got] + [k.cpu()])
    assert transforms.calls == epochs
    return out


@pytest.mark.parametrize("crop_type", [["horizontal", "vertical"], ["horizontal", "vertical", "anchored"]], ids=["free", "anchored"])
def test_two_ranks_build_the_one_process_batch(dev, crop_type):
    whole = _epochs(dev, crop_type, 0, 1, None, False)
    ranks = [_epochs(dev, crop_type, rank, 2, "global", True) for rank in range(2)]
    assert len(whole) == 2 and [t.shape[0] for t in ranks[0][0]] == [2] * 7 and [t.shape[0] for t in ranks[1][0]] == [1] * 7
    assert not _same(whole[0][3], whole[1][3])      # the epochs differ: other crops, another call
    for e in range(2):
        for i in range(7):
            assert _same(torch.cat([ranks[0][e][i], ranks[1][e][i]], dim=0), whole[e][i]), (e, i)
    # the package without the feature: crops of the rank's own samples, draws for the rank's own frames, frame word from 0
    old = [_epochs(dev, crop_type, rank, 2, "own", False) for rank in range(2)]
    differing = [(e, i) for e in range(2) for i in range(7) if not _same(torch.cat([old[0][e][i], old[1][e][i]], dim=0), whole[e][i])]
    print(f"{crop_type}: without crops='global' / shard= {len(differing)} of 14 tensors differ from the one-process batch")
    assert differing, "the test cannot tell the sharded draws from per-rank draws"
    # each half alone: global crops without shard= and the reverse are not enough either
    for crops, sharded in (("global", False), ("own", True)):
        half = [_epochs(dev, crop_type, rank, 2, crops, sharded, epochs=1) for rank in range(2)]
        assert any(not _same(torch.cat([half[0][0][i], half[1][0][i]], dim=0), whole[0][i]) for i in range(7)), (crops, sharded)
