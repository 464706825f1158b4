"""Data-parallel kb.training.train without a GPU: the step count with ranks, that a rank's host draws -- Transforms.draw, the removal
densities, the crops -- are the slices of the global batch's and leave the generators where one process leaves them, the C entry
point's refusal, and what launch() and train_ranks(world=2) refuse before anything is started or written."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kbnet_amd as kb  # noqa: E402
import run_cases as rc  # noqa: E402
import train_cases as tc  # noqa: E402

KbnError = kb._lib.KbnError


def test_n_train_steps_counts_the_batches_every_rank_has_a_frame_of():
    steps = kb.training.n_train_steps
    assert steps(3, 2, [3], world=2) == 3            # batches of 2 and 1 frames: one step an epoch, three epochs
    assert steps(3, 2, [3]) == steps(3, 2, [3], world=1) == 6
    assert steps(3, 3, [1, 3], world=2) == 3         # the 2 + 1 split of tests/train_cases.py: a step
    assert steps(1003, 8, [2, 8, 20, 30, 45, 60], world=8) == 60 * 125      # the last batch holds 3 frames
    assert steps(1003, 8, [2, 8, 20, 30, 45, 60], world=3) == 60 * 126
    assert steps(5, 2, [4], world=3) == 0            # no batch reaches three frames
    assert isinstance(steps(3, 2, [3], world=2), int)


def _transform(monkeypatch, n_local, shard):
    """One Transforms.transform call on CPU tensors with ops.augment replaced by a recorder -> (what it was handed, np.random's
    state, torch's state, the object's call count)."""
    seen = {}

    def record(images, range_maps, validity_maps, flags, densities, **options):
        seen.update(flags=list(flags), densities=None if densities is None else densities.clone(), n=images[0].shape[0], **options)
        return [list(images), list(range_maps), list(validity_maps)]

    monkeypatch.setattr(kb.ops, "augment", record)
    np.random.seed(21)
    torch.manual_seed(22)
    t = kb.transforms.Transforms(normalized_image_range=[0, 1], random_flip_type=["horizontal", "vertical"], random_remove_points=[0.6, 0.7],
                                 random_noise_type="gaussian", random_noise_spread=0.1, seed=7)
    for call in range(2):      # two calls: the count of calls is a word of the draws
        t.transform([torch.zeros(n_local, 3, 4, 8)], [torch.zeros(n_local, 1, 4, 8)], [], random_transform_probability=0.9, shard=shard)
        assert seen["call"] == call
    return seen, np.random.get_state(), torch.get_rng_state(), t.calls


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_a_shards_draws_are_the_slice_of_the_global_draws(monkeypatch):
    whole, numpy_state, torch_state, calls = _transform(monkeypatch, 5, None)
    assert whole["frame_base"] == 0 and whole["n"] == 5 and len(set(whole["flags"])) > 1 and calls == 2
    assert len(set(whole["densities"].tolist())) == 5
    for first, last in [kb.dist.shard_bounds(5, rank, 2) for rank in range(2)] + [(5, 5), (0, 5)]:      # 3 + 2 frames, an empty shard, all
        got, ns, ts, n_calls = _transform(monkeypatch, last - first, (first, 5))
        assert got["frame_base"] == first and got["n"] == last - first
        assert got["flags"] == whole["flags"][first:last]
        assert torch.equal(got["densities"], whole["densities"][first:last]) and got["densities"].is_contiguous()
        assert got["seed"] == whole["seed"] == 7
        assert _same_state(ns, numpy_state) and torch.equal(ts, torch_state) and n_calls == calls == 2, (first, last)
    # and the power of the comparison: a rank that draws for its own two frames alone gets other decisions and leaves another state
    own, ns, ts, _ = _transform(monkeypatch, 2, None)
    assert not _same_state(ns, numpy_state) and not torch.equal(own["densities"], whole["densities"][3:5])


def test_draw_of_the_global_batch_is_what_transform_slices():
    t = kb.transforms.Transforms(random_flip_type=["horizontal"], random_remove_points=[0.6, 0.7], seed=1)
    np.random.seed(3)
    whole = t.draw(7, 0.8)
    after = np.random.get_state()
    np.random.seed(3)
    assert t.draw(7, 0.8)[2:5] == whole[2:5] and _same_state(np.random.get_state(), after)


def test_a_shard_outside_its_batch_is_refused():
    t = kb.transforms.Transforms(seed=1)
    for shard in [(4, 5), (-1, 5), (0, 1)]:
        with pytest.raises(ValueError, match="shard"):
            t.transform([torch.zeros(2, 3, 4, 8)], shard=shard)
    assert t.calls == 0


SIZES = [(24, 40), (26, 44), (26, 44), (24, 40), (25, 43)]      # frames of different raw sizes in one batch


@pytest.mark.parametrize("crop_type", [["horizontal", "vertical"], ["horizontal", "vertical", "anchored"]], ids=["free", "anchored"])
def test_global_crop_draws_of_two_ranks_concatenate_to_the_one_process_draws(crop_type):
    shape = (16, 24)
    np.random.seed(31)
    whole = kb.loader.draw_crops(SIZES, shape, crop_type)
    after = np.random.get_state()
    np.random.seed(31)
    assert whole == [kb.loader.draw_crop(h, w, shape, crop_type) for h, w in SIZES]      # draw_crop, sample by sample in batch order
    parts = []
    for rank in range(2):
        np.random.seed(31)
        parts.append(kb.loader.draw_crops(SIZES, shape, crop_type, keep=kb.dist.shard_bounds(len(SIZES), rank, 2)))
        assert _same_state(np.random.get_state(), after), rank
    assert [len(p) for p in parts] == [3, 2] and parts[0] + parts[1] == whole
    np.random.seed(31)
    assert kb.loader.draw_crops(SIZES, shape, crop_type, keep=(5, 5)) == [] and _same_state(np.random.get_state(), after)
    # crops="own": rank 1 draws for its two samples alone -- other crops than the global batch's
    np.random.seed(31)
    own = kb.loader.draw_crops(SIZES[3:], shape, crop_type)
    assert own != whole[3:] and not _same_state(np.random.get_state(), after)


def test_loader_refuses_an_unknown_crops_mode():
    with pytest.raises(KbnError, match="crops"):
        kb.loader.TrainingFrameLoader(["a"], ["b"], ["c"], device="cuda:0", crops="all")


def test_entry_point_refuses_a_frame_word_past_32_bits():
    lib = kb._lib.load()
    table = (kb._lib.AugmentTensor * 1)()      # all zero: never read before the refusal, a NULL src after it
    at = lib.kbn_augment_forward_at
    assert at(table, 1, bytes(2), 2, 1, 1, None, None, 0, 0, 0, 0.0, 0, 0, 0xFFFFFFFE, 3, None) == kb._lib.KBN_ERR_UNSUPPORTED
    assert at(table, 1, bytes(2), 2, 1, 1, None, None, 0, 0, 0, 0.0, 0, 0, 0xFFFFFFFD, 3, None) == kb._lib.KBN_ERR_INVALID_ARGUMENT
    assert at(None, 0, None, 0, 0, 0, None, None, 0, 0, 0, 0.0, 0, 0, 0, 0, None) == kb._lib.KBN_ERR_INVALID_ARGUMENT
    header = open(os.path.join(ROOT, "include", "kbnet_hip.h")).read()
    assert "int kbn_augment_forward_at(" in header and "unsigned frame_base" in header
    x = torch.zeros(2, 1, 4, 8)
    for frame_base in (-1, 0xFFFFFFFE):
        with pytest.raises(KbnError, match="frame_base"):
            kb.ops.augment([], [x], [], [0, 0], None, frame_base=frame_base)
    assert C.sizeof(kb._lib.AugmentTensor) == 64


def _write_paths(filepath, paths):
    with open(filepath, "w") as f:
        f.write("\n".join(paths) + "\n")


def _arguments(tmp_path):
    lists = [str(tmp_path / name) for name in rc.write_lists(str(tmp_path), _write_paths)]
    names = ("train_image_path", "train_sparse_depth_path", "train_intrinsics_path", "val_image_path", "val_sparse_depth_path",
             "val_intrinsics_path", "val_ground_truth_path")
    arguments = dict(zip(names, lists[:3] + lists))
    arguments.update(tc.train_settings(kb.kitti_config().narrow()), checkpoint_path=str(tmp_path / "trained"), device="cuda")
    return arguments


def test_launch_refuses_before_it_starts_anything(tmp_path, monkeypatch):
    arguments = _arguments(tmp_path)
    started = []
    monkeypatch.setattr(kb.training.subprocess, "Popen", lambda *a, **k: started.append(a))
    for n_gpus in (0, 17, -1, True, 2.0):
        with pytest.raises(KbnError, match="n_gpus"):
            kb.training.launch(n_gpus, backend="gloo", **arguments)
    for devices in ([0], [0, 0, 0], [0, -1]):
        with pytest.raises(KbnError, match="devices"):
            kb.training.launch(2, backend="gloo", devices=devices, **arguments)
    with pytest.raises(KbnError, match="devices"):
        kb.training.launch(2, backend="nccl", devices=[0, 0], **arguments)      # RCCL ranks do not share a device
    with pytest.raises(KbnError, match="backend"):
        kb.training.launch(2, backend="mpi", **arguments)
    with pytest.raises(KbnError, match="rank is set by launch"):
        kb.training.launch(2, backend="gloo", rank=1, **arguments)
    with pytest.raises(KbnError, match="timeout"):
        kb.training.launch(2, backend="gloo", timeout=0, **arguments)
    assert not started and not os.path.exists(arguments["checkpoint_path"])


def test_train_keeps_the_references_signature_and_train_ranks_adds_three():
    import inspect
    one, ranks = inspect.signature(kb.training.train).parameters, inspect.signature(kb.training.train_ranks).parameters
    assert list(ranks)[:len(one)] == list(one) and list(ranks)[len(one):] == ["rank", "world", "sync_batch_norm"]
    assert all(ranks[name].default == p.default and ranks[name].kind == p.kind for name, p in one.items())
    assert [ranks[name].default for name in ("rank", "world", "sync_batch_norm")] == [0, 1, True]
    for name in ("rank", "world", "sync_batch_norm"):
        with pytest.raises(TypeError, match=name):
            kb.training.train("a", "b", "c", None, None, None, None, **{name: 1})
    with pytest.raises(KbnError, match="no CPU fallback"):      # train() is train_ranks(world=1): its refusals are this function's
        kb.training.train("a", "b", "c", None, None, None, None, device="cpu")


def test_train_with_ranks_needs_a_process_group(tmp_path):
    arguments = _arguments(tmp_path)
    assert not torch.distributed.is_initialized()
    with pytest.raises(KbnError, match="process group"):
        kb.training.train_ranks(**arguments, rank=1, world=2)
    with pytest.raises(KbnError, match="process group"):
        kb.training.train_ranks(**arguments, rank=0, world=2)
    for rank, world in ((2, 2), (-1, 1), (0, 0)):
        with pytest.raises(KbnError, match="rank"):
            kb.training.train_ranks(**arguments, rank=rank, world=world)
    assert not os.path.exists(arguments["checkpoint_path"])
