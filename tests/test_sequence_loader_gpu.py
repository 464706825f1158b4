"""GPU: both loaders and the entry points on sequence entries (previous<TAB>current<TAB>next) against the same runs on the
triplet files np.concatenate([previous, current, next], axis=1) makes of the same frames -- what the reference's setup scripts would
have written.  Everything is exact: torch.equal batches, equal bytes, equal checkpoints.

    python -m pytest tests/test_sequence_loader_gpu.py -m gpu -q

Two synthetic sequences of five frames, 24 x 40 and 20 x 36, RGB with 16-bit depth, as PNG and as packed frames; ten samples
(window 1, the ends repeated).  The entry-point tests use the three 24 x 40 frames of tests/golden/io, their triplets cut into frames."""
import os
import shutil

import numpy as np
import pytest
import torch

import kbnet_amd as kb
import run_cases as rc
import train_cases as tc

pytestmark = pytest.mark.gpu
KbnError = kb._lib.KbnError
KITTI_CROP = ["horizontal", "bottom"]      # run_kbnet's KITTI training script
SIZES = ((24, 40), (20, 36))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _write(path, data):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        f.write(data)
    return path


def _image_file(path, px, packed):
    return _write(path, kb.loader.encode_frame(px) if packed else kb.loader.encode_image_png(px))


def _depth_file(path, z, packed):
    return _write(path, kb.loader.encode_frame(z) if packed else kb.loader.encode_depth_png(z))


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """lists[(form, kind)] = (image entries, sparse depth paths, intrinsics paths) for form 'sequence' / 'triplet', kind 'png' /
    'packed'; the same ten samples in the same order in all four.  frames[kind][s]: the frame files of sequence s."""
    root = str(tmp_path_factory.mktemp("sequences"))
    rng = np.random.default_rng(42)
    lists, frames = {}, {"png": [], "packed": []}
    pixels = [[rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for _ in range(5)] for h, w in SIZES]
    depths = [[(rng.integers(0, 65536, size=(h, w)) * (rng.uniform(size=(h, w)) < 0.3)).astype(np.uint16) for _ in range(5)] for h, w in SIZES]
    intrinsics = []
    for s in range(2):
        for i in range(5):
            k = np.array([[700.0 + 10 * s + i, 0.0, SIZES[s][1] / 2.0], [0.0, 705.0 + i, SIZES[s][0] / 2.0], [0.0, 0.0, 1.0]], dtype=np.float32)
            intrinsics.append(os.path.join(root, f"k_{s}_{i}.npy"))
            np.save(intrinsics[-1], k)
    for kind in ("png", "packed"):
        packed, ext = kind == "packed", ".kbf" if kind == "packed" else ".png"
        entries, triplets, depth_paths = [], [], []
        for s in range(2):
            files = [_image_file(os.path.join(root, kind, f"seq{s}", f"{i:04d}{ext}"), pixels[s][i], packed) for i in range(5)]
            frames[kind].append(files)
            entries += kb.loader.sequence_lines(files, window=1, ends="repeat")
            for i in range(5):
                before, after = max(i - 1, 0), min(i + 1, 4)
                triplet = np.concatenate([pixels[s][before], pixels[s][i], pixels[s][after]], axis=1)
                triplets.append(_image_file(os.path.join(root, kind, f"triplet{s}", f"{i:04d}{ext}"), triplet, packed))
                depth_paths.append(_depth_file(os.path.join(root, kind, f"depth{s}", f"{i:04d}{ext}"), depths[s][i], packed))
        lists[("sequence", kind)] = (entries, depth_paths, intrinsics)
        lists[("triplet", kind)] = (triplets, depth_paths, intrinsics)
    return {"root": root, "lists": lists, "frames": frames, "pixels": pixels}


def _loader(dev, paths, **kw):
    settings = dict(shape=(16, 32), random_crop_type=KITTI_CROP, batch_size=4, shuffle=True, device=dev, workers=2, prefetch=2)
    settings.update(kw)
    return kb.loader.TrainingFrameLoader(*paths, **settings)


def _epochs(dev, paths, epochs=2, **kw):
    """Every batch of `epochs` epochs under one NumPy seed and one torch generator."""
    np.random.seed(3)
    loader = _loader(dev, paths, generator=torch.Generator().manual_seed(5), **kw)
    return [[t.clone() for t in batch] for _ in range(epochs) for batch in loader]


def _same(a, b):
    assert len(a) == len(b) and len(a) > 0
    for x, y in zip(a, b):
        assert len(x) == len(y) == 5
        for t, u in zip(x, y):
            assert t.shape == u.shape and torch.equal(t, u)


MODES = {
    "kitti crop, shuffled": dict(),
    "kitti crop, in order": dict(shuffle=False),
    "every crop type, shuffled": dict(random_crop_type=["horizontal", "vertical", "anchored"]),
    "no crop, a size a batch": dict(shape=None, shuffle=False, batch_size=5),
}


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("kind", ["png", "packed"])
def test_training_batches_equal_the_triplet_files(dev, data, kind, mode):
    got = _epochs(dev, data["lists"][("sequence", kind)], **MODES[mode])
    _same(got, _epochs(dev, data["lists"][("triplet", kind)], **MODES[mode]))
    assert sum(b[0].shape[0] for b in got) == 20, "ten samples an epoch, two epochs"
    if mode == "kitti crop, in order" and kind == "png":      # and the triplet path is not merely equal but right: sample 1 of sequence 0
        image0, image1, image2 = (got[0][k][1].cpu().numpy() for k in range(3))
        y, x = 24 - 16, int(round(40 / 2.0 - got[0][4][1, 0, 2].item()))      # 'bottom'; x from the principal point the crop moved
        for image, i in ((image1, 0), (image0, 1), (image2, 2)):
            assert np.array_equal(image, np.transpose(data["pixels"][0][i][y:y + 16, x:x + 32], (2, 0, 1)).astype(np.float32))


@pytest.mark.parametrize("kind", ["png", "packed"])
def test_ranks_with_global_crops(dev, data, kind):
    """rank 0/2 and 1/2 under crops='global': batches of 3 over ten samples, so the last global batch holds one sample and rank 1's
    shard of it is empty."""
    for rank in (0, 1):
        kw = dict(batch_size=3, rank=rank, world=2, crops="global")
        got = _epochs(dev, data["lists"][("sequence", kind)], **kw)
        _same(got, _epochs(dev, data["lists"][("triplet", kind)], **kw))
        assert got[3][0].shape[0] == (1 if rank == 0 else 0)


@pytest.mark.parametrize("kind", ["png", "packed"])
def test_state_dict_mid_epoch_continues_in_a_fresh_loader(dev, data, kind):
    whole = _epochs(dev, data["lists"][("triplet", kind)], epochs=1)
    np.random.seed(3)
    first = _loader(dev, data["lists"][("sequence", kind)], generator=torch.Generator().manual_seed(5))
    it = iter(first)
    got = [[t.clone() for t in next(it)]]
    state, drawn = first.state_dict(), np.random.get_state()
    assert state["next"] == 1 and len(state["plans"]) == 2
    np.random.seed(99)      # the fresh loader's session starts elsewhere ...
    second = _loader(dev, data["lists"][("sequence", kind)], generator=torch.Generator().manual_seed(77))
    second.load_state_dict(state)
    np.random.set_state(drawn)      # ... and is put where the first stood
    got += [[t.clone() for t in batch] for batch in second]
    _same(got, whole)


def test_every_distinct_file_of_a_batch_is_read_once(dev, data, monkeypatch):
    """Samples 0 .. 3 of sequence 0 name twelve frames, five of them distinct; with their four depth maps nine files are read."""
    read, original = [], kb.loader._read

    def counting(path):
        read.append(path)
        return original(path)

    monkeypatch.setattr(kb.loader, "_read", counting)
    images, depths, ks = data["lists"][("sequence", "png")]
    np.random.seed(3)
    batches = list(_loader(dev, (images[:4], depths[:4], ks[:4]), shuffle=False))
    assert len(batches) == 1 and batches[0][0].shape[0] == 4
    assert sorted(read) == sorted(data["frames"]["png"][0] + depths[:4])


@pytest.mark.parametrize("kind", ["png", "packed"])
def test_inference_loader_on_window_0_entries(dev, data, kind, tmp_path):
    """p<TAB>p<TAB>p, the reference's validation images: only `current` is read, and the batches are those of the frame written
    three times side by side.  Packed single frames work here for the first time."""
    packed, ext = kind == "packed", ".kbf" if kind == "packed" else ".png"
    files = data["frames"][kind][0]
    _, depths, ks = data["lists"][("sequence", kind)]
    tripled = [_image_file(str(tmp_path / f"{i}{ext}"), np.concatenate([data["pixels"][0][i]] * 3, axis=1), packed) for i in range(5)]
    entries = kb.loader.sequence_lines(files, window=0)
    runs = []
    for images in (entries, tripled):
        loader = kb.loader.InferenceFrameLoader(images, depths[:5], ks[:5], use_image_triplet=True, batch_size=2, device=dev, workers=2)
        runs.append([[t.clone() for t in batch] for batch in loader])
    assert [b[0].shape[0] for b in runs[0]] == [2, 2, 1]
    for x, y in zip(*runs):
        assert len(x) == len(y) == 3 and all(torch.equal(t, u) for t, u in zip(x, y))
    assert np.array_equal(runs[0][0][0][1].cpu().numpy(), np.transpose(data["pixels"][0][1], (2, 0, 1)).astype(np.float32))


def test_mismatched_neighbours_and_mixed_batches_raise_when_the_batch_is_due(dev, data):
    images, depths, ks = (list(v) for v in data["lists"][("sequence", "png")])
    triplets = data["lists"][("triplet", "png")][0]
    small = data["frames"]["png"][1][0]      # a 20 x 36 frame as the `next` of a 24 x 40 sample
    bad = list(images)
    bad[5] = "\t".join(kb.loader.split_sample(images[1])[:2] + (small,))
    np.random.seed(3)
    it = iter(_loader(dev, (bad, depths, ks), shuffle=False))      # constructing and starting the epoch raises nothing
    assert next(it)[0].shape[0] == 4
    with pytest.raises(KbnError) as e:
        next(it)
    assert "three frames of a sample must have one size and format" in str(e.value) and small in str(e.value)
    mixed = list(images)
    mixed[6] = triplets[6]
    np.random.seed(3)
    it = iter(_loader(dev, (mixed, depths, ks), shuffle=False))
    assert next(it)[0].shape[0] == 4
    with pytest.raises(KbnError) as e:
        next(it)
    assert "all triplet files or all sequence entries" in str(e.value) and triplets[6] in str(e.value)
    loader = kb.loader.InferenceFrameLoader(mixed[4:8], depths[4:8], ks[4:8], batch_size=4, device=dev, workers=2)
    with pytest.raises(KbnError) as e:
        list(loader)
    assert "all triplet files or all sequence entries" in str(e.value)
    # the depth map of a sequence sample has the size of a FRAME
    wrong = list(depths)
    wrong[0] = depths[5]
    np.random.seed(3)
    with pytest.raises(KbnError) as e:
        next(iter(_loader(dev, (images, wrong, ks), shuffle=False)))
    assert "depth map" in str(e.value) and depths[5] in str(e.value)


# ------------------------------------------------------------------------------------------------ the entry points
@pytest.fixture(scope="module")
def golden_lists(tmp_path_factory):
    """The four lists of tests/golden/io as they are (triplet files), and with every triplet cut into its three frames: the
    `current` frame keeps the triplet's base name, so names derived from it are the triplet run's."""
    root = tmp_path_factory.mktemp("golden_sequences")
    images, depths, ks, truths = rc.path_lists()
    entries = []
    for path in images:
        with open(path, "rb") as f:
            px = kb.loader.decode_png(f.read())
        w = px.shape[1] // 3
        fields = [_image_file(str(root / which / os.path.basename(path)), np.ascontiguousarray(px[:, k * w:(k + 1) * w]), False)
                  for k, which in enumerate(("previous", "current", "next"))]
        entries.append("\t".join(fields))
    out = {}
    for form, image_list in (("triplet", images), ("sequence", entries)):
        os.makedirs(root / form)
        names = []
        for name, paths in zip(("image.txt", "sparse_depth.txt", "intrinsics.txt", "ground_truth.txt"), (image_list, depths, ks, truths)):
            kb.loader.write_paths(str(root / form / name), paths)
            names.append(str(root / form / name))
        out[form] = names
    return out


def test_run_on_sequence_entries(dev, golden_lists, tmp_path):
    outs = {}
    for form, lists in golden_lists.items():
        outs[form] = str(tmp_path / form)
        kb.inference.run(lists[0], lists[1], lists[2], lists[3], checkpoint_path=outs[form], depth_model_restore_path=rc.CHECKPOINT,
                         save_outputs=True, keep_input_filenames=True, device="cuda", batch_size=2, workers=2,
                         **rc.run_settings(kb.kitti_config().narrow()))
    metrics = {}
    for form, out in outs.items():
        with open(os.path.join(out, "results.txt")) as f:
            lines = f.read().splitlines()
        at = lines.index("Evaluation results:")
        metrics[form] = lines[at:at + 5]
    assert metrics["sequence"] == metrics["triplet"] and len(metrics["sequence"]) == 5
    for directory in rc.DIRECTORIES:
        names = sorted(os.listdir(os.path.join(outs["triplet"], "outputs", directory)))
        assert names == sorted(os.listdir(os.path.join(outs["sequence"], "outputs", directory))) == [f"triplet_{i}.png" for i in range(3)]
        for name in names:
            with open(os.path.join(outs["triplet"], "outputs", directory, name), "rb") as a, \
                    open(os.path.join(outs["sequence"], "outputs", directory, name), "rb") as b:
                assert a.read() == b.read(), (directory, name)


def test_train_two_steps_on_sequence_entries(dev, golden_lists, tmp_path):
    """Two epochs of one step each, a checkpoint and (from step 2) a validation a step: the smallest configuration of
    tests/test_train_gpu.py, through train()'s path-list arguments with no new argument."""
    settings = tc.train_settings(kb.kitti_config().narrow())
    settings.update(learning_rates=[1e-4, 5e-5], learning_schedule=[1, 2])
    pose = str(tmp_path / tc.POSE_CHECKPOINT)
    tc.write_pose_checkpoint(kb, pose)
    depth = shutil.copy(rc.CHECKPOINT, str(tmp_path))
    tensors = {}
    for form, lists in golden_lists.items():
        out = str(tmp_path / form)
        torch.manual_seed(0)
        np.random.seed(0)
        kb.training.train(lists[0], lists[1], lists[2], lists[0], lists[1], lists[2], lists[3], checkpoint_path=out,
                          depth_model_restore_path=depth, pose_model_restore_path=pose, device="cuda", workers=2, **settings)
        tensors[form] = {}
        for model in ("depth_model", "pose_model"):
            ckpt = torch.load(os.path.join(out, f"{model}-2.pth"), map_location="cpu")
            for key, value in ckpt.items():
                if key.endswith("_state_dict") and key != "optimizer_state_dict":
                    tensors[form].update({f"{model}.{key}.{name}": t for name, t in value.items()})
    assert len(tensors["sequence"]) > 100 and set(tensors["sequence"]) == set(tensors["triplet"])
    for name, t in tensors["sequence"].items():
        assert torch.equal(t, tensors["triplet"][name]), name
