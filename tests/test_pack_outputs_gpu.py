"""GPU: packed outputs and packed ground truth.  loader.OutputWriter(file_format="packed") and
kb.inference.run_with_format(output_format="packed") against the PNG path on the same inputs -- file by file the same pixels, and every
packed file byte for byte loader.encode_frame of them --, the exported files fed back as sparse depth and ground truth, and packed
ground-truth lists against PNG ones.

    python -m pytest tests/test_pack_outputs_gpu.py -m gpu -q
"""
import os
import re

import numpy as np
import pytest
import torch

import kbnet_amd as kb
import run_cases as rc

pytestmark = pytest.mark.gpu
KbnError = kb._lib.KbnError
BATCH_SIZES = (1, 2, 3)      # 2: a ragged 2 + 1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def read(path):
    with open(path, "rb") as f:
        return f.read()


def same_file_pair(png_path, packed_path):
    """The PNG and the packed file hold the same pixels (native PNG reader on one side, decode_frame on the other), and the packed
    file is byte for byte encode_frame of them.  Returns the pixels."""
    want = kb.loader.decode_png(read(png_path))
    data = read(packed_path)
    kb.loader.check_frame(data)
    got = kb.loader.decode_frame(data)
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), packed_path
    assert data == kb.loader.encode_frame(want), packed_path
    return want


def same_outputs(png_root, packed_root, names, truth_names=None):
    for directory in rc.DIRECTORIES:
        listed = names if directory != "ground_truth" or truth_names is None else truth_names
        assert sorted(os.listdir(os.path.join(png_root, directory))) == sorted(listed), directory
        assert sorted(os.listdir(os.path.join(packed_root, directory))) == sorted(kb.loader.packed_filename(n) for n in listed), directory
        for name in listed:
            same_file_pair(os.path.join(png_root, directory, name), os.path.join(packed_root, directory, kb.loader.packed_filename(name)))


# ------------------------------------------------------------------------------------------------ OutputWriter
def test_packed_writer_reuses_slots_and_reads_its_own_buffer(dev, tmp_path):
    """tests/test_run_gpu.py's test of the PNG writer, for both formats on the same batches: three submits through two slots, the
    caller overwriting its tensors with NaN right after each submit returns."""
    n, h, w = 2, 24, 40
    batches = [rc.make_sources(n, h, w, seed=50 + b) for b in range(3)]
    truths = [np.random.default_rng(60 + b).integers(0, 65536, size=(n, h, w), dtype=np.uint16) for b in range(3)]
    image, depth_a, depth_b = (torch.empty(s, device=dev) for s in ((n, 3, h, w), (n, 1, h, w), (n, 1, h, w)))
    roots = {fmt: str(tmp_path / fmt) for fmt in ("png", "packed")}
    for fmt, root in roots.items():
        with kb.loader.OutputWriter(root, threads=4, in_flight=2, level=1, file_format=fmt) as writer:
            for b, (sources, truth) in enumerate(zip(batches, truths)):
                for t, src in zip((image, depth_a, depth_b), sources):
                    t.copy_(torch.from_numpy(src))
                given = truth.copy() if b < 2 else None      # the last batch goes without ground truth
                writer.submit([f"{b}_{i}.png" for i in range(n)], image, depth_a, depth_b, ground_truth_samples=given)
                for t in (image, depth_a, depth_b):          # the writer must not read these any more
                    t.fill_(float("nan"))
                if given is not None:
                    given[:] = 0
    names = [f"{b}_{i}.png" for b in range(3) for i in range(n)]
    same_outputs(roots["png"], roots["packed"], names, truth_names=names[:4])
    for b, ((src_image, src_a, src_b), truth) in enumerate(zip(batches, truths)):      # and the pixels are the batch's, not NaN's
        for i in range(n):
            name = f"{b}_{i}.kbf"
            assert np.array_equal(kb.loader.decode_frame(read(os.path.join(roots["packed"], "image", name))), rc.oracle_rgb(src_image, 255.0, 0.0)[i])
            assert np.array_equal(kb.loader.decode_frame(read(os.path.join(roots["packed"], "output_depth", name))), rc.oracle_samples(src_a)[i])
            assert np.array_equal(kb.loader.decode_frame(read(os.path.join(roots["packed"], "sparse_depth", name))), rc.oracle_samples(src_b)[i])
            if b < 2:
                assert np.array_equal(kb.loader.decode_frame(read(os.path.join(roots["packed"], "ground_truth", name))), truth[i])
    assert not [f for d in rc.DIRECTORIES for f in os.listdir(os.path.join(roots["packed"], d)) if ".tmp" in f]


def test_packed_writer_serves_a_short_batch_in_a_larger_slot(dev, tmp_path):
    n, h, w = 3, 5, 67
    sources = rc.make_sources(n, h, w, seed=70)
    on_device = [torch.from_numpy(t).to(dev) for t in sources]
    roots = {fmt: str(tmp_path / fmt) for fmt in ("png", "packed")}
    for fmt, root in roots.items():
        with kb.loader.OutputWriter(root, in_flight=1, file_format=fmt) as writer:
            writer.submit(["a.png", "b.png", "c.png"], *on_device)
            writer.submit(["d.png"], *(t[2:] for t in on_device))      # one frame in the slot of three
    same_outputs(roots["png"], roots["packed"], ["a.png", "b.png", "c.png", "d.png"], truth_names=[])
    for directory in ("image", "output_depth", "sparse_depth"):
        assert read(os.path.join(roots["packed"], directory, "d.kbf")) == read(os.path.join(roots["packed"], directory, "c.kbf"))


# ------------------------------------------------------------------------------------------------ run()
def run(tmp, name, lists=None, **more):
    directory = tmp / name
    directory.mkdir()
    if lists is None:
        lists = [str(directory / n) for n in rc.write_lists(str(directory), kb.loader.write_paths)]
    checkpoint_path = str(directory / "run")
    result = kb.inference.run_with_format(lists[0], lists[1], lists[2], ground_truth_path=lists[3], checkpoint_path=checkpoint_path,
                              depth_model_restore_path=rc.CHECKPOINT, return_results=True, workers=4,
                              **rc.run_settings(kb.kitti_config().narrow()), **more)
    return result, read(os.path.join(checkpoint_path, "results.txt")).decode(), os.path.join(checkpoint_path, "outputs")


def write_list(tmp, name, paths):
    path = str(tmp / name)
    kb.loader.write_paths(path, paths)
    return path


@pytest.fixture(scope="module")
def runs(dev, tmp_path_factory):
    """run() on the three golden frames once per batch size and output format; shared by the tests below, unchanged."""
    tmp = tmp_path_factory.mktemp("packed_runs")
    return tmp, {(bs, fmt): run(tmp, f"{fmt}{bs}", save_outputs=True, batch_size=bs, png_level=1, output_format=fmt)
                 for bs in BATCH_SIZES for fmt in ("png", "packed")}


VARIABLE = re.compile(r"^(Total time: |checkpoint_path=|Saving outputs to )|\.txt$")


@pytest.mark.parametrize("bs", BATCH_SIZES)
def test_run_packed_against_png(runs, bs):
    (png, png_text, png_outputs), (packed, packed_text, packed_outputs) = runs[1][(bs, "png")], runs[1][(bs, "packed")]
    a, b = png_text.splitlines(), packed_text.splitlines()
    assert len(a) == len(b)
    variable = 0
    for x, y in zip(a, b):
        if VARIABLE.search(x):
            assert VARIABLE.search(y).group(0) == VARIABLE.search(x).group(0)
            variable += 1
        else:
            assert x == y
    assert variable == 4 + 3      # the four lists, checkpoint_path, the time line, the outputs' directory
    assert torch.equal(png["per_frame"], packed["per_frame"]) and png["mean"] == packed["mean"] and png["std"] == packed["std"]
    assert torch.equal(png["output_depth"], packed["output_depth"])
    same_outputs(png_outputs, packed_outputs, ["{:010d}.png".format(i) for i in range(rc.N_FRAMES)])


def test_exported_files_feed_a_second_run(runs):
    """Closing the loop: the packed run's output_depth files as sparse depth AND ground truth of a second run (beside packed copies
    of the triplets: a loader batch is all packed or all PNG), the PNG run's files into a third.  Equal metrics, equal depth."""
    tmp, by = runs
    images, _, intrinsics, _ = rc.path_lists()
    packed_images = [str(tmp / f"triplet_{i}.kbf") for i in range(rc.N_FRAMES)]
    kb.loader.pack_frames(images, packed_images, workers=2)
    results = {}
    for fmt, image_paths in (("packed", packed_images), ("png", images)):
        outputs = by[(2, fmt)][2]
        name = "{:010d}.png" if fmt == "png" else "{:010d}.kbf"
        depths = [os.path.join(outputs, "output_depth", name.format(i)) for i in range(rc.N_FRAMES)]
        lists = [write_list(tmp, f"loop_{fmt}_{what}.txt", paths)
                 for what, paths in (("image", image_paths), ("sparse", depths), ("k", intrinsics), ("truth", depths))]
        results[fmt] = run(tmp, f"loop_{fmt}", lists=lists, batch_size=2)[0]
    assert torch.equal(results["png"]["per_frame"], results["packed"]["per_frame"])
    assert results["png"]["mean"] == results["packed"]["mean"] and results["png"]["std"] == results["packed"]["std"]
    assert torch.equal(results["png"]["output_depth"], results["packed"]["output_depth"])
    assert torch.isfinite(results["packed"]["per_frame"]).all()


def test_packed_ground_truth_list(runs):
    """ground_truth_path listing packed copies of depth_*.png: the PNG list's per-frame metrics; a mixed batch is refused, naming
    two of its files."""
    tmp, by = runs
    images, depths, intrinsics, truths = rc.path_lists()
    packed_truths = [str(tmp / f"truth_{i}.kbf") for i in range(rc.N_FRAMES)]
    kb.loader.pack_frames(truths, packed_truths, workers=2)
    head = [write_list(tmp, f"gt_{what}.txt", paths) for what, paths in (("image", images), ("sparse", depths), ("k", intrinsics))]
    for bs in (2, 3):
        got = run(tmp, f"gt_packed{bs}", lists=head + [write_list(tmp, f"gt_packed{bs}.txt", packed_truths)], batch_size=bs)[0]
        assert torch.equal(got["per_frame"], by[(bs, "png")][0]["per_frame"])
        assert torch.equal(got["output_depth"], by[(bs, "png")][0]["output_depth"])
    mixed = [packed_truths[0], truths[1], packed_truths[2]]
    with pytest.raises(KbnError) as refused:
        run(tmp, "gt_mixed", lists=head + [write_list(tmp, "gt_mixed.txt", mixed)], batch_size=3)
    assert mixed[0] in str(refused.value) and mixed[1] in str(refused.value)
    # batches of one kind each are fine: frames 0 and 1 packed, frame 2 a PNG, two a batch
    by_batch = [packed_truths[0], packed_truths[1], truths[2]]
    got = run(tmp, "gt_by_batch", lists=head + [write_list(tmp, "gt_by_batch.txt", by_batch)], batch_size=2)[0]
    assert torch.equal(got["per_frame"], by[(2, "png")][0]["per_frame"])
