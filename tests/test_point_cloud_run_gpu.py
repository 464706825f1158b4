"""GPU: point clouds of a run.  loader.PointCloudWriter at batch sizes 1, 2 and 3 on the fixtures of tests/run_cases.py
(three frames, ckpt_kitti_narrow.pth), and kb.inference.run_with_point_clouds against run_with_format on the same inputs: the clouds
are the oracle's on the returned depth and on the written PNGs, everything else is byte for byte what run_with_format writes.

    python -m pytest tests/test_point_cloud_run_gpu.py -m gpu -q
"""
import os

import numpy as np
import pytest
import torch

import kbnet_amd as kb
import point_cloud_cases as pc
import run_cases as rc

pytestmark = pytest.mark.gpu
CLOUDS = ("output_depth", "sparse_depth")
DIRECTORY = {"output_depth": "point_cloud", "sparse_depth": "sparse_point_cloud"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def read(path):
    with open(path, "rb") as f:
        return f.read()


# ------------------------------------------------------------------------------------------------ PointCloudWriter
@pytest.fixture(scope="module")
def frames(dev):
    """Three frames of 24 x 40 as a run holds them: normalised image, a dense depth, a sparse depth (30 % of the pixels) with a NaN,
    and another camera a frame."""
    image, depth_a, depth_b = rc.make_sources(3, 24, 40, seed=11)
    depth_a = np.clip(depth_a, 0.5, None)      # make_sources plants what the depth rule needs; a dense cloud wants depths
    depth_a.reshape(-1)[:4] = [np.nan, 0.0, np.inf, -1.0]
    intrinsics = pc.intrinsics_for(3, 24, 40, seed=12)
    return tuple(torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in (image, depth_a, depth_b, intrinsics))


def write_clouds(root, frames, batch_size, **more):
    image, depth_a, depth_b, intrinsics = frames
    names = [f"{i:03d}.png" for i in range(image.shape[0])]
    with kb.loader.PointCloudWriter(root, clouds=CLOUDS, threads=4, in_flight=1, **more) as writer:      # one slot: every batch reuses it
        for at in range(0, len(names), batch_size):
            b = slice(at, at + batch_size)
            writer.submit(names[b], image[b].clone(), depth_a[b].clone(), depth_b[b].clone(), intrinsics[b].clone())
    return names


def test_writer_gives_the_same_files_at_every_batch_size(dev, frames, tmp_path):
    """Batch sizes 1, 2 (a ragged 2 + 1) and 3, and 3 then 1 through one slot (a short batch in a larger slot): the same files, and
    they are the oracle's."""
    roots = {bs: str(tmp_path / f"bs{bs}") for bs in (1, 2, 3)}
    for bs, root in roots.items():
        names = write_clouds(root, frames, bs)
    image, depth_a, depth_b, intrinsics = frames
    with kb.loader.PointCloudWriter(str(tmp_path / "short"), clouds=CLOUDS, in_flight=1) as writer:
        writer.submit(names, image, depth_a, depth_b, intrinsics)
        writer.submit(["again.png"], image[2:], depth_a[2:], depth_b[2:], intrinsics[2:])      # one frame in the slot of three
    kinv = kb.ops.intrinsics_inverse(intrinsics)
    coordinates = kb.ops.camera_coordinates(kinv, 24, 40).cpu().numpy()
    rgb = rc.oracle_rgb(image.cpu().numpy(), 255.0, 0.0)
    for cloud, depth in zip(CLOUDS, (depth_a, depth_b)):
        d = depth.cpu().numpy()
        for i, name in enumerate(names):
            ply = kb.loader.point_cloud_filename(name)
            data = read(os.path.join(roots[1], DIRECTORY[cloud], ply))
            want = pc.oracle_records(d[i, 0], coordinates[i], rgb[i], 0.0, np.inf)
            assert data == kb.loader.ply_header(want.size // 15, True) + want.tobytes(), (cloud, name)
            for bs in (2, 3):
                assert read(os.path.join(roots[bs], DIRECTORY[cloud], ply)) == data, (cloud, name, bs)
            assert read(os.path.join(str(tmp_path / "short"), DIRECTORY[cloud], ply)) == data
        assert read(os.path.join(str(tmp_path / "short"), DIRECTORY[cloud], "again.ply")) == data      # frame 2's
        assert sorted(os.listdir(os.path.join(roots[2], DIRECTORY[cloud]))) == sorted(kb.loader.point_cloud_filename(n) for n in names)
    xyz, colours = kb.loader.load_point_cloud(os.path.join(roots[3], "point_cloud", "000.ply"))
    kept = int(pc.kept_mask(depth_a[0, 0].cpu().numpy(), 0.0, np.inf).sum())      # the planted NaN, Inf, 0 and -1 are gone
    assert 900 < kept <= 24 * 40 - 4 and xyz.shape == (kept, 3) and colours.shape == xyz.shape and np.isfinite(xyz).all()


def test_writer_depth_range_and_one_cloud(dev, frames, tmp_path):
    image, depth_a, depth_b, intrinsics = frames
    root = str(tmp_path / "ranged")
    with kb.loader.PointCloudWriter(root, clouds=["sparse_depth"], depth_range=(10.0, 40.0)) as writer:
        writer.submit(["a.png", "b.png", "c.png"], image, None, depth_b, intrinsics)      # the output depth is not asked for
    assert os.listdir(root) == ["sparse_point_cloud"]
    d = depth_b.cpu().numpy()
    for i, name in enumerate(("a.ply", "b.ply", "c.ply")):
        xyz, _ = kb.loader.load_point_cloud(os.path.join(root, "sparse_point_cloud", name))
        assert len(xyz) == int(((d[i, 0] >= 10.0) & (d[i, 0] <= 40.0)).sum()) and len(xyz) > 0
    with pytest.raises(kb._lib.KbnError):
        writer.submit(["a.png"], image[:1], None, depth_b[:1], intrinsics[:1])      # after close()


# ------------------------------------------------------------------------------------------------ run_with_point_clouds
@pytest.fixture(scope="module")
def runs(dev, tmp_path_factory):
    """run_with_format, then run_with_point_clouds, on the three golden frames with the same arguments and the SAME checkpoint_path
    (the first run's directory is moved aside in between), so that results.txt can be compared line for line."""
    tmp = tmp_path_factory.mktemp("cloud_runs")
    lists = [str(tmp / n) for n in rc.write_lists(str(tmp), kb.loader.write_paths)]
    checkpoint_path = str(tmp / "run")
    common = dict(ground_truth_path=lists[3], checkpoint_path=checkpoint_path, depth_model_restore_path=rc.CHECKPOINT, return_results=True,
                  workers=4, save_outputs=True, batch_size=2, png_level=1, **rc.run_settings(kb.kitti_config().narrow()))
    plain = kb.inference.run_with_format(lists[0], lists[1], lists[2], **common)
    os.rename(checkpoint_path, str(tmp / "plain"))
    clouds = kb.inference.run_with_point_clouds(lists[0], lists[1], lists[2], point_clouds=CLOUDS, **common)
    return lists, (plain, str(tmp / "plain")), (clouds, checkpoint_path)


def test_run_writes_the_clouds(runs):
    lists, _, (result, root) = runs
    outputs = os.path.join(root, "outputs")
    names = ["{:010d}".format(i) for i in range(rc.N_FRAMES)]
    assert sorted(os.listdir(outputs)) == sorted(rc.DIRECTORIES + ("point_cloud", "sparse_point_cloud"))
    for directory in ("point_cloud", "sparse_point_cloud"):
        assert sorted(os.listdir(os.path.join(outputs, directory))) == [n + ".ply" for n in names]
    output_depth = result["output_depth"].numpy()
    n, _, h, w = output_depth.shape
    intrinsics = np.stack([np.load(p).astype(np.float32) for p in rc.path_lists()[2]])
    kinv = kb.ops.intrinsics_inverse(torch.from_numpy(intrinsics).cuda())
    coordinates = kb.ops.camera_coordinates(kinv, h, w).cpu().numpy()
    for i, name in enumerate(names):
        rgb = kb.loader.decode_png(read(os.path.join(outputs, "image", name + ".png")))
        # the output cloud: H W points, the oracle's records on the returned depth, coloured with the image PNG's pixels
        want = pc.oracle_records(output_depth[i, 0], coordinates[i], rgb, 0.0, np.inf)
        data = read(os.path.join(outputs, "point_cloud", name + ".ply"))
        assert data == kb.loader.ply_header(h * w, True) + want.tobytes(), name
        # the sparse cloud: as many points as the sparse depth PNG has positive pixels, with the image PNG's colours there
        samples = kb.loader.decode_png(read(os.path.join(outputs, "sparse_depth", name + ".png")))
        xyz, colours = kb.loader.load_point_cloud(os.path.join(outputs, "sparse_point_cloud", name + ".ply"))
        assert len(xyz) == int((samples > 0).sum()) and 0 < len(xyz) < h * w
        assert np.array_equal(colours, rgb[samples > 0])
        # and its points lie on the output cloud's rays: z = depth, x / z and y / z the pixel's coordinates
        rays = np.transpose(coordinates[i], (1, 2, 0))[samples > 0]
        depth = samples[samples > 0].astype(np.float64) / 256.0
        assert np.abs(xyz - rays * depth[:, None]).max() <= (1.0 / 256.0) * np.abs(rays).max()      # the PNG's quantum: the cloud holds the fp32 depth


def test_run_changes_nothing_else(runs):
    _, (plain, plain_root), (clouds, root) = runs
    for directory in rc.DIRECTORIES:
        a, b = os.path.join(plain_root, "outputs", directory), os.path.join(root, "outputs", directory)
        assert sorted(os.listdir(a)) == sorted(os.listdir(b)) and len(os.listdir(a)) == rc.N_FRAMES
        for name in os.listdir(a):
            assert read(os.path.join(a, name)) == read(os.path.join(b, name)), (directory, name)
    assert sorted(os.listdir(os.path.join(plain_root, "outputs"))) == sorted(rc.DIRECTORIES)
    a = read(os.path.join(plain_root, "results.txt")).decode().splitlines()
    b = read(os.path.join(root, "results.txt")).decode().splitlines()
    assert len(a) == len(b)
    different = [(x, y) for x, y in zip(a, b) if x != y]
    assert all(x.startswith("Total time: ") and y.startswith("Total time: ") for x, y in different) and len(different) <= 1
    assert torch.equal(plain["per_frame"], clouds["per_frame"]) and plain["mean"] == clouds["mean"] and plain["std"] == clouds["std"]
    assert torch.equal(plain["output_depth"], clouds["output_depth"])


def test_run_without_save_outputs_still_writes_the_clouds(runs, tmp_path):
    lists = runs[0]
    checkpoint_path = str(tmp_path / "run")
    kb.inference.run_with_point_clouds(lists[0], lists[1], lists[2], checkpoint_path=checkpoint_path, depth_model_restore_path=rc.CHECKPOINT,
                                       batch_size=2, workers=2, point_cloud_depth_range=(0.0, 1000.0),
                                       **rc.run_settings(kb.kitti_config().narrow()))
    assert os.listdir(os.path.join(checkpoint_path, "outputs")) == ["point_cloud"]
    reference = os.path.join(runs[2][1], "outputs", "point_cloud")
    for name in sorted(os.listdir(reference)):
        assert read(os.path.join(checkpoint_path, "outputs", "point_cloud", name)) == read(os.path.join(reference, name))
