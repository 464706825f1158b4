"""No GPU: point clouds.  The oracle of tests/point_cloud_cases.py against the reference's backprojection, the entry
point's refusals, the PLY header and its strict reader, run_with_point_clouds' signature, and the proof that the byte comparison of
tests/test_point_cloud_gpu.py rejects the mistakes a backprojection kernel can make.

    python -m pytest tests/test_point_cloud_cpu.py -q
"""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import kbnet_amd as kb
import point_cloud_cases as pc

KbnError = kb._lib.KbnError


# ------------------------------------------------------------------------------------------------ the oracle and the reference
def test_oracle_fp64_is_the_reference_backprojection():
    """backproject64 against net_utils.backproject_to_camera in float64 (tests/golden/gen_point_cloud_golden.py), to 1e-12 of each
    component's largest value: x is the column, y the row, both integers from 0, and the axes are the reference's."""
    g = np.load(pc.GOLDEN)
    depth, intrinsics = pc.golden_case()
    assert np.array_equal(g["depth"], depth) and np.array_equal(g["intrinsics"], intrinsics)
    got, want = pc.backproject64(depth, intrinsics), g["points"]
    assert got.shape == want.shape == (2, 3, 7, 9)
    for j in range(3):
        error, scale = np.abs(got[:, j] - want[:, j]).max(), np.abs(want[:, j]).max()
        print(f"component {j}: max error {error:.3e}, largest value {scale:.3e}")
        assert error <= 1e-12 * scale, j


def test_oracle_records_are_the_fp32_points_of_the_kept_pixels():
    """The byte oracle against the fp64 form on the golden's case: the same pixels in the same order, every component within the
    roundings of float32 (the coordinates handed in are float32 roundings of the fp64 ones)."""
    depth, intrinsics = pc.golden_case()
    n, _, h, w = depth.shape
    coordinates = pc.coordinates64(np.linalg.inv(intrinsics), h, w).astype(np.float32)
    d32 = depth.astype(np.float32)
    d32[0, 0, 2, 3], d32[1, 0, 0, 0] = 0.0, np.nan
    points = pc.backproject64(d32, intrinsics)
    for i in range(n):
        records = pc.oracle_records(d32[i, 0], coordinates[i], None, 0.0, np.inf)
        xyz = records.view("<f4").reshape(-1, 3)
        keep = pc.kept_mask(d32[i, 0], 0.0, np.inf)
        assert keep.sum() == h * w - 1 and xyz.shape[0] == keep.sum()
        want = np.transpose(points[i], (1, 2, 0))[keep]      # row-major
        assert np.abs(xyz - want).max() <= 4 * 2.0 ** -24 * np.abs(want).max()


# ------------------------------------------------------------------------------------------------ refusals, by status
def test_entry_point_refusals():
    lib = kb._lib.load()
    n, h, w = 2, 3, 5
    need = lib.kbn_point_cloud_workspace_bytes(n, h, w)
    assert need >= 4 * n and need % 16 == 0
    for bad in ((0, h, w), (n, 0, w), (n, h, 0), (-1, h, w), (n, 1 << 16, 1 << 16)):
        assert lib.kbn_point_cloud_workspace_bytes(*bad) == 0, bad
    buffers = {name: (C.c_double * 64)() for name in ("depth", "image", "kinv", "out", "points", "workspace")}      # 8-byte aligned host memory: never reached
    p = {name: C.addressof(b) for name, b in buffers.items()}

    def call(depth=p["depth"], image=p["image"], kinv=p["kinv"], out=p["out"], points=p["points"], workspace=p["workspace"], n=n, h=h, w=w,
             out_stride=h * w * 15, workspace_bytes=need):
        return lib.kbn_point_cloud_forward(depth, h * w, image, 255.0, 0.0, kinv, 0.0, float("inf"), n, h, w, out, out_stride, points,
                                           workspace, workspace_bytes, None)

    invalid, short = kb._lib.KBN_ERR_INVALID_ARGUMENT, kb._lib.KBN_ERR_WORKSPACE
    assert call(depth=None) == invalid and call(kinv=None) == invalid and call(out=None) == invalid
    assert call(points=None) == invalid and call(workspace=None) == invalid
    assert call(n=0) == invalid and call(h=0) == invalid and call(w=0) == invalid and call(n=-3) == invalid
    assert call(out_stride=h * w * 15 - 1) == invalid
    assert call(image=None, out_stride=h * w * 12 - 1) == invalid      # a NULL image alone is legal: the record is 12 bytes then
    assert call(workspace_bytes=need - 1) == short and call(workspace_bytes=0) == short
    assert call(depth=p["depth"] + 2) == invalid and call(points=p["points"] + 4) == invalid


def test_ops_size_functions():
    assert kb.ops.point_cloud_stride(352, 1216, True) == 352 * 1216 * 15 and kb.ops.point_cloud_stride(3, 5, False) == 180
    assert kb.ops.point_cloud_workspace_bytes(8, 352, 1216) == 8 * 418 * 4
    for bad in (lambda: kb.ops.point_cloud_stride(0, 4, True), lambda: kb.ops.point_cloud_workspace_bytes(0, 4, 4)):
        with pytest.raises(KbnError):
            bad()
    with pytest.raises(KbnError):      # no CPU fallback
        import torch
        kb.ops.point_cloud(torch.zeros(1, 1, 2, 2), torch.eye(3)[None])


# ------------------------------------------------------------------------------------------------ header and reader
HEADER_COLOUR = (b"ply\nformat binary_little_endian 1.0\ncomment kbnet_amd point cloud: camera frame, metres\nelement vertex 3\n"
                 b"property float x\nproperty float y\nproperty float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
                 b"end_header\n")


def test_ply_header_text():
    assert kb.loader.POINT_CLOUD_EXTENSION == ".ply"
    assert kb.loader.ply_header(3, True) == HEADER_COLOUR
    assert kb.loader.ply_header(0, False) == (b"ply\nformat binary_little_endian 1.0\ncomment kbnet_amd point cloud: camera frame, metres\n"
                                              b"element vertex 0\nproperty float x\nproperty float y\nproperty float z\nend_header\n")
    with pytest.raises(KbnError):
        kb.loader.ply_header(-1, True)


def host_file(path, xyz, rgb):
    body = np.empty((len(xyz), 12 if rgb is None else 15), dtype=np.uint8)
    body[:, :12] = np.ascontiguousarray(xyz, dtype="<f4").view(np.uint8).reshape(-1, 12)
    if rgb is not None:
        body[:, 12:] = rgb
    data = kb.loader.ply_header(len(xyz), rgb is not None) + body.tobytes()
    with open(path, "wb") as f:
        f.write(data)
    return data


@pytest.mark.parametrize("points, colour", [(5, True), (5, False), (0, True), (0, False), (1, True)])
def test_reader_round_trip(tmp_path, points, colour):
    rng = np.random.default_rng(points)
    xyz = rng.normal(size=(points, 3)).astype(np.float32)
    if points:
        xyz[0, 1] = np.float32(1e-42)      # a denormal survives
    rgb = rng.integers(0, 256, size=(points, 3), dtype=np.uint8) if colour else None
    path = str(tmp_path / "cloud.ply")
    host_file(path, xyz, rgb)
    got_xyz, got_rgb = kb.loader.load_point_cloud(path)
    assert got_xyz.dtype == np.float32 and got_xyz.shape == (points, 3) and np.array_equal(got_xyz.view(np.uint32), xyz.view(np.uint32))
    if colour:
        assert got_rgb.dtype == np.uint8 and np.array_equal(got_rgb, rgb)
    else:
        assert got_rgb is None


def test_reader_is_strict(tmp_path):
    rng = np.random.default_rng(9)
    path = str(tmp_path / "cloud.ply")
    data = host_file(path, rng.normal(size=(4, 3)).astype(np.float32), rng.integers(0, 256, size=(4, 3), dtype=np.uint8))
    kb.loader.load_point_cloud(path)
    foreign = data.replace(b"comment kbnet_amd point cloud: camera frame, metres\n", b"comment made elsewhere\n")
    ascii_ply = data.replace(b"binary_little_endian", b"ascii")
    doubles = data.replace(b"property float x", b"property double x")
    spaced = data.replace(b"element vertex 4", b"element vertex  4")
    signed = data.replace(b"element vertex 4", b"element vertex +4")
    for name, bad in (("truncated body", data[:-1]), ("one trailing byte", data + b"\0"), ("foreign header", foreign), ("ascii", ascii_ply),
                      ("doubles", doubles), ("two spaces", spaced), ("a sign", signed), ("no header", data[60:]), ("empty", b""),
                      ("header alone, four points stated", data[:len(kb.loader.ply_header(4, True))])):
        with open(path, "wb") as f:
            f.write(bad)
        with pytest.raises(KbnError):
            kb.loader.load_point_cloud(path)
        print("refused:", name)


# ------------------------------------------------------------------------------------------------ run_with_point_clouds
def test_signature_is_run_with_format_plus_two_keywords():
    base = inspect.signature(kb.inference.run_with_format).parameters
    got = inspect.signature(kb.inference.run_with_point_clouds).parameters
    names = list(got)
    assert names[:len(base)] == list(base) and names[len(base):] == ["point_clouds", "point_cloud_depth_range"]
    for name, parameter in base.items():
        assert got[name].kind == parameter.kind and got[name].default == parameter.default, name
    for name, default in (("point_clouds", ("output_depth",)), ("point_cloud_depth_range", None)):
        assert got[name].kind is inspect.Parameter.KEYWORD_ONLY and got[name].default == default


@pytest.mark.parametrize("clouds", [(), ("depth",), ("output_depth", "ground_truth"), ("output_depth", "output_depth"), "points", None, [""]])
def test_bad_point_clouds_raise_before_anything_is_touched(tmp_path, clouds):
    checkpoint_path = str(tmp_path / "run")
    with pytest.raises(KbnError):
        kb.inference.run_with_point_clouds(str(tmp_path / "image.txt"), str(tmp_path / "sparse.txt"), str(tmp_path / "k.txt"),
                                           checkpoint_path=checkpoint_path, point_clouds=clouds)
    assert os.listdir(str(tmp_path)) == []
    with pytest.raises(KbnError):
        kb.loader.PointCloudWriter(str(tmp_path / "outputs"), clouds=clouds)
    assert os.listdir(str(tmp_path)) == []


def test_bad_depth_range_raises_before_anything_is_touched(tmp_path):
    with pytest.raises(KbnError):
        kb.inference.run_with_point_clouds(str(tmp_path / "image.txt"), str(tmp_path / "sparse.txt"), str(tmp_path / "k.txt"),
                                           checkpoint_path=str(tmp_path / "run"), point_cloud_depth_range=(5.0, 1.0))
    with pytest.raises(KbnError):
        kb.loader.PointCloudWriter(str(tmp_path / "outputs"), depth_range=(5.0, 1.0))
    assert os.listdir(str(tmp_path)) == []


def test_point_cloud_names_and_file_names():
    assert kb.loader.point_cloud_names(["sparse_depth", "output_depth"]) == ("sparse_depth", "output_depth")
    assert kb.loader.point_cloud_names("sparse_depth") == ("sparse_depth",)
    assert kb.loader.point_cloud_filename("0000000003.png") == "0000000003.ply" and kb.loader.point_cloud_filename("a.b.png") == "a.b.ply"


# ------------------------------------------------------------------------------------------------ the power of the byte comparison
def power_case():
    """Two frames of 40 x 41 (1640 pixels: a tile boundary inside), the second with c_2 != 1; depths with a NaN, an Inf, zeros and
    pixels exactly at the range's ends; an image whose channels differ."""
    n, h, w = 2, 40, 41
    kinv = np.linalg.inv(pc.intrinsics_for(n, h, w, seed=3).astype(np.float64))
    coordinates = pc.coordinates64(kinv, h, w).astype(np.float32)
    depth = pc.depth_for("all", n, h, w, seed=4)
    depth[:, 0, 3, 5], depth[:, 0, 7, 1], depth[:, 0, 20, 20], depth[:, 0, 30, 2] = np.nan, np.inf, 0.0, -1.0
    depth[:, 0, 9, 9], depth[:, 0, 35, 40] = 1.0, 80.0      # the ends of the range used below
    rgb = np.random.default_rng(5).integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    return depth, coordinates, rgb, 1.0, 80.0


def test_the_case_has_what_the_mistakes_need():
    depth, coordinates, rgb, lo, hi = power_case()
    assert np.all(coordinates[0, 2] == 1.0) and np.all(coordinates[1, 2] != 1.0)
    keep = pc.kept_mask(depth[1, 0], lo, hi)
    assert keep[9, 9] and keep[35, 40] and not keep[3, 5] and not keep[7, 1] and not keep[20, 20] and not keep[30, 2]
    counts = pc.tile_counts(keep)
    assert len(counts) == 2 and counts[0] and counts[1]


@pytest.mark.parametrize("mistake", pc.MISTAKES)
def test_byte_comparison_rejects(mistake):
    depth, coordinates, rgb, lo, hi = power_case()
    frame = 1      # c_2 != 1 there
    want = pc.oracle_records(depth[frame, 0], coordinates[frame], rgb[frame], lo, hi)
    assert np.array_equal(want, pc.oracle_records(depth[frame, 0].copy(), coordinates[frame].copy(), rgb[frame].copy(), lo, hi))
    wrong = pc.oracle_records(depth[frame, 0], coordinates[frame], rgb[frame], lo, hi, mistake=mistake)
    assert wrong.shape != want.shape or not np.array_equal(wrong, want), mistake
    if mistake in ("column_major", "swap_xy", "bgr", "rank_off_by_one", "z_is_d"):      # these keep the count: only the bytes tell
        assert wrong.shape == want.shape
