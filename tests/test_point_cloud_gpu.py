"""GPU: ops.point_cloud (kbn_point_cloud_forward, csrc/point_cloud.hip) is byte for byte the NumPy oracle of
tests/point_cloud_cases.py on the coordinates ops.camera_coordinates gives for the same inverse intrinsics -- over shapes below, at
and past a tile, planes off the 16-byte phase, a channel slice, the scan's carry loop, five densities, with and without colour --
inside guarded buffers: nothing past count * record of a slot, nothing past the stated workspace, nothing between the slots.

    python -m pytest tests/test_point_cloud_gpu.py -m gpu -q
"""
import functools

import numpy as np
import pytest
import torch

import kbnet_amd as kb
import point_cloud_cases as pc
import run_cases as rc

pytestmark = pytest.mark.gpu
KbnError = kb._lib.KbnError
GUARD_BYTE = 0xA5
SLOT_GUARD = 49      # bytes between the slots: odd, so that the slots of a batch start at different phases mod 16
SCALE, SHIFT = 255.0, 0.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def inputs(shape_name, density):
    """(depth N x 1 x H x W, intrinsics N x 3 x 3, image N x 3 x H x W) float32, the same for every test that asks."""
    _, n, h, w = next(s for s in pc.SHAPES if s[0] == shape_name)
    seed = 100 * [s[0] for s in pc.SHAPES].index(shape_name) + pc.DENSITIES.index(density)
    return pc.depth_for(density, n, h, w, seed), pc.intrinsics_for(n, h, w, seed), pc.image_for(n, h, w, seed)


def guarded_depth(dev, depth, channel_slice):
    """The depth on the device with NaN around it: inside a flat buffer, 64 floats from either end, or (channel_slice) as channel 1
    of an N x 3 x H x W tensor -- dense planes with a foreign batch stride."""
    n, _, h, w = depth.shape
    if channel_slice:
        wide = torch.full((n, 3, h, w), float("nan"), device=dev)
        wide[:, 1:2] = torch.from_numpy(depth).to(dev)
        return wide[:, 1:2]
    flat = torch.full((n * h * w + 128,), float("nan"), device=dev)
    flat[64:64 + n * h * w] = torch.from_numpy(depth).to(dev).reshape(-1)
    return flat[64:64 + n * h * w].view(n, 1, h, w)


def launch(dev, depth, kinv, image, lo, hi):
    """ops.point_cloud into 0xA5-filled buffers -> (the whole slot buffer N x (stride + guard), points, the whole workspace buffer,
    the stated workspace size), on the host."""
    n, _, h, w = depth.shape
    stride = kb.ops.point_cloud_stride(h, w, image is not None)
    need = kb.ops.point_cloud_workspace_bytes(n, h, w)
    slots = torch.full((n, stride + SLOT_GUARD), GUARD_BYTE, dtype=torch.uint8, device=dev)
    work = torch.full((need + 256,), GUARD_BYTE, dtype=torch.uint8, device=dev)
    points = torch.full((n,), -1, dtype=torch.int64, device=dev)
    assert slots.data_ptr() % 16 == 0      # the phases test_tile_phases counts are those of the run
    records, counts = kb.ops.point_cloud(depth, kinv, image, min_depth=lo, max_depth=hi, scale=SCALE, shift=SHIFT, out=slots[:, :stride],
                                         out_points=points, workspace=work[:need])
    assert records.data_ptr() == slots.data_ptr() and counts.data_ptr() == points.data_ptr()
    torch.cuda.synchronize()
    return slots.cpu().numpy(), points.cpu().numpy(), work.cpu().numpy(), need


def check_against_oracle(dev, depth, intrinsics, image, lo, hi, channel_slice=False):
    """One guarded call against the oracle, frame by frame; a second call gives the same bytes.  -> the records of every frame."""
    n, _, h, w = depth.shape
    colour = image is not None
    record = pc.RECORD[colour]
    kinv = kb.ops.intrinsics_inverse(torch.from_numpy(intrinsics).to(dev))
    coordinates = kb.ops.camera_coordinates(kinv, h, w).cpu().numpy()
    on_device = guarded_depth(dev, depth, channel_slice)
    image_t = torch.from_numpy(image).to(dev) if colour else None
    rgb = rc.oracle_rgb(image, SCALE, SHIFT) if colour else None
    slots, points, work, need = launch(dev, on_device, kinv, image_t, lo, hi)
    frames = []
    for i in range(n):
        want = pc.oracle_records(depth[i, 0], coordinates[i], rgb[i] if colour else None, lo, hi)
        assert points[i] == want.size // record, (i, points[i], want.size // record)
        assert np.array_equal(slots[i, :want.size], want), i
        assert np.all(slots[i, want.size:] == GUARD_BYTE), i      # the rest of the slot and the guard behind it
        frames.append(want)
    assert np.all(work[need:] == GUARD_BYTE)
    again = launch(dev, on_device, kinv, image_t, lo, hi)
    assert np.array_equal(again[0], slots) and np.array_equal(again[1], points)
    return frames


@pytest.mark.parametrize("colour", [True, False], ids=["xyzrgb", "xyz"])
@pytest.mark.parametrize("shape_name", [s[0] for s in pc.SHAPES])
def test_records_are_the_oracles(dev, shape_name, colour):
    for density in pc.DENSITIES:
        depth, intrinsics, image = inputs(shape_name, density)
        frames = check_against_oracle(dev, depth, intrinsics, image if colour else None, 0.0, float("inf"),
                                      channel_slice=shape_name == "odd_planes")
        kept = [f.size // pc.RECORD[colour] for f in frames]
        pixels = depth.shape[2] * depth.shape[3]
        if density == "all":
            assert kept == [pixels] * len(frames)
        elif density == "none":
            assert kept == [0] * len(frames)
        elif density == "last_pixel":
            assert kept == [1] * len(frames)


def test_tile_phases():
    """Of the inputs above: over the cases, the payloads of the tiles start at all 16 phases mod 16 (the slot buffers are 16-byte
    aligned, launch() asserts it, and frame i's slot starts i * (stride + SLOT_GUARD) bytes in)."""
    seen = {True: set(), False: set()}
    for shape_name, n, h, w in pc.SHAPES:
        for density in pc.DENSITIES:
            depth = inputs(shape_name, density)[0]
            for colour in (True, False):
                record = pc.RECORD[colour]
                for i in range(n):
                    counts = pc.tile_counts(pc.kept_mask(depth[i, 0], 0.0, np.inf))
                    base = i * (h * w * record + SLOT_GUARD)
                    seen[colour] |= {(base + p) % 16 for p in pc.tile_phases(counts, record)}
    assert seen[True] == set(range(16))
    assert seen[False] - {0, 4, 8, 12}      # and 12-byte records meet phases off the dword grid


def planted_depth():
    """1 x 26 x 41 (a tile and 42 pixels), all pixels in (1, 80), with everything that must be dropped planted over both tiles, the
    range's ends hit exactly and missed by one ulp."""
    depth = pc.depth_for("all", 1, 26, 41, seed=77)
    flat = depth.reshape(-1)
    lo, hi = np.float32(2.0), np.float32(50.0)
    planted = [np.nan, np.inf, -np.inf, 0.0, -0.0, -3.5, -1e-42, 1e-42, 1.4e-45, lo, hi, np.nextafter(lo, np.float32(0)),
               np.nextafter(hi, np.float32(100)), np.nextafter(lo, np.float32(100)), np.nextafter(hi, np.float32(0)),
               np.finfo(np.float32).max, np.finfo(np.float32).tiny]
    values = np.asarray(planted, dtype=np.float32)
    flat[5:5 + values.size] = values
    flat[1024 - 3:1024 - 3 + values.size] = values      # across the tile boundary
    flat[-1] = hi
    return depth, values, float(lo), float(hi)


@pytest.mark.parametrize("colour", [True, False], ids=["xyzrgb", "xyz"])
def test_dropped_values_and_range_ends(dev, colour):
    depth, values, lo, hi = planted_depth()
    intrinsics, image = pc.intrinsics_for(1, 26, 41, seed=78), pc.image_for(1, 26, 41, seed=78)
    keep = pc.kept_mask(depth[0, 0], lo, hi).reshape(-1)[5:5 + values.size]
    # the oracle's own reading of the planted values: only the two ends and their inner neighbours stay
    assert keep.tolist() == [False] * 9 + [True, True, False, False, True, True, False, False]
    check_against_oracle(dev, depth, intrinsics, image if colour else None, lo, hi)
    # with the open range every finite depth above 0 stays, the denormals and the largest float among them
    keep = pc.kept_mask(depth[0, 0], 0.0, np.inf).reshape(-1)[5:5 + values.size]
    assert keep.tolist() == [False] * 7 + [True, True] + [True] * 8
    check_against_oracle(dev, depth, intrinsics, image if colour else None, 0.0, float("inf"))


def test_fp64_bound(dev):
    """Against the fp64 backprojection under the fp64 inverse of K, every component within 6 * 2^-24 * (|k0 x| + |k1 y| + |k2|) * d:
    the fp32 rounding of the inverse's three entries (one 2^-24 of each term), of the product k0 x, of the FMA, of the sum and of the
    product with d -- five half-ulp roundings of quantities no larger than the sum of magnitudes, second-order terms under the sixth."""
    shape_name = "odd_planes"
    depth, intrinsics, _ = inputs(shape_name, "all")
    n, _, h, w = depth.shape
    kinv64 = np.linalg.inv(intrinsics.astype(np.float64))
    want = pc.backproject64(depth, intrinsics)
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    magnitude = np.stack([np.abs(kinv64[:, j, 0, None, None] * x) + np.abs(kinv64[:, j, 1, None, None] * y) + np.abs(kinv64[:, j, 2, None, None])
                          for j in range(3)], axis=1)      # N x 3 x H x W
    bound = 6.0 * 2.0 ** -24 * magnitude * depth.astype(np.float64)
    frames = check_against_oracle(dev, depth, intrinsics, None, 0.0, float("inf"), channel_slice=True)
    for i, records in enumerate(frames):
        got = records.view("<f4").reshape(h, w, 3).astype(np.float64)
        error = np.abs(got - np.transpose(want[i], (1, 2, 0)))
        ratio = (error / np.transpose(bound[i], (1, 2, 0))).max()
        print(f"frame {i}: largest error / bound {ratio:.3f}")
        assert ratio <= 1.0, i


def test_refusals_name_the_offender(dev):
    depth = torch.ones((2, 1, 4, 6), device=dev)
    kinv = torch.eye(3, device=dev).repeat(2, 1, 1)
    stride = kb.ops.point_cloud_stride(4, 6, False)
    for bad in (lambda: kb.ops.point_cloud(depth.cpu(), kinv), lambda: kb.ops.point_cloud(depth, kinv[:1]),
                lambda: kb.ops.point_cloud(depth, kinv, torch.ones((2, 3, 4, 5), device=dev)),
                lambda: kb.ops.point_cloud(depth, kinv, out=torch.empty((2, stride - 1), dtype=torch.uint8, device=dev)),
                lambda: kb.ops.point_cloud(depth, kinv, out_points=torch.empty((2,), dtype=torch.int32, device=dev)),
                lambda: kb.ops.point_cloud(depth, kinv, workspace=torch.empty((4,), dtype=torch.uint8, device=dev)),
                lambda: kb.ops.point_cloud(depth.double(), kinv)):
        with pytest.raises(KbnError):
            bad()
    records, points = kb.ops.point_cloud(depth[:, 0], kinv)      # N x H x W is welcome
    assert tuple(records.shape) == (2, stride) and points.tolist() == [24, 24]


def test_profile_entry(dev):
    depth, intrinsics, image = inputs("one_tile", "all")
    kinv = kb.ops.intrinsics_inverse(torch.from_numpy(intrinsics).to(dev))
    kb.ops.PROFILE = []
    try:
        kb.ops.point_cloud(torch.from_numpy(depth).to(dev), kinv, torch.from_numpy(image).to(dev))
        (name, work, executed, pipe, nbytes, start, end), = kb.ops.PROFILE
    finally:
        kb.ops.PROFILE = None
    assert name == "point_cloud" and work == 0.0 and nbytes == 1024 * (8 + 12 + 15)
