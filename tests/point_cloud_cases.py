"""What the point-cloud tests share: the NumPy oracle of ops.point_cloud's records -- with the mistakes the proof of power
plants into it --, the fp64 backprojection, the operator's cases and the golden's case.  Nothing here needs a GPU."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "point_cloud_backproject.npz")
TILE = 1024                      # pixels a workgroup of csrc/point_cloud.hip owns
RECORD = {False: 12, True: 15}   # bytes of a record without and with colour
MISTAKES = ("column_major", "swap_xy", "bgr", "keep_nan", "drop_max", "rank_off_by_one", "z_is_d")


# ------------------------------------------------------------------------------------------------ the oracle
def kept_mask(depth, lo, hi, mistake=None):
    """H x W bool: finite, above 0, inside the closed [lo, hi] -- in float32."""
    d = np.asarray(depth, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        upper = d < np.float32(hi) if mistake == "drop_max" else d <= np.float32(hi)
        keep = (d > 0) & (d >= np.float32(lo)) & upper
        keep &= ~np.isinf(d) if mistake == "keep_nan" else np.isfinite(d)
        if mistake == "keep_nan":
            keep |= np.isnan(d)
    return keep


def oracle_records(depth, coordinates, rgb, lo, hi, mistake=None):
    """One frame's records, as a uint8 array: depth H x W float32, coordinates 3 x H x W float32 (ops.camera_coordinates' frame), rgb
    H x W x 3 uint8 or None.  The kept pixels in row-major order; a point is coordinates * depth, ONE float32 product a component; the
    bytes are float32 x, y, z little-endian, then r, g, b, interleaved without padding.  `mistake`: one of MISTAKES, planted for the
    proof of power."""
    d = np.asarray(depth, dtype=np.float32)
    c = np.asarray(coordinates, dtype=np.float32)
    h, w = d.shape
    keep = kept_mask(d, lo, hi, mistake)
    with np.errstate(invalid="ignore", over="ignore"):
        xyz = np.stack([c[0] * d, c[1] * d, d if mistake == "z_is_d" else c[2] * d], axis=-1).astype(np.float32)      # H x W x 3
    if mistake == "swap_xy":
        xyz = xyz[..., [1, 0, 2]]
    colours = None if rgb is None else np.asarray(rgb, dtype=np.uint8)[..., ::-1 if mistake == "bgr" else 1]
    if mistake == "column_major":
        order = np.flatnonzero(keep.T.reshape(-1))
        rows, cols = order % h, order // h
    else:
        order = np.flatnonzero(keep.reshape(-1))
        rows, cols = order // w, order % w
    if mistake == "rank_off_by_one" and order.size:
        # every pixel from the second tile on lands one record late: the first tile's last record is there twice, the last is lost
        flat = rows * w + cols
        late = int(np.searchsorted(flat, TILE))
        if 0 < late < order.size:
            rows = np.concatenate([rows[:late], rows[late - 1:-1]])
            cols = np.concatenate([cols[:late], cols[late - 1:-1]])
    record = RECORD[rgb is not None]
    out = np.empty((order.size, record), dtype=np.uint8)
    out[:, :12] = np.ascontiguousarray(xyz[rows, cols].astype("<f4")).view(np.uint8).reshape(-1, 12)
    if rgb is not None:
        out[:, 12:] = colours[rows, cols]
    return out.reshape(-1)


def coordinates64(kinv, h, w):
    """K^-1 [x y 1]^T for integer pixel coordinates x = 0 .. w-1 (columns), y = 0 .. h-1 (rows), in float64: N x 3 x h x w."""
    kinv = np.asarray(kinv, dtype=np.float64)
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    grid = np.stack([x, y, np.ones_like(x)], axis=0).reshape(3, -1)
    return np.matmul(kinv, grid).reshape(kinv.shape[0], 3, h, w)


def backproject64(depth, intrinsics):
    """The oracle's fp64 form: N x 1 x H x W depth, N x 3 x 3 intrinsics -> N x 3 x H x W points K^-1 [x y 1]^T z."""
    d = np.asarray(depth, dtype=np.float64)
    n, _, h, w = d.shape
    return coordinates64(np.linalg.inv(np.asarray(intrinsics, dtype=np.float64)), h, w) * d


# ------------------------------------------------------------------------------------------------ the golden's case
def golden_case():
    """2 x 7 x 9, K with skew and different focal lengths a frame: (depth N x 1 x H x W float64, intrinsics N x 3 x 3 float64)."""
    rng = np.random.default_rng(20260)
    depth = rng.uniform(0.5, 80.0, size=(2, 1, 7, 9))
    intrinsics = np.array([[[7.1, 0.35, 4.2], [0.0, 6.4, 3.3], [0.0, 0.0, 1.0]],
                           [[5.3, -0.6, 3.9], [0.0, 8.2, 2.7], [0.0, 0.0, 1.0]]], dtype=np.float64)
    return depth, intrinsics


# ------------------------------------------------------------------------------------------------ the operator's cases
# (name, n, h, w): less than a tile; exactly one; a tile and one pixel with W % 4 != 0; odd H W, so that the second and third planes
# leave the 16-byte phase (its depth is a channel slice with a foreign batch stride); 257 tiles, so that the scan's carry loop runs
SHAPES = (("sub_tile", 1, 5, 7), ("one_tile", 1, 32, 32), ("tile_plus_one", 1, 25, 41), ("odd_planes", 3, 33, 35), ("carry", 1, 513, 512))
DENSITIES = ("all", "none", "random5", "last_pixel", "empty_run")


def intrinsics_for(n, h, w, seed=0):
    """N x 3 x 3 float32: focal lengths near the frame's size, a principal point off the centre, skew, a last row that is not
    (0, 0, 1) in the second frame on (so that c_2 != 1 there)."""
    rng = np.random.default_rng(seed)
    k = np.zeros((n, 3, 3), dtype=np.float32)
    for i in range(n):
        k[i] = [[0.9 * w + rng.uniform(0, 3), 0.2 * (i + 1), 0.48 * w + rng.uniform(0, 1)],
                [0.0, 1.1 * h + rng.uniform(0, 3), 0.53 * h + rng.uniform(0, 1)],
                [0.0, 0.0, 1.0]]
        if i:
            k[i, 2] = [1e-4 * i, -2e-4, 1.0 + 0.01 * i]
    return k


def depth_for(density, n, h, w, seed=0):
    """N x 1 x H x W float32 in (1, 80) where kept, 0 elsewhere."""
    rng = np.random.default_rng(seed)
    full = rng.uniform(1.0, 80.0, size=(n, 1, h, w)).astype(np.float32)
    flat = np.zeros((n, h * w), dtype=bool)
    if density == "all":
        flat[:] = True
    elif density == "random5":
        flat[:] = rng.uniform(size=flat.shape) < 0.05
    elif density == "last_pixel":
        flat[:, -1] = True
    elif density == "empty_run":      # full tiles, a run of empty ones (where the frame has as many), full tiles again
        tiles = -(-h * w // TILE)
        flat[:] = True
        lo, hi = (TILE, (tiles - 1) * TILE) if tiles >= 3 else (h * w // 3, 2 * h * w // 3)
        flat[:, lo:hi] = False
    elif density != "none":
        raise ValueError(density)
    return np.where(flat.reshape(n, 1, h, w), full, np.float32(0.0)).astype(np.float32)


def image_for(n, h, w, seed=0):
    """N x 3 x H x W float32 around [0, 1], a little beyond at both ends."""
    return np.random.default_rng(seed + 1).uniform(-0.05, 1.05, size=(n, 3, h, w)).astype(np.float32)


def tile_phases(counts_per_tile, record):
    """The phases mod 16 at which the payloads of a 16-byte aligned slot's non-empty tiles start."""
    starts = np.concatenate([[0], np.cumsum(counts_per_tile)[:-1]])
    return {int(s * record % 16) for s, c in zip(starts, counts_per_tile) if c}


def tile_counts(keep):
    """Kept pixels of every tile of one frame's H x W mask."""
    flat = np.asarray(keep).reshape(-1)
    pad = -flat.size % TILE
    return np.concatenate([flat, np.zeros(pad, dtype=bool)]).reshape(-1, TILE).sum(axis=1)
