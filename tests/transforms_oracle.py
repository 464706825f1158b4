"""The training augmentation (kb.transforms.Transforms / ops.augment / csrc/augment.hip) restated in NumPy: Philox4x32-10, the
host decisions, and steps (b) to (e) in fp32 with every operation rounded on its own -- the bits the device must produce -- plus
the Gaussian branch in fp64, the gate that follows from the two, and the planted mistakes of tests/test_transforms_power_cpu.py.

    flags       one value a frame: bit 0 horizontal flip, 1 vertical flip (every tensor), 2 remove, 3 noise (range maps only)
    images      [0, 1]: x / 255;  [-1, 1]: 2 (x / 255) - 1, one rounding for the subtraction;  [0, 255]: x
    remove      candidates of frame b of range map i: its elements > 0, over all c H W elements (count of them).  Each has the key
                word 0 of philox(counter = (e, b, call, 0 | i << 8), key = seed), e the element's index in the SOURCE frame
                (plane H W + y W + x, before any flip).  The k = trunc(fp32(density_b) * fp32(count)) candidates with the
                smallest (key, e) become 0.
    noise       after removal: out = (v + spread * noise) * (v > 0 ? 1 : 0); words of philox(counter = (e, b, call, 1 | i << 8)):
                uniform   noise = (w0 >> 8) 2^-24 - 0.5
                gaussian  noise = sqrt(-2 log(((w0 >> 8) + 1) 2^-24)) * cos(2 pi (w1 >> 8) 2^-24)
    flips       last: the output frame is the processed source frame flipped along W and / or H

GAUSS_GATE (the section 8h rule): the device's Gaussian result is compared with the fp64 evaluation of the same
draws, |a - b| <= GAUSS_GATE * spread, where GAUSS_GATE is 3 x the largest |fp32 oracle - fp64 oracle| / spread over the draws of
the GPU test's Gaussian case (transforms_cases.noise_case), rounded up to one digit; test_transforms_cpu measures and asserts it.
"""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
FLIP_H, FLIP_V, REMOVE, NOISE = 1, 2, 4, 8
GAUSS_GATE = 2e-4

MISTAKES = ("tie_by_larger_index", "round_k", "candidates_nonzero", "key_by_destination", "noise_before_removal",
            "second_map_reuses_first", "call_ignored", "fused_signed_range")

_U32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Four uint32 arrays: Philox4x32-10 of the counter words (arrays or numbers, broadcast) under the key (k0, k1)."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) & _U32 for c in (c0, c1, c2, c3)])
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(M0) * c0      # below 2^64: both factors are below 2^32
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & _U32, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & _U32
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def draw(n_batch, probability, horizontal=False, vertical=False, remove=False, noise=False):
    """Flags from np.random.rand in the reference's order (src/transforms.py:94-160): the transform decision, then one draw for each
    enabled branch."""
    do = np.random.rand(n_batch) <= probability
    flags = np.zeros(n_batch, dtype=np.int64)
    for enabled, bit in ((horizontal, FLIP_H), (vertical, FLIP_V), (remove, REMOVE), (noise, NOISE)):
        if enabled:
            flags |= bit * np.logical_and(do, np.random.rand(n_batch) <= 0.50)
    return [int(f) for f in flags]


def normalize(x, normalized_image_range, mistake=None):
    rng = [float(v) for v in normalized_image_range]
    x = np.asarray(x, dtype=np.float32)
    if rng == [0.0, 255.0]:
        return x.copy()
    t = x / np.float32(255.0)
    if rng == [0.0, 1.0]:
        return t
    if rng == [-1.0, 1.0]:
        if mistake == "fused_signed_range":   # x * (2 / 255) - 1 contracted into one fused multiply-subtract
            return (x.astype(np.float64) * np.float64(np.float32(2.0 / 255.0)) - 1.0).astype(np.float32)
        return np.float32(2.0) * t - np.float32(1.0)
    raise ValueError("Unsupported normalization range: {}".format(list(normalized_image_range)))


def flip(frame, flags):
    if flags & FLIP_H:
        frame = frame[..., ::-1]
    if flags & FLIP_V:
        frame = frame[..., ::-1, :]
    return frame


def removal_count(density, count, mistake=None):
    """k = trunc(fp32(density) * fp32(count)): the reference's int(density * n) on an fp32 tensor; never more than count."""
    product = np.float32(density) * np.float32(count)
    if not product >= 1:
        return 0
    k = int(np.round(product)) if mistake == "round_k" else int(product)
    return min(k, int(count))


def removal_keys(shape, b, map_index, seed, call, flags=0, mistake=None):
    """(key, tie-break index) of every element of a c x H x W source frame, flat."""
    c, h, w = shape
    e = np.arange(c * h * w, dtype=np.uint64)
    at = e
    if mistake == "key_by_destination":
        plane, y, x = np.unravel_index(np.arange(c * h * w), shape)
        if flags & FLIP_H:
            x = w - 1 - x
        if flags & FLIP_V:
            y = h - 1 - y
        at = ((plane * h + y) * w + x).astype(np.uint64)
    if mistake == "second_map_reuses_first":
        map_index = 0
    if mistake == "call_ignored":
        call = 0
    key = philox4x32_10(at, b, call, 0 | (map_index << 8), seed & 0xFFFFFFFF, seed >> 32)[0].astype(np.uint64)
    return key, e


def noise_values(shape, b, map_index, seed, call, noise_type, dtype, mistake=None):
    c, h, w = shape
    e = np.arange(c * h * w, dtype=np.uint64)
    if mistake == "second_map_reuses_first":
        map_index = 0
    if mistake == "call_ignored":
        call = 0
    w0, w1, _, _ = philox4x32_10(e, b, call, 1 | (map_index << 8), seed & 0xFFFFFFFF, seed >> 32)
    scale = dtype(2.0 ** -24)
    if noise_type == "uniform":
        return (w0 >> np.uint32(8)).astype(dtype) * scale - dtype(0.5)
    if noise_type == "gaussian":
        u1 = ((w0 >> np.uint32(8)).astype(np.int64) + 1).astype(dtype) * scale
        u2 = (w1 >> np.uint32(8)).astype(dtype) * scale
        two_pi = dtype(np.float32(6.283185307179586)) if dtype is np.float32 else dtype(2.0 * np.pi)
        return np.sqrt(dtype(-2.0) * np.log(u1)) * np.cos(two_pi * u2)
    raise ValueError("Unsupported noise type: {}".format(noise_type))


def range_frame(src, b, map_index, flags, density, *, noise_type, noise_spread, seed, call, dtype=np.float32, mistake=None):
    """One c x H x W frame of a range map through removal and noise, BEFORE the flip.  Returns (frame as `dtype`, removed mask,
    count, k); with dtype float64 the removal is the same and only the noise arithmetic is wider."""
    shape = src.shape
    v = np.asarray(src, dtype=np.float32).reshape(-1).copy()
    removed = np.zeros(v.size, dtype=bool)
    count = k = 0

    def remove(values):
        nonlocal removed, count, k
        base = values if mistake == "noise_before_removal" else src.reshape(-1)      # the right order sees the source values
        cand = np.flatnonzero(base != 0 if mistake == "candidates_nonzero" else base > 0)
        count = cand.size
        k = removal_count(density, count, mistake)
        if k:
            key, e = removal_keys(shape, b, map_index, seed, call, flags, mistake)
            tie = (np.uint64(0xFFFFFFFF) - e) if mistake == "tie_by_larger_index" else e
            order = np.lexsort((tie[cand], key[cand]))      # by key, then by the tie-break index
            removed[cand[order[:k]]] = True
            values[removed] = 0
        return values

    def noise(values):
        n = noise_values(shape, b, map_index, seed, call, noise_type, dtype, mistake)
        mask = np.where(values > 0, dtype(1), dtype(0))
        return (values.astype(dtype) + dtype(noise_spread) * n) * mask

    if mistake == "noise_before_removal":
        if flags & NOISE:
            v = noise(v)
        if flags & REMOVE:
            v = remove(v)
    else:
        if flags & REMOVE:
            v = remove(v)
        if flags & NOISE:
            v = noise(v)
    return v.astype(dtype).reshape(shape), removed.reshape(shape), count, k


def augment(images, range_maps, validity_maps, flags, densities, *, normalized_image_range=(0, 255), noise_type="none", noise_spread=0.0,
            seed=0, call=0, dtype=np.float32, mistake=None):
    """ops.augment on NumPy arrays.  Returns (images, range_maps, validity_maps, info): lists of new arrays, and info[i][b] =
    dict(count, k, removed) for frame b of range map i (removed: the mask in SOURCE coordinates)."""
    assert mistake is None or mistake in MISTAKES, mistake
    flags = [int(f) for f in flags]
    out_images = []
    for x in images:
        y = normalize(x, normalized_image_range, mistake)
        out_images.append(np.stack([flip(y[b], f) for b, f in enumerate(flags)]))
    out_validity = [np.stack([flip(np.asarray(x, dtype=np.float32)[b], f) for b, f in enumerate(flags)]) for x in validity_maps]
    out_ranges, info = [], []
    for i, x in enumerate(range_maps):
        frames, per_frame = [], []
        for b, f in enumerate(flags):
            density = float(densities[b]) if densities is not None else 0.0
            frame, removed, count, k = range_frame(np.asarray(x[b], dtype=np.float32), b, i, f, density, noise_type=noise_type,
                                                   noise_spread=noise_spread, seed=seed, call=call, dtype=dtype, mistake=mistake)
            frames.append(flip(frame, f))
            per_frame.append(dict(count=count, k=k, removed=removed))
        out_ranges.append(np.stack(frames))
        info.append(per_frame)
    return out_images, out_ranges, out_validity, info
