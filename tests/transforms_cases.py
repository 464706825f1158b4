"""The inputs of tests/test_transforms_gpu.py, built once from seeds in NumPy, and the comparison it makes -- shared with
tests/test_transforms_power_cpu.py, which plants mistakes into the oracle at these very inputs and asserts that the comparison
sees each of them.

A case is a dict: images / ranges / validity (lists of N x C x H x W float32 arrays), flags, densities (N float32, or None), and
the keyword arguments of ops.augment under `options`; `left` (optional) asks the GPU test to pass every tensor as a view that starts
`left` elements into the rows of a wider base tensor (an offset, non-contiguous view)."""
import numpy as np

import transforms_oracle as to

SEED = 0x5EED0123456789AB


def _images(rng, n, c, h, w, count=1):
    return [rng.integers(0, 256, size=(n, c, h, w)).astype(np.float32) for _ in range(count)]


def _depth(rng, n, c, h, w, fraction):
    """Sparse depth: about `fraction` of the elements positive (1 .. 80, quantised to 1 / 256 as a 16-bit PNG gives it), the rest 0."""
    z = np.round(rng.uniform(1.0, 80.0, size=(n, c, h, w)) * 256.0) / 256.0
    return np.where(rng.random((n, c, h, w)) < fraction, z, 0.0).astype(np.float32)


def _case(name, images, ranges, validity, flags, densities=None, left=None, **options):
    options.setdefault("seed", SEED)
    options.setdefault("call", 3)
    return dict(name=name, images=images, ranges=ranges, validity=validity, flags=list(flags),
                densities=None if densities is None else np.asarray(densities, dtype=np.float32), left=left, options=options)


def flip_cases():
    rng = np.random.default_rng(11)
    cases = []
    for name, (n, c, h, w), flags, mc, left in (("1x3x5x7", (1, 3, 5, 7), [3], 1, None),
                                                ("5x3x19x67", (5, 3, 19, 67), [0, 1, 2, 3, 1], 1, None),      # all four combinations in one batch
                                                ("2x1x33x130", (2, 1, 33, 130), [2, 1], 2, None),             # two-channel maps
                                                ("2x3x6x16", (2, 3, 6, 16), [1, 3], 1, None),                 # W % 4 == 0, dense: the 16-byte path
                                                ("view+1", (2, 3, 6, 24), [3, 1], 1, 1),                      # misaligned view: the scalar path
                                                ("view+4", (2, 3, 6, 24), [1, 2], 1, 4)):                     # aligned view with padded rows: 16-byte path, strided
        depth = _depth(rng, n, mc, h, w, 0.3)
        cases.append(_case("flip " + name, _images(rng, n, c, h, w, 2), [depth], [(depth > 0).astype(np.float32), depth.copy()], flags,
                           left=left, normalized_image_range=[-1, 1] if len(cases) % 2 else [0, 1]))
    return cases


def removal_edge_case(flips=False):
    """6 x 1 x 9 x 13.  Frame 0: no candidate; 1: one candidate at density 0.7 (k = 0); 2: nine positives among negatives and zeros at
    0.65 (5.85: trunc 5, round 6); 3: density 0.0; 4: density 1.0; 5: no flag."""
    rng = np.random.default_rng(12)
    x = _depth(rng, 6, 1, 9, 13, 0.4)
    x[0] = np.where(x[0] > 0, -x[0], 0.0)
    x[1] = 0.0
    x[1, 0, 4, 5] = 7.5
    positives = np.flatnonzero(x[2].reshape(-1) > 0)
    x[2].reshape(-1)[positives[9:]] *= -1.0
    assert int((x[2] > 0).sum()) == 9 and int((x[2] < 0).sum()) > 3 and int((x[2] == 0).sum()) > 3
    flags = [4 | 1, 4 | 2, 4 | 3, 4, 4 | 1, 1] if flips else [4, 4, 4, 4, 4, 0]
    return _case("removal edge" + (" flipped" if flips else ""), [], [x], [], flags, [0.7, 0.7, 0.65, 0.0, 1.0, 0.65])


def removal_kitti_case():
    """3 x 1 x 96 x 320 with about 5 % positives, two range maps in one call, mixed flags, densities in [0.6, 0.7]."""
    rng = np.random.default_rng(13)
    a, b = _depth(rng, 3, 1, 96, 320, 0.05), _depth(rng, 3, 1, 96, 320, 0.05)
    return _case("removal 3x1x96x320", _images(rng, 3, 3, 96, 320), [a, b], [(a > 0).astype(np.float32)], [4, 0, 4 | 1], [0.6123, 0.65, 0.6987],
                 normalized_image_range=[0, 1])


def removal_dense_case():
    """One fully positive 1 x 1 x 96 x 320 frame: 30 720 candidates."""
    rng = np.random.default_rng(14)
    return _case("removal dense", [], [_depth(rng, 1, 1, 96, 320, 2.0)], [], [4], [0.6543])


def removal_two_channel_case():
    rng = np.random.default_rng(15)
    return _case("removal c=2", [], [_depth(rng, 2, 2, 7, 12, 0.5)], [], [4 | 2, 4], [0.62, 0.7])


TIE_SEED = 1     # found by trying seeds 0 .. 7 on the CPU: 7 of them have an equal pair among their 122 880 keys (3 has none); tie_case finds the pair


def tie_case(seed=TIE_SEED):
    """One fully positive 1 x 1 x 192 x 640 frame whose keys hold two equal ones, with the density that cuts between them:
    k = r + 1, r the number of candidates below the pair.  Returns (case, r) or None when this seed's keys are all distinct."""
    shape = (1, 192, 640)
    key, e = to.removal_keys(shape, 0, 0, seed, 0)
    order = np.lexsort((e, key))
    same = np.flatnonzero(key[order][1:] == key[order][:-1])
    if same.size == 0:
        return None
    r = int(same[0])
    count = key.size
    density = np.float32((r + 1.5) / count)
    x = np.full((1,) + shape, 2.5, dtype=np.float32)
    return _case("tie", [], [x], [], [4], [density], seed=seed, call=0), r


def noise_case(noise_type):
    """4 x 1 x 24 x 40, two range maps (the second equal to the first: only the map index tells their draws apart), negatives, zeros
    and small positives among the points; frames: noise, removal + noise, nothing, noise under both flips."""
    rng = np.random.default_rng(16)
    x = _depth(rng, 4, 1, 24, 40, 0.3)
    x[rng.random(x.shape) < 0.05] = -3.0
    small = (rng.random(x.shape) < 0.1) & (x > 0)
    x[small] = 0.015625
    return _case("noise " + noise_type, [], [x, x.copy()], [(x > 0).astype(np.float32)], [8, 12, 0, 8 | 3], [0.5, 0.64, 0.5, 0.5],
                 noise_type=noise_type, noise_spread=0.5 if noise_type == "uniform" else 0.1)


def all_cases():
    return (flip_cases() + [removal_edge_case(), removal_edge_case(True), removal_kitti_case(), removal_dense_case(), removal_two_channel_case(),
                            tie_case()[0], noise_case("uniform"), noise_case("gaussian")])


def expected(case, dtype=np.float32, mistake=None, **override):
    options = dict(case["options"], **override)
    return to.augment(case["images"], case["ranges"], case["validity"], case["flags"], case["densities"], dtype=dtype, mistake=mistake, **options)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def mismatches(case, got, want=None, want64=None):
    """What the GPU test asserts to be empty: `got` = (images, ranges, validity) as lists of float32 arrays against the oracle's
    fp32 result bit for bit -- but the range maps of a Gaussian case against the fp64 result within GAUSS_GATE * spread, with the
    zeros in the same places.  Returns a list of findings."""
    want = expected(case) if want is None else want
    found = []
    gaussian = case["options"].get("noise_type") == "gaussian" and any(f & to.NOISE for f in case["flags"])
    for role, g_list, w_list in zip(("images", "ranges", "validity"), got[:3], want[:3]):
        if len(g_list) != len(w_list):
            found.append(f"{role}: {len(g_list)} tensors, expected {len(w_list)}")
            continue
        for i, (g, w) in enumerate(zip(g_list, w_list)):
            if g.shape != w.shape:
                found.append(f"{role}[{i}]: shape {g.shape}, expected {w.shape}")
            elif role == "ranges" and gaussian:
                w64 = (expected(case, dtype=np.float64) if want64 is None else want64)[1][i]
                spread = case["options"]["noise_spread"]
                worst = float(np.abs(g.astype(np.float64) - w64).max()) / spread
                if not worst <= to.GAUSS_GATE:
                    found.append(f"{role}[{i}]: {worst:.3e} x spread from the fp64 oracle, gate {to.GAUSS_GATE:.1e}")
                if not np.array_equal(g == 0, w64 == 0):
                    found.append(f"{role}[{i}]: zeros in other places than the oracle's")
            else:
                bad = int((_bits(g) != _bits(w)).sum())
                if bad:
                    found.append(f"{role}[{i}]: {bad} of {g.size} elements differ in bits")
    return found
