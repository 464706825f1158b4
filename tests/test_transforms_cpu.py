"""CPU: the augmentation oracle (tests/transforms_oracle.py) and the host side of kb.transforms / ops.augment.

The oracle's Philox against the published known answers; the oracle under Transforms.draw's decisions against what the REFERENCE's
Transforms produced (tests/golden/transforms.npz, written by tests/golden/gen_transforms_golden.py; and live where the reference
checkout is present); the statistical properties of the oracle's removal and noise over many seeds; the Gaussian gate; and the
refusals a machine without a GPU can reach.

What can and cannot equal the reference: its decisions (np.random) and densities (torch.rand) are reproduced exactly, its flips and
normalisation bit for bit; WHICH points go and WHAT noise they get come from another generator (Philox here, randperm / randn
there), so those are compared by count, by support and by distribution."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

import kbnet_amd as kb
import transforms_cases as tc
import transforms_oracle as to

KbnError = kb._lib.KbnError
HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE_SRC = "/root/reference/src"
GOLDEN = np.load(os.path.join(HERE, "golden", "transforms.npz"))
RUNS = json.loads(bytes(GOLDEN["runs"]).decode())


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10, and the words differ between counters and between keys."""
    assert [int(w) for w in to.philox4x32_10(0, 0, 0, 0, 0, 0)] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    ones = 0xFFFFFFFF
    assert [int(w) for w in to.philox4x32_10(ones, ones, ones, ones, ones, ones)] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    a = to.philox4x32_10(np.arange(5), 1, 2, 3, 4, 5)
    assert a[0].dtype == np.uint32 and a[0].shape == (5,) and len(set(int(w) for w in a[0])) == 5
    assert int(to.philox4x32_10(3, 1, 2, 3, 4, 5)[0]) == int(a[0][3]) != int(to.philox4x32_10(3, 1, 2, 3, 4, 6)[0])


def _transforms(run, seed=7):
    return kb.transforms.Transforms(normalized_image_range=run["range"], random_flip_type=run["flip"], random_remove_points=run["remove"],
                                    random_noise_type=run["noise"], random_noise_spread=run["spread"], seed=seed)


def _against_reference(run, image, depth, validity, ref_image, ref_depth, ref_validity, ref_densities):
    """The oracle, under Transforms.draw's decisions for the run's NumPy seed, against the reference's outputs."""
    t = _transforms(run)
    np.random.seed(run["np_seed"])
    flags = t.draw(image.shape[0], run["p"])
    np.random.seed(run["np_seed"])
    assert flags == to.draw(image.shape[0], run["p"], t.do_random_horizontal_flip, t.do_random_vertical_flip, t.do_random_remove_points,
                            t.do_random_noise)
    noise_type = run["noise"] if t.do_random_noise else "none"
    images, ranges, validities, info = to.augment([image], [depth], [validity], flags, ref_densities, normalized_image_range=run["range"],
                                                  noise_type=noise_type, noise_spread=run["spread"], seed=t.seed, call=0)
    # images and validity maps: bit-equal (flips and normalisation are deterministic given the decisions)
    assert np.array_equal(images[0].view(np.uint32), ref_image.view(np.uint32)), run["name"]
    assert np.array_equal(validities[0].view(np.uint32), ref_validity.view(np.uint32)), run["name"]
    for b, f in enumerate(flags):
        src = to.flip(depth[b], f)                  # the flipped source frame: what either side started from, in output coordinates
        ref, own = ref_depth[b], ranges[0][b]
        positives = src > 0
        # the range map is flipped like the rest: nothing appears outside the flipped source's positives
        assert not (ref[~positives] != 0).any() and not (own[~positives] != 0).any(), (run["name"], b)
        count = int(positives.sum())
        k = to.removal_count(ref_densities[b], count) if f & to.REMOVE else 0
        assert info[0][b]["count"] == (count if f & to.REMOVE else 0) and info[0][b]["k"] == k
        ref_removed, own_removed = positives & (ref == 0), positives & (own == 0)
        if not f & to.NOISE:      # (a noised survivor is nonzero but for a draw that cancels it exactly)
            assert int(ref_removed.sum()) == k == int(own_removed.sum()), (run["name"], b, k)
            assert np.array_equal(ref[~ref_removed], src[~ref_removed]) and np.array_equal(own[~own_removed], src[~own_removed])
        else:
            assert int(ref_removed.sum()) == k == int(own_removed.sum()), (run["name"], b, k)
            # noise on exactly the surviving positives: every one of them moved, on either side
            assert (ref[positives & ~ref_removed] != src[positives & ~ref_removed]).all(), (run["name"], b)
            assert (own[positives & ~own_removed] != src[positives & ~own_removed]).all(), (run["name"], b)
            if k == 0:          # without removal the two sides noised the very same elements
                assert np.array_equal(ref != src, own != src)
            bound = abs(run["spread"]) * (0.5 if run["noise"] == "uniform" else 6.0) + 1e-5
            assert float(np.abs(own - src)[positives & ~own_removed].max(initial=0.0)) <= bound
    return flags


@pytest.mark.parametrize("run", RUNS, ids=[r["name"] for r in RUNS])
def test_oracle_and_draw_against_the_reference_golden(run):
    g = lambda k: GOLDEN[run["name"] + "::" + k]
    lo, hi = run["remove"]
    densities = ((hi - lo) * torch.from_numpy(g("rand")) + lo).numpy()      # the reference's expression, in torch's fp32
    assert np.array_equal(densities, g("densities"))
    flags = _against_reference(run, GOLDEN["image"], GOLDEN["depth"], GOLDEN["validity"], g("image"), g("depth"), g("validity"), densities)
    if run["p"] == 1.0 and run["name"] != "flips":
        assert any(flags)
    if run["name"].startswith("all"):
        assert 0 in flags and len(set(flags)) >= 3       # p = 0.5: frames left alone beside frames with different decisions


@pytest.mark.skipif(not os.path.isdir(REFERENCE_SRC), reason="needs the reference checkout (build container only)")
@pytest.mark.parametrize("run", RUNS, ids=[r["name"] for r in RUNS])
def test_oracle_and_draw_against_the_imported_reference(run):
    """The same comparison live, on other inputs and seeds than the fixture's."""
    sys.path.insert(0, REFERENCE_SRC)
    try:
        import transforms as ref_transforms
    finally:
        sys.path.remove(REFERENCE_SRC)
    run = dict(run, np_seed=run["np_seed"] + 100, torch_seed=run["torch_seed"] + 100)
    rng = np.random.default_rng(77)
    image = rng.integers(0, 256, size=(5, 3, 7, 10)).astype(np.float32)
    depth = tc._depth(rng, 5, 1, 7, 10, 0.5)
    validity = (depth > 0).astype(np.float32)
    t = ref_transforms.Transforms(normalized_image_range=run["range"], random_flip_type=run["flip"], random_remove_points=run["remove"],
                                  random_noise_type=run["noise"], random_noise_spread=run["spread"])
    torch.manual_seed(run["torch_seed"])
    lo, hi = run["remove"]
    densities = ((hi - lo) * torch.rand(5) + lo).numpy()
    np.random.seed(run["np_seed"])
    torch.manual_seed(run["torch_seed"])
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        [o_image], [o_depth], [o_validity] = t.transform(images_arr=[torch.from_numpy(image.copy())], range_maps_arr=[torch.from_numpy(depth.copy())],
                                                         validity_maps_arr=[torch.from_numpy(validity.copy())],
                                                         random_transform_probability=run["p"])
    _against_reference(run, image, depth, validity, o_image.numpy(), o_depth.numpy(), o_validity.numpy(), densities)


def test_constructor_enables_what_the_reference_enables():
    T = kb.transforms.Transforms
    t = T()
    assert (t.do_random_horizontal_flip, t.do_random_vertical_flip, t.do_random_remove_points, t.do_random_noise) == (False, False, True, False)
    t = T(random_flip_type=["horizontal", "vertical"], random_remove_points=[-1, -1], random_noise_type="gaussian", random_noise_spread=0.1)
    assert (t.do_random_horizontal_flip, t.do_random_vertical_flip, t.do_random_remove_points, t.do_random_noise) == (True, True, False, True)
    assert not T(random_noise_type="gaussian", random_noise_spread=-1).do_random_noise
    assert not T(random_noise_type="none", random_noise_spread=1.0).do_random_noise
    torch.manual_seed(1234)
    assert T().seed == 1234 and T(seed=99).seed == 99 and T().calls == 0
    np.random.seed(5)
    assert T(random_remove_points=[-1, -1]).draw(4, 1.0) == [0, 0, 0, 0]          # nothing enabled: only the first draw is taken
    np.random.seed(5)
    np.random.rand(4)
    rest = np.random.rand(4)
    np.random.seed(5)
    T(random_remove_points=[-1, -1]).draw(4, 1.0)
    assert np.array_equal(np.random.rand(4), rest)
    np.random.seed(6)
    assert T(random_flip_type=["horizontal"]).draw(64, 0.0) == [0] * 64           # p = 0: every decision is ANDed away


# ------------------------------------------------------------------------------------------------ properties over many seeds
SEEDS = 96


def test_removal_takes_exactly_k_positives_uniformly():
    """Over SEEDS seeds on one frame of 40 candidates among negatives and zeros: exactly k removed, only positives, and every
    candidate's removal frequency within 5 binomial standard deviations of k / count."""
    rng = np.random.default_rng(3)
    x = tc._depth(rng, 1, 1, 8, 12, 1.0)[0]
    flat = x.reshape(-1)
    flat[40:70] = 0.0
    flat[70:] *= -1.0
    count, density = 40, 0.65
    k = to.removal_count(density, count)
    assert k == 26
    hits = np.zeros(flat.size)
    for seed in range(SEEDS):
        out, removed, c, kk = to.range_frame(x, 0, 0, to.REMOVE, density, noise_type="none", noise_spread=0.0, seed=1000 + seed, call=seed % 3)
        assert (c, kk) == (count, k) and int(removed.sum()) == k
        assert not removed.reshape(-1)[40:].any()
        assert np.array_equal(out.reshape(-1)[~removed.reshape(-1)], flat[~removed.reshape(-1)]) and not out.reshape(-1)[removed.reshape(-1)].any()
        hits += removed.reshape(-1)
    p = k / count
    sigma = math.sqrt(SEEDS * p * (1 - p))
    assert float(np.abs(hits[:40] - SEEDS * p).max()) <= 5 * sigma, (hits[:40], SEEDS * p, sigma)


@pytest.mark.parametrize("noise_type, variance", [("uniform", 1.0 / 12.0), ("gaussian", 1.0)])
def test_noise_moments(noise_type, variance):
    """Mean within 5 sigma / sqrt(n) and variance within 5 standard errors (sqrt((m4 - sigma^4) / n): kurtosis 1.8 uniform, 3 normal)
    over SEEDS seeds x 96 elements; uniform noise inside [-0.5, 0.5)."""
    draws = np.concatenate([to.noise_values((1, 8, 12), seed % 5, seed % 2, 2000 + seed, seed % 7, noise_type, np.float32).astype(np.float64)
                            for seed in range(SEEDS)])
    n = draws.size
    sigma = math.sqrt(variance)
    assert abs(draws.mean()) <= 5 * sigma / math.sqrt(n)
    kurtosis = 1.8 if noise_type == "uniform" else 3.0
    assert abs(draws.var() - variance) <= 5 * math.sqrt((kurtosis - 1.0) * variance ** 2 / n)
    assert np.isfinite(draws).all()
    if noise_type == "uniform":
        assert draws.min() >= -0.5 and draws.max() < 0.5
    # range maps of one call, and successive calls, get different draws
    a = to.noise_values((1, 8, 12), 0, 0, 1, 0, noise_type, np.float32)
    assert not np.array_equal(a, to.noise_values((1, 8, 12), 0, 1, 1, 0, noise_type, np.float32))
    assert not np.array_equal(a, to.noise_values((1, 8, 12), 0, 0, 1, 1, noise_type, np.float32))
    assert np.array_equal(a, to.noise_values((1, 8, 12), 0, 0, 1, 0, noise_type, np.float32))


def test_gaussian_gate_is_three_times_the_fp32_oracles_distance():
    """GAUSS_GATE = 3 x max |fp32 oracle - fp64 oracle| / spread over the GPU test's Gaussian case, rounded up to one digit."""
    case = tc.noise_case("gaussian")
    w32, w64 = tc.expected(case), tc.expected(case, dtype=np.float64)
    spread = case["options"]["noise_spread"]
    distance = max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(w32[1], w64[1])) / spread
    print(f"fp32 oracle from fp64 oracle: {distance:.3e} x spread; gate {to.GAUSS_GATE:.1e}")
    exponent = math.floor(math.log10(3 * distance))
    assert to.GAUSS_GATE == pytest.approx(math.ceil(3 * distance / 10 ** exponent) * 10 ** exponent, rel=1e-9), distance
    assert tc.mismatches(case, w32[:3], want64=w64) == []
    for a, b in zip(w32[1], w64[1]):
        assert np.array_equal(a == 0, b == 0)


def test_tie_case_premise():
    """The hard-coded seed holds two equal keys, and in fp32 k = r + 1 cuts between them: the smaller index goes, the larger stays."""
    case, r = tc.tie_case()
    key, e = to.removal_keys((1, 192, 640), 0, 0, tc.TIE_SEED, 0)
    order = np.lexsort((e, key))
    assert key[order][r] == key[order][r + 1] and (r == 0 or key[order][r - 1] < key[order][r]) and e[order][r] < e[order][r + 1]
    assert to.removal_count(case["densities"][0], key.size) == r + 1
    removed = tc.expected(case)[3][0][0]["removed"].reshape(-1)
    assert int(removed.sum()) == r + 1 and removed[e[order][r]] and not removed[e[order][r + 1]]


# ------------------------------------------------------------------------------------------------------------ host refusals
def _cpu_inputs(n=2, h=4, w=6):
    return torch.zeros(n, 3, h, w), torch.zeros(n, 1, h, w), torch.zeros(n, 1, h, w)


def test_cpu_tensors_are_refused():
    image, depth, validity = _cpu_inputs()
    with pytest.raises(KbnError, match="no CPU fallback"):
        kb.ops.augment([image], [depth], [validity], [0, 0], None)
    with pytest.raises(KbnError, match="no CPU fallback"):
        kb.transforms.Transforms(random_remove_points=[-1, -1]).transform([image], [depth], [validity])
    with pytest.raises(KbnError):
        kb.transforms.train_inputs(kb.transforms.Transforms(), image, image, image, depth, 1.0)


def test_five_dimensional_input_is_refused_by_dimension_count():
    t = kb.transforms.Transforms(random_remove_points=[-1, -1])
    with pytest.raises(ValueError, match="Unsupported number of dimensions: 5"):
        t.transform([torch.zeros(2, 3, 3, 4, 6)])
    with pytest.raises(ValueError, match="Unsupported number of dimensions: 5"):
        kb.ops.augment([torch.zeros(2, 3, 3, 4, 6)], [], [], [0, 0], None)
    with pytest.raises(ValueError, match="Unsupported number of dimensions: 3"):
        kb.ops.augment([torch.zeros(2, 4, 6)], [], [], [0, 0], None)


def test_bad_range_and_noise_type_are_refused():
    image, depth, validity = _cpu_inputs()
    with pytest.raises(ValueError, match="Unsupported normalization range"):
        kb.ops.augment([image], [depth], [validity], [0, 0], None, normalized_image_range=[0, 2])
    with pytest.raises(ValueError, match="Unsupported normalization range"):
        kb.transforms.Transforms(normalized_image_range=[1, 0], random_remove_points=[-1, -1]).transform([image])
    with pytest.raises(ValueError, match="Unsupported noise type: salt"):
        kb.ops.augment([image], [depth], [validity], [0, 8], None, noise_type="salt", noise_spread=1.0)
    # as in the reference, a bad type is found only when it is first applied: no frame flagged, no complaint about the type
    with pytest.raises(KbnError, match="no CPU fallback"):
        kb.ops.augment([image], [depth], [validity], [0, 0], None, noise_type="salt", noise_spread=1.0)


def test_mismatched_shapes_dtypes_and_flags_are_refused():
    image, depth, validity = _cpu_inputs()
    with pytest.raises(KbnError, match=r"range_maps\[0\] has shape"):
        kb.ops.augment([image], [torch.zeros(2, 1, 4, 7)], [validity], [0, 0], None)
    with pytest.raises(KbnError, match=r"validity_maps\[0\] has shape"):
        kb.ops.augment([image], [depth], [torch.zeros(3, 1, 4, 6)], [0, 0], None)
    with pytest.raises(KbnError, match=r"images\[1\]: expected float32"):
        kb.ops.augment([image, image.double()], [depth], [validity], [0, 0], None)
    with pytest.raises(KbnError, match=r"range_maps\[0\]: expected float32"):
        kb.ops.augment([image], [depth.half()], [validity], [0, 0], None)
    with pytest.raises(KbnError, match="flags"):
        kb.ops.augment([image], [depth], [validity], [0], None)
    with pytest.raises(KbnError, match="flags"):
        kb.ops.augment([image], [depth], [validity], [0, 16], None)
    assert kb.ops.augment([], [], [], [], None) == ([], [], [])


def test_binding_constants_are_the_headers():
    import ctypes
    import re
    header = open(os.path.join(os.path.dirname(HERE), "include", "kbnet_hip.h")).read()
    for name in ("KBN_AUGMENT_ROLE_IMAGE", "KBN_AUGMENT_ROLE_RANGE", "KBN_AUGMENT_ROLE_VALIDITY", "KBN_AUGMENT_RANGE_0_255", "KBN_AUGMENT_RANGE_0_1",
                 "KBN_AUGMENT_RANGE_M1_1", "KBN_AUGMENT_NOISE_NONE", "KBN_AUGMENT_NOISE_GAUSSIAN", "KBN_AUGMENT_NOISE_UNIFORM",
                 "KBN_AUGMENT_STAGE_SELECT", "KBN_AUGMENT_STAGE_APPLY", "KBN_AUGMENT_MAX_FRAMES", "KBN_AUGMENT_WORKSPACE_RECORD_BYTES"):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == getattr(kb._lib, name), name
    assert ctypes.sizeof(kb._lib.AugmentTensor) == kb.ops._AUGMENT_RECORD.size == 64
    assert (kb.ops.AUGMENT_FLIP_HORIZONTAL, kb.ops.AUGMENT_FLIP_VERTICAL, kb.ops.AUGMENT_REMOVE, kb.ops.AUGMENT_NOISE) == (to.FLIP_H, to.FLIP_V, to.REMOVE, to.NOISE)
    lib = kb._lib.load()
    # the workspace: a 16-byte record and 8 bytes an element for every frame of every range map; nothing for the other roles
    table = (kb._lib.AugmentTensor * 3)()
    for slot, (channels, role) in zip(table, ((3, kb._lib.KBN_AUGMENT_ROLE_IMAGE), (2, kb._lib.KBN_AUGMENT_ROLE_RANGE), (1, kb._lib.KBN_AUGMENT_ROLE_RANGE))):
        slot.channels, slot.role = channels, role
    assert lib.kbn_augment_workspace_bytes(table, 3, 3, 4, 5) == 3 * (16 + 8 * 2 * 4 * 5) + 3 * (16 + 8 * 1 * 4 * 5)
    assert lib.kbn_augment_workspace_bytes(table, 1, 3, 4, 5) == 0 and lib.kbn_augment_workspace_bytes(None, 3, 3, 4, 5) == 0
    assert lib.kbn_augment_forward(None, 0, None, 0, 0, 0, None, None, 0, 0, 0, 0.0, 0, 0, 0, None) == kb._lib.KBN_ERR_INVALID_ARGUMENT
