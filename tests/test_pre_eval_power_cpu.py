"""CPU: the comparisons tests/test_pre_eval_gpu.py makes (pre_eval_cases.pre_mismatches / eval_mismatches / unpack_mismatches, at the
GPU tests' own inputs) see every planted mistake: each is injected into a copy of the oracle's computation (mistake=...), the result is
handed to the comparison as if the device had produced it, and the cases named below must each report it.  The unspoilt oracles pass
every case, so a finding is the mistake's and not the comparison's; and the restated outlier removal, which carries the preprocess
mistakes, equals oracle.kbnet_oracle.validity_and_outlier_removal bit for bit on every case."""
import numpy as np
import pytest

import pre_eval_cases as cases

LARGE = "large 1x2049x2048"

# mistake -> the cases whose comparison must catch it (others may as well)
PRE_CATCHERS = {
    "radius_minus_1": ["2x5x3 k3 t1.5", "1x16x64 k15 t0.0", "2x37x130 k7 t1.5", "negative k3"],
    "pad_zero": ["1x1x1 k3 t1.5", "2x5x3 k15 t0.5", "3x33x70 k9 t0.0"],                        # a kept point near the border goes
    "seam64": ["2x17x65 k3 t1.5", "2x37x130 k15 t0.5", "3x33x70 k7 t0.0"],                     # the planted 1.0 | 6.0 across column 64
    "seam16": ["2x17x65 k3 t0.5", "2x37x130 k7 t1.5", "3x33x70 k15 t0.0"],                     # ... and across row 16
    "le": ["1x1x1 k1 t0.0", "2x5x3 k3 t1.5", "1x16x64 k7 t0.5", "2x37x130 k9 t1.5"],           # a minimum exactly at depth - threshold
    "per_frame_max": ["negative k3", "negative k7"],                                           # nothing else can see the fill value
    "binary_validity": ["negative k3", "negative k7", LARGE],
    "max_skips_last": [LARGE],                                                                 # the reduction past its grid cap
}
EVAL_CATCHERS = {
    "closed_bounds": ["bounds"],
    "validity_nonzero": ["validity"],                                                          # -1, -1e-30, -inf and NaN are not > 0
    "fma_terms": ["ulp 1", "ulp 4", "ulp 64"],                                                 # at the count x 2**-51 gate
    "batch_count": ["size 255", "empty frame"],
    "empty_is_zero": ["empty frame"],
}
UNPACK_CATCHERS = {
    "alpha_first": ["n1 h1 w1 c4 raw1 x0 depth u16", "n3 h7 w67 c4 raw201 x67 depth u16"],
    "gray_not_replicated": ["n1 h1 w1 c1 raw1 x0 depth u16", "n3 h7 w64 c1 raw192 x64 depth None"],
    "signed_depth": ["n3 h7 w5 c3 raw15 x5 depth u16", "n3 h7 w64 no image depth u16", "n1 h1 w1 no image depth u16"],
    "x_offset_ignored": ["n1 h1 w1 c3 raw3 x1 depth u16", "n3 h7 w67 c3 raw203 x1 depth u16", "n3 h7 w64 c4 raw192 x128 depth u16"],
    "tail_dropped": ["n1 h1 w1 c3 raw1 x0 depth u16", "n3 h7 w3 c1 raw9 x3 depth u8", "n3 h7 w67 no image depth u8", "n1 h7 w5 c4 raw15 x0 depth u16"],
}


@pytest.fixture(scope="module")
def pre():
    found = {c["name"]: c for c in cases.pre_small_cases() + [cases.pre_large_case()]}
    return found, {name: cases.pre_expected(c) for name, c in found.items()}


@pytest.fixture(scope="module")
def evaluation():
    found = {c["name"]: c for c in cases.eval_small_cases() + [cases.eval_large_case()]}
    return found, {name: cases.eval_expected(c) for name, c in found.items()}, {name: cases.reference_metrics(c) for name, c in found.items()}


@pytest.fixture(scope="module")
def unpack():
    found = {c["name"]: c for c in cases.unpack_all_cases()}
    return found, {name: cases.unpack_expected(c) for name, c in found.items()}


def test_every_mistake_has_catchers():
    assert set(PRE_CATCHERS) == set(cases.PRE_MISTAKES) and all(PRE_CATCHERS.values())
    assert set(EVAL_CATCHERS) == set(cases.EVAL_MISTAKES) and all(EVAL_CATCHERS.values())
    assert set(UNPACK_CATCHERS) == set(cases.UNPACK_MISTAKES) and all(UNPACK_CATCHERS.values())


# --------------------------------------------------------------------------------------------------------------------- preprocess
def test_the_restated_outlier_removal_is_the_oracle_bit_for_bit(pre):
    found, want = pre
    assert len(found) == 6 * 5 * 3 + 2 + 1 + 6 + 1
    for name, case in found.items():
        filtered, validity = cases.outlier_removal(case["sparse"], case["kernel_size"], case["threshold"])
        assert cases.pre_mismatches(case, (want[name][0], validity, filtered), want=want[name]) == [], name


@pytest.mark.parametrize("mistake", cases.PRE_MISTAKES)
def test_preprocess_comparison_catches(pre, mistake):
    found, want = pre
    for name in PRE_CATCHERS[mistake]:
        findings = cases.pre_mismatches(found[name], cases.pre_expected(found[name], mistake=mistake), want=want[name])
        print(f"{mistake} in {name}: {findings}")
        assert findings, (mistake, name)


def test_image_comparison_sees_one_flipped_bit_and_a_doubly_rounded_range(pre):
    found, want = pre
    case = found["image c3 [-1, 1]"]
    image, validity, filtered = want[case["name"]]
    spoilt = image.copy()
    spoilt.view(np.uint32)[1, 2, 16, 64] ^= 1
    assert cases.pre_mismatches(case, (spoilt, validity, filtered), want=want[case["name"]])
    x = case["image"].astype(np.float64)                     # 2 x / 255 - 1 evaluated exactly and rounded once differs somewhere
    assert cases.pre_mismatches(case, ((2.0 * x / 255.0 - 1.0).astype(np.float32), validity, filtered), want=want[case["name"]])
    one = found["image c1 [0, 1]"]                           # x * (1 / 255) in fp32 is not x / 255 for every byte value
    assert cases.pre_mismatches(one, (one["image"] * np.float32(1.0 / 255.0), validity, filtered), want=want[one["name"]])


def test_preprocess_cases_are_not_vacuous(pre):
    """What the GPU tests assert before they compare, here for every case at once: points removed and points kept wherever a window
    can hold two, and the negative-depth cases depending on the batch maximum."""
    found, want = pre
    for name, case in found.items():
        removed, kept = cases.pre_points(case, want[name])
        if int((case["sparse"] != 0).sum()) >= 2 and case["kernel_size"] > 1:
            assert removed >= 1 and kept >= 1, name
    for name, mistake in (("negative k3", "per_frame_max"), ("negative k7", "per_frame_max"), (LARGE, "max_skips_last")):
        assert (cases.pre_expected(found[name], mistake=mistake)[1] != want[name][1]).any(), name


# --------------------------------------------------------------------------------------------------------------------- evaluation
def test_the_unspoilt_evaluation_oracle_passes_every_case(evaluation):
    found, want, reference = evaluation
    for name, case in found.items():
        assert cases.eval_mismatches(case, want[name][0], want=want[name], reference=reference[name]) == [], name
        assert all((want[name][1][i] == 0) == (i in case["empty"]) for i in range(len(want[name][1]))), name
        if case["planted"]:
            assert (cases.eval_masked_out(case) >= 1).all(), name
    assert np.isnan(want["empty frame"][0][1]).all() and np.isnan(reference["empty frame"][1]).all()
    assert np.isposinf(want["zero prediction"][0][1, 2:]).all() and np.isposinf(reference["zero prediction"][1, 2:]).all()


@pytest.mark.parametrize("mistake", cases.EVAL_MISTAKES)
def test_evaluation_comparison_catches(evaluation, mistake):
    found, want, reference = evaluation
    for name in EVAL_CATCHERS[mistake]:
        spoilt = cases.eval_expected(found[name], mistake=mistake)[0]
        findings = cases.eval_mismatches(found[name], spoilt, want=want[name], reference=reference[name])
        print(f"{mistake} in {name}: {findings[:2]}")
        assert findings, (mistake, name)


def test_the_gate_catches_fma_terms_where_the_reference_bound_does_not(evaluation):
    """An FMA in 1000 o - 1000 g moves the MAE of the near-equal cases by 1e-2 .. 5e-6 relative: the 64-ulp case stays inside the
    2e-5 of evaluation_metrics in some frame, and only the count x 2**-51 gate sees it there."""
    found, want, reference = evaluation
    for ulps in (1, 4, 64):
        name = f"ulp {ulps}"
        spoilt = cases.eval_expected(found[name], mistake="fma_terms")[0]
        moved = np.abs(spoilt[:, 0] - want[name][0][:, 0]) / want[name][0][:, 0]
        print(f"{name}: MAE moved by {moved}")
        assert (moved > 1e3 * want[name][1] * cases.EVAL_GATE).all()
        assert (cases.eval_distances(found[name], spoilt, want[name])[1] > 1).any()
    assert (moved < cases.REFERENCE_RTOL).any()


def test_evaluation_comparison_wants_nan_and_inf_in_their_places(evaluation):
    found, want, reference = evaluation
    for name, frame in (("empty frame", 1), ("zero prediction", 1)):
        for value in (0.0, 1.0, np.nan, np.inf):
            spoilt = want[name][0].copy()
            if not (spoilt[frame, 2] == value or (np.isnan(value) and np.isnan(spoilt[frame, 2]))):
                spoilt[frame, 2] = value
                assert cases.eval_mismatches(found[name], spoilt, want=want[name], reference=reference[name]), (name, value)


# ------------------------------------------------------------------------------------------------------------------------- unpack
def test_the_unspoilt_unpack_oracle_passes_every_case(unpack):
    found, want = unpack
    assert len(found) == 3 * (5 * (16 + 3)) + 20
    for name, case in found.items():
        assert cases.unpack_mismatches(case, want[name], want=want[name]) == [], name
    samples = np.concatenate([c["depth_raw"].reshape(-1) for c in found.values() if c["depth_raw"] is not None and c["depth_raw"].dtype == np.uint16])
    assert np.isin(cases.DEPTH_SAMPLES, samples).all()
    assert max(c["quads"] for c in found.values()) > 256


@pytest.mark.parametrize("mistake", cases.UNPACK_MISTAKES)
def test_unpack_comparison_catches(unpack, mistake):
    found, want = unpack
    for name in UNPACK_CATCHERS[mistake]:
        findings = cases.unpack_mismatches(found[name], cases.unpack_expected(found[name], mistake=mistake), want=want[name])
        print(f"{mistake} in {name}: {findings}")
        assert findings, (mistake, name)
