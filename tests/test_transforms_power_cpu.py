"""CPU: the comparison tests/test_transforms_gpu.py makes (transforms_cases.mismatches, at the GPU tests' own inputs) sees every
planted mistake: each is injected into a copy of the oracle's run (transforms_oracle.augment(mistake=...)), the result is handed to
the comparison as if the device had produced it, and the cases named below must each report it.  The unspoilt oracle passes
every case, so a finding is the mistake's and not the comparison's."""
import numpy as np
import pytest

import transforms_cases as tc
import transforms_oracle as to

# mistake -> the cases whose comparison must catch it (others may as well)
CATCHERS = {
    "tie_by_larger_index": ["tie"],                                           # only a tie AT the boundary tells the two orders apart
    "round_k": ["removal edge", "removal 3x1x96x320", "noise uniform"],       # 0.65 x 9 = 5.85 -> 5, not 6
    "candidates_nonzero": ["removal edge", "removal edge flipped", "noise uniform", "noise gaussian"],     # negatives among the points
    "key_by_destination": ["removal edge flipped", "removal 3x1x96x320", "removal c=2"],                   # removal under a flip
    "noise_before_removal": ["noise uniform", "noise gaussian"],
    "second_map_reuses_first": ["removal 3x1x96x320", "noise uniform", "noise gaussian"],                  # two range maps in one call
    "call_ignored": ["removal edge", "removal 3x1x96x320", "removal dense", "removal c=2", "noise uniform", "noise gaussian"],
    "fused_signed_range": ["flip 5x3x19x67", "flip 2x3x6x16", "flip view+4"],                              # the cases normalised to [-1, 1]
}


@pytest.fixture(scope="module")
def cases():
    found = {c["name"]: c for c in tc.all_cases()}
    return found, {name: tc.expected(c) for name, c in found.items()}


def test_every_mistake_has_catchers():
    assert set(CATCHERS) == set(to.MISTAKES)


def test_the_unspoilt_oracle_passes_every_case(cases):
    found, want = cases
    for name, case in found.items():
        assert tc.mismatches(case, want[name][:3], want=want[name]) == [], name


@pytest.mark.parametrize("mistake", to.MISTAKES)
def test_comparison_catches(cases, mistake):
    found, want = cases
    for name in CATCHERS[mistake]:
        case = found[name]
        spoilt = tc.expected(case, mistake=mistake)
        findings = tc.mismatches(case, spoilt[:3], want=want[name])
        print(f"{mistake} in {name}: {findings}")
        assert findings, (mistake, name)


def test_determinism_comparisons_have_something_to_see():
    """The GPU determinism test asserts that the next call differs: at its inputs the oracle's calls 3 and 4 differ in the removed
    set and in the noise, and two maps of one call differ although their data are equal."""
    case = tc.noise_case("uniform")
    a, b = tc.expected(case), tc.expected(case, call=4)
    assert not np.array_equal(a[1][0], b[1][0]) and not np.array_equal(a[3][0][1]["removed"], b[3][0][1]["removed"])
    assert np.array_equal(case["ranges"][0], case["ranges"][1]) and not np.array_equal(a[1][0], a[1][1])
    assert not np.array_equal(a[3][0][1]["removed"], a[3][1][1]["removed"])
