"""GPU: the three small kernels every reported frame passes through -- ops.preprocess (csrc/pre_eval.hip, kbn_preprocess_forward),
ops.eval_metrics (kbn_eval_accumulate) and ops.unpack_frames (csrc/unpack.hip) -- against the oracles of tests/pre_eval_cases.py at its
cases: every window size the header promises, partial tiles, ties at the threshold, negative depths (the only inputs that show the
batch-global fill), both reductions past their grid caps, mask boundaries, poisoned masked-out pixels, empty frames, every channel
count, row tail and column offset of the unpacking.  Bit for bit, but the four metrics, which are held to cases.EVAL_GATE x count
against the float64 sum of the same fp32 terms and to the 2e-5 of test_eval_metrics_golden against evaluation_metrics.
tests/test_pre_eval_power_cpu.py shows that these comparisons see the mistakes worth making.

    python -m pytest tests/test_pre_eval_gpu.py -m gpu -q
"""
import numpy as np
import pytest
import torch

import kbnet_amd as kb
import pre_eval_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need a visible MI355X (run with -m gpu on a GPU box)")
    kb._lib.load()   # a missing extension is an error on a GPU box, never a skip
    return torch.device("cuda:0")


def _host(t):
    return None if t is None else t.cpu().numpy()


# --------------------------------------------------------------------------------------------------------------------- preprocess
def _preprocess(case, dev, order=None):
    """ops.preprocess on the case (its frames in `order`): (image or None, validity, filtered) as NumPy arrays."""
    pick = slice(None) if order is None else list(order)
    sparse = torch.from_numpy(case["sparse"][pick]).to(dev)
    image = None if case["image"] is None else torch.from_numpy(case["image"][pick]).to(dev)
    got = kb.ops.preprocess(image, sparse, case["kernel_size"], case["threshold"], normalized_image_range=case["range"])
    torch.cuda.synchronize()
    assert torch.equal(sparse.cpu(), torch.from_numpy(case["sparse"][pick]))       # the input is left alone
    return [_host(t) for t in got]


def _check_preprocess(case, dev):
    want = cases.pre_expected(case)
    removed, kept = cases.pre_points(case, want)
    print(f"{case['name']}: {removed} points removed, {kept} kept")
    if int((case["sparse"] != 0).sum()) >= 2 and case["kernel_size"] > 1:     # a lone point is its own window's minimum: it stays
        assert removed >= 1 and kept >= 1, (case["name"], removed, kept)
    found = cases.pre_mismatches(case, _preprocess(case, dev), want=want)
    assert found == [], (case["name"], found)
    return want


@pytest.mark.parametrize("shape", cases.PRE_SHAPES, ids=cases.pre_shape_name)
def test_preprocess_every_window_and_threshold(dev, shape):
    """Kernel sizes 1 .. 15 (radius 0 .. PRE_MAXR) and thresholds with exact ties, from one pixel to two partial tiles each way."""
    for case in cases.pre_grid_cases(shape):
        _check_preprocess(case, dev)


@pytest.mark.parametrize("make", [lambda: cases.pre_negative_cases()[0], lambda: cases.pre_negative_cases()[1], cases.pre_large_case],
                         ids=["negative k3", "negative k7", "large 1x2049x2048"])       # the large case is built when it runs
def test_preprocess_negative_depths_show_the_batch_maximum(dev, make):
    """Negative depths pass through as negative validity, and under a negative threshold the result depends on the fill
    10 x max(batch): a per-frame maximum -- or, in the large case, a reduction that misses the last element -- changes it."""
    case = make()
    want = _check_preprocess(case, dev)
    other = cases.pre_expected(case, mistake="max_skips_last" if case["kind"] == "large" else "per_frame_max")
    differing = int((other[1] != want[1]).sum())
    print(f"{case['name']}: {differing} pixels depend on the batch maximum")
    assert differing > 0
    assert (want[1] < 0).any() and (want[2][want[1] < 0] > 0).all()      # validity = depth < 0 survives, filtered = depth x depth


def test_preprocess_all_zero_batch(dev):
    want = _check_preprocess(cases.pre_zero_case(), dev)
    assert not want[1].any() and not want[2].any()


@pytest.mark.parametrize("case", cases.pre_image_cases(), ids=lambda c: c["name"])
def test_preprocess_image_normalisation(dev, case):
    """One and three channels, every byte value and non-integers between them, in the three ranges of --normalized_image_range."""
    image = case["image"]
    assert all(np.isin(np.arange(256), image[:, ch]).all() for ch in range(image.shape[1])) and (image != np.round(image)).any()
    _check_preprocess(case, dev)


@pytest.mark.parametrize("case", [cases.pre_grid_cases((3, 33, 70))[7]] + cases.pre_negative_cases()[:1], ids=lambda c: c["name"])
def test_preprocess_permuted_frames(dev, case):
    """The fill is the batch's maximum, so the frames' order cannot matter: permuting them permutes the outputs bit for bit."""
    _, validity, filtered = _preprocess(case, dev)
    for order in ((2, 0, 1), (1, 2, 0), (0, 2, 1)):
        _, v, f = _preprocess(case, dev, order)
        assert np.array_equal(v.view(np.uint32), validity[list(order)].view(np.uint32)), order
        assert np.array_equal(f.view(np.uint32), filtered[list(order)].view(np.uint32)), order


def test_preprocess_refusals(dev):
    """As include/kbnet_hip.h documents them: kernel_size odd and >= 1 or KBN_ERR_INVALID_ARGUMENT, past 15 KBN_ERR_UNSUPPORTED."""
    sparse = torch.from_numpy(cases.pre_grid_cases((2, 5, 3))[0]["sparse"]).to(dev)
    for kernel_size in (2, 4, 8, 16, 0, -1, -3):
        with pytest.raises(kb._lib.KbnError, match=rf"status {kb._lib.KBN_ERR_INVALID_ARGUMENT}\)"):
            kb.ops.preprocess(None, sparse, kernel_size=kernel_size)
    with pytest.raises(kb._lib.KbnError, match=rf"status {kb._lib.KBN_ERR_UNSUPPORTED}\)"):
        kb.ops.preprocess(None, sparse, kernel_size=17)
    image = torch.zeros(2, 3, 5, 3, device=dev)
    for value_range in ([0, 2], [1, 0], [-1, 255]):
        with pytest.raises(ValueError):
            kb.ops.preprocess(image, sparse, normalized_image_range=value_range)
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------------------------------------- evaluation
def _lay_out(x, layout, dev):
    t = torch.from_numpy(x).to(dev)                      # N x H x W
    if layout == "nhw":
        return t
    if layout == "n1hw":
        return t[:, None]
    n, h, w = t.shape
    base = torch.full((n, 1, h + 2, w + 8), float("nan"), device=dev)
    view = base[:, :, 1:1 + h, 3:3 + w]
    view.copy_(t[:, None])
    assert not view.is_contiguous()
    return view


def _check_eval(case, dev):
    want = cases.eval_expected(case)
    counts = want[1]
    for i in range(len(counts)):
        assert (counts[i] == 0) == (i in case["empty"]), (case["name"], i, counts[i])
    if case["planted"]:
        assert (cases.eval_masked_out(case) >= 1).all()
    got = kb.ops.eval_metrics(*[_lay_out(case[k], case["layout"], dev) for k in ("output_depth", "ground_truth", "validity")],
                              case["dmin"], case["dmax"])
    assert got.dtype == torch.float64 and got.shape == (len(counts), 4)
    got = got.cpu().numpy()
    relative, in_gates = cases.eval_distances(case, got, want)
    print(f"{case['name']}: counts {counts.astype(int).tolist()}, worst distance from the float64 oracle {relative.max(initial=0.0):.3e} relative = "
          f"{in_gates.max(initial=0.0):.3e} x count x 2**-51")
    found = cases.eval_mismatches(case, got, want=want)
    assert found == [], (case["name"], found)
    return got


@pytest.mark.parametrize("case", cases.eval_small_cases() + [cases.eval_large_case], ids=lambda c: "large 1x1025x1024" if callable(c) else c["name"])
def test_eval_metrics(dev, case):
    case = case() if callable(case) else case       # the large case is built when it runs
    got = _check_eval(case, dev)
    if case["name"] == "empty frame":
        assert np.isnan(got[1]).all() and np.isfinite(got[[0, 2]]).all()
    if case["name"] == "zero prediction":
        assert np.isfinite(got[1, :2]).all() and np.isposinf(got[1, 2:]).all()


# ------------------------------------------------------------------------------------------------------------------------- unpack
def _unpack(case, dev):
    """ops.unpack_frames on the case.  Its outputs come from torch.empty: a block of each output's size is filled with the sentinel
    and freed first, so that an element the kernel leaves unwritten does not hold an earlier call's (equal) value."""
    n, h, w = (case["image_u8"].shape[:2] if case["image_u8"] is not None else case["depth_raw"].shape[:2]) + (case["width"],)
    image_u8 = None if case["image_u8"] is None else torch.from_numpy(case["image_u8"]).to(dev)
    depth_raw = case["depth_raw"]
    if depth_raw is not None:
        depth_raw = torch.from_numpy(depth_raw.view(np.int16) if depth_raw.dtype == np.uint16 else depth_raw).to(dev)
    torch.cuda.synchronize()
    for shape in [(n, 3, h, w)] * (image_u8 is not None) + [(n, 1, h, w)] * (depth_raw is not None):
        junk = torch.full(shape, float(cases.SENTINEL), device=dev)
        del junk
    image, depth = kb.ops.unpack_frames(image_u8, depth_raw, width=case["width"] if image_u8 is not None else None, x_offset=case["x_offset"])
    torch.cuda.synchronize()
    return _host(image), _host(depth)


def _check_unpack(group, dev):
    for case in group:
        found = cases.unpack_mismatches(case, _unpack(case, dev))
        assert found == [], (case["name"], found)


@pytest.mark.parametrize("c", [1, 3, 4])
def test_unpack_frames_image_cases(dev, c):
    group = cases.unpack_cases(c)
    assert max(case["quads"] for case in group) > 256 > min(case["quads"] for case in group)
    samples = np.concatenate([case["depth_raw"].reshape(-1) for case in group if case["depth_raw"] is not None and case["depth_raw"].dtype == np.uint16])
    assert np.isin(cases.DEPTH_SAMPLES, samples).all()
    _check_unpack(group, dev)


def test_unpack_frames_depth_only(dev):
    _check_unpack(cases.unpack_depth_only_cases(), dev)
