"""ops.histogram_tensorflow (kbn_histogram_forward) against np.histogram(values.astype(float), bins=edges) on the host: counts, min
and max exactly, the two sums within the rounding of any float64 summation order, the same bits twice -- at sizes below, at and
above a wave and a quad, over several workgroups with a tail, over more chunks than the grid has workgroups, on misaligned and
strided views, with values planted at the bucket edges (tests/event_cases.py; test_event_writer_cpu.py proves the oracle's power)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kbnet_amd as kb  # noqa: E402
import event_cases as ec  # noqa: E402

pytestmark = pytest.mark.gpu

WORKGROUP = 4096                         # elements a workgroup takes at least (csrc/histogram.hip HIST_BLOCK_ELEMENTS)
COUNTS = [1, 63, 64, 65, 4097, 3 * WORKGROUP + 5]
CAPPED = 1027 * WORKGROUP + 5            # more chunks than the 1024 workgroups of the widest grid


def _run(t):
    """(counts, min, max, sum, sum_squares, raw bytes) of one call: ONE copy of the 6224-byte buffer."""
    counts, stats = kb.ops.histogram_tensorflow(t)
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (1548,) and stats.dtype == torch.float64 and tuple(stats.shape) == (4,)
    assert counts.is_cuda and stats.is_cuda and stats.data_ptr() == counts.data_ptr() + 4 * 1548 == counts._base.data_ptr() + 4 * 1548
    raw = counts._base.cpu().numpy()
    assert raw.nbytes == 6224
    mn, mx, total, squares = raw[1548:].view(np.float64)
    return raw[:1548].astype(np.int64), mn, mx, total, squares, raw.tobytes()


def _check(t, values, what):
    """All gates of one device view `t` whose elements are `values` (host float32, any shape)."""
    values = np.asarray(values, dtype=np.float32).reshape(-1)
    counts, mn, mx, total, squares, raw = _run(t)
    want = ec.histogram_oracle(values)
    lo, hi, num, want_total, want_squares, bound_total, bound_squares = ec.stats_oracle(values)
    print(f"{what}: n {values.size}, counted {counts.sum()}, occupied bins {np.count_nonzero(counts)}, min {mn}, max {mx}", end="")
    assert np.array_equal(counts, want), (what, np.flatnonzero(counts != want)[:8])
    assert np.array_equal(np.float64(mn), lo, equal_nan=True) and np.array_equal(np.float64(mx), hi, equal_nan=True), (what, mn, lo, mx, hi)
    assert float(t.numel()) == num
    if want_total is not None:
        print(f", sum error {abs(total - want_total):.3e} (bound {bound_total:.3e}), squares error {abs(squares - want_squares):.3e} "
              f"(bound {bound_squares:.3e})", end="")
        assert abs(total - want_total) <= bound_total and abs(squares - want_squares) <= bound_squares, what
    elif np.isnan(values).any():      # values.sum() and values.dot(values) of TensorBoard run over everything
        assert np.isnan(total) and np.isnan(squares), what
    print()
    assert _run(t)[5] == raw, what      # the same bits twice
    return counts


@pytest.mark.parametrize("finite", [False, True], ids=["planted", "finite"])
@pytest.mark.parametrize("n", COUNTS)
def test_contiguous(n, finite):
    values = ec.seeded_values(n, seed=n, finite=finite)
    t = torch.from_numpy(values).cuda()
    assert t.data_ptr() % 16 == 0
    counts = _check(t, values, f"contiguous {n}")
    if n >= 28 and not finite:
        assert counts.sum() < n and np.isnan(_run(t)[1]) and np.isnan(_run(t)[2])      # NaN propagates into min and max


@pytest.mark.parametrize("n", [1, 2, 3, 65, 4097, 3 * WORKGROUP + 5])
@pytest.mark.parametrize("offset", [1, 2, 3])
def test_off_the_16_byte_boundary(n, offset):
    values = ec.seeded_values(n + offset + 3, seed=100 + n + offset, finite=True)
    base = torch.from_numpy(values).cuda()
    t = base[offset:offset + n]
    assert t.is_contiguous() and t.data_ptr() % 16 == 4 * offset
    _check(t, values[offset:offset + n], f"offset {offset}, {n}")


def test_the_views_log_summary_passes():
    rng = np.random.default_rng(7)
    pose = rng.normal(size=(5, 4, 4)).astype(np.float32)
    pose[1, 0, 3] = 0.0
    t = torch.from_numpy(pose).cuda()
    _check(t[:, 0, 3], pose[:, 0, 3], "pose[:, 0, 3]")
    x = ec.seeded_values(3 * 2 * 7 * 9, seed=8, finite=True).reshape(3, 2, 7, 9)
    t = torch.from_numpy(x).cuda()
    view = t[:, 0:1]
    assert not view.is_contiguous()
    _check(view, x[:, 0:1], "x[:, 0:1]")
    _check(torch.unsqueeze(t[:, 0, :, :], dim=1), x[:, 0:1], "unsqueeze(x[:, 0])")
    # a sparse depth map: long runs of zeros (one LDS atomic a run), all in the bin [0, 1e-12)
    depth = (rng.uniform(1.0, 80.0, size=(2, 1, 24, 40)) * (rng.uniform(size=(2, 1, 24, 40)) < 0.05)).astype(np.float32)
    counts = _check(torch.from_numpy(depth).cuda(), depth, "sparse depth")
    assert counts[774] == np.count_nonzero(depth == 0)


def test_more_chunks_than_workgroups():
    values = ec.seeded_values(CAPPED, seed=9, plant=False)
    values[-5:] = [0.0, -0.0, 1e-13, -1e-13, 7.0]      # the tail
    _check(torch.from_numpy(values).cuda(), values, f"capped grid {CAPPED}")


def test_refusals():
    with pytest.raises(ValueError, match="The input has no element."):
        kb.ops.histogram_tensorflow(torch.empty(0, device="cuda"))
    with pytest.raises(kb._lib.KbnError):
        kb.ops.histogram_tensorflow(torch.ones(4))
    with pytest.raises(kb._lib.KbnError):
        kb.ops.histogram_tensorflow(torch.ones(4, device="cuda", dtype=torch.float64))
