"""CPU: do the inputs of tests/loss_cases.py have the power to tell a wrong backward kernel from a right one?

Every entry of COLUMNS (loss_grad_oracle.MISTAKES but the one that no input here can show, see below) is the closed-form backward (tests/loss_grad_oracle.py, fp64) with one deliberate
mistake of the kind one can make in csrc/loss_backward.hip.  For each, at least one case of loss_cases.CASES and one column of
the N x 8 sums must move a GATED quantity by at least 10 x its gate:

  depth   more pixels than the cap (pixels // 1000 of the case) are 10 gates or more away, the gate being
          1e-3 |g64| + 1e-3 rms_frame(g64) per pixel
  pose    a frame's max |g - g64| over rows 0-2 is at least 10 x 5e-3 max |g64|

These are the gates of tests/test_loss_backward_gpu.py.  The other half of the argument keeps a CORRECT fp32 evaluation (the
oracle's own fp32 autograd) within a third of every gate on every case and column, the pixel cap as stated, so the same inputs
cannot fail a right kernel.

    python -m pytest tests/test_loss_grad_power_cpu.py -s -q      (prints the table: mistake, best case and column, factor)
"""
import functools

import pytest
import torch

import loss_cases
import loss_grad_oracle as lg
import loss_oracle as lo

POWER = 10.0
# the columns a mistake can show in, so that the search does not run the closed form 72 times per mistake
COLUMNS = {
    "gradient kept where the position was clamped": (0, 1, 2, 3),
    "-(g_u u + g_v v) / d dropped": (0, 1, 2, 3),
    "frame 0's K for every frame": (0, 1, 2, 3),
    "K instead of K^T in the pose gradient": (0, 1, 2, 3),
    "SSIM coefficient C dropped": (2, 3),
    "stretch weights ignored": (2, 3),
    "halo of 1 instead of 2": (2, 3),
    "smoothness sign flipped for the left / upper neighbour": (6, 7),
    "validity weight squared": (4,),
    "validity weight dropped": (4,),
    "pair 1 accumulated into pose01": (1, 3),
}


@functools.lru_cache(maxsize=None)
def _case64(name):
    args = [a.double() for a in loss_cases.case(name)]
    return args, lg.autograd_columns(args, lo.loss_sums)


def factors(got, want):
    """-> (depth, pose): the depth factor is the largest f such that MORE pixels than the cap are at least f gates away (so a
    kernel with that error fails the depth gate scaled by f); the pose factor is the worst frame's ratio to its gate."""
    ratio = lg.depth_gate(got[0], want[0]).flatten()
    cap = ratio.numel() // 1000
    depth = float(ratio.sort(descending=True).values[cap])          # the (cap + 1)-th worst pixel
    pose = max(float(lg.pose_gate(got[1], want[1]).max()), float(lg.pose_gate(got[2], want[2]).max()))
    return depth, pose


def test_the_table_has_the_issues_mistakes():
    assert set(COLUMNS) == set(lg.MISTAKES) - set(lg.INVISIBLE) and len(COLUMNS) >= 10


def test_the_missing_1e_7_cannot_be_seen():
    """d = q2 + 1e-7: no case has a point within 0.1 of the camera plane (loss_cases.two_plane asserts it, for the reason given in
    tests/golden/gen_loss_golden.py), so leaving the 1e-7 out moves a gradient by about 1e-6 of itself, a thousandth of the gates.
    Recorded, not asserted as caught: the kernel takes d from the helper the forward uses (csrc/loss_common.h), which the
    forward's tests hold to 2e-5."""
    worst = 0.0
    for name in loss_cases.CASES:
        args, want = _case64(name)
        for column in (0, 1, 2, 3):
            got = lg.backward(args, lg.grad_sums_of(column, args[0].shape[0]), mistakes=lg.INVISIBLE)
            worst = max(worst, *factors(got, want[column]))
    print(f"\nd without the 1e-7: at most {worst:.3g} of a gate")
    assert worst < 1.0


@pytest.mark.parametrize("mistake", list(COLUMNS))
def test_every_mistake_is_caught_ten_times_over(mistake):
    best = (0.0, None, None, None)
    for name in loss_cases.CASES:
        args, want = _case64(name)
        for column in COLUMNS[mistake]:
            got = lg.backward(args, lg.grad_sums_of(column, args[0].shape[0]), mistakes=(mistake,))
            depth, pose = factors(got, want[column])
            best = max(best, (depth, name, column, "depth"), (pose, name, column, "pose"), key=lambda b: b[0])
    print(f"\n| {mistake} | {best[1]} | column {best[2]} | {best[3]} | {best[0]:.3g} |")
    assert best[0] >= POWER, (mistake, best)


@pytest.mark.parametrize("name", list(loss_cases.CASES))
def test_fp32_autograd_is_three_times_inside_the_gates(name):
    """The oracle's own fp32 autograd against its fp64 autograd, every column: at most pixels // 1000 pixels of the case outside a
    third of the depth gate (the kinks), those finite; every frame's pose gradients within a third of theirs."""
    _, want = _case64(name)
    got = lg.autograd_columns(loss_cases.case(name), lo.loss_sums)
    for column in lg.COLUMNS:
        lg.check_gates(f"{name} column {column} fp32 autograd", got[column], want[column], fraction=1.0 / 3.0)
