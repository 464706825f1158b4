"""GPU: kbn_photometric_loss_backward / ops.photometric_loss_backward / KBNetModel.compute_loss(...)[0].backward() against
torch.autograd through tests/loss_oracle.py in fp64 on the CPU (tests/test_loss_grad_oracle_cpu.py pins that oracle to
gradients captured from the reference).

Gates (tests/loss_grad_oracle.py check_gates), fixed from the fp32-against-fp64 distance of the oracle's own autograd:
  depth   per pixel |g - g64| <= 1e-3 |g64| + 1e-3 rms_frame(g64); the loss has kinks (floor of the sample position, sgn at 0,
          the clamp) that put a pixel on the other branch in one precision and not in the other, so at most pixels // 1000
          pixels of a case and column may miss, and those are finite
  pose    rows 0-2, per frame: max |g - g64| <= 5e-3 max |g64|; row 3 exactly 0
Every gate is taken per column of the N x 8 sums (grad_sums one-hot), so that the 0.04-weighted smoothness term cannot hide
behind SSIM, and once with a random positive grad_sums.

    python -m pytest tests/test_loss_backward_gpu.py -m gpu -s -q      (prints every figure before it asserts)
"""
import functools
import math
import os

import numpy as np
import pytest
import torch

import kbnet_amd as kb
from conftest import GOLDEN_DIR

import loss_cases
import loss_grad_oracle as lg
import loss_oracle as lo

pytestmark = pytest.mark.gpu

GOLDENS = ("everything_37x45", "two_plane_50x130")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need a visible MI355X (run with -m gpu on a GPU box)")
    kb._lib.load()   # a missing extension is an error on a GPU box, never a skip
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev):
    return kb.modules.KBNetModel.from_config(kb.kitti_config().narrow(), dev)


@functools.lru_cache(maxsize=None)
def _want(name):
    """The yardstick of one case, computed once: {column: (grad_depth, grad_pose01, grad_pose02)} in fp64 on the CPU."""
    return lg.autograd_columns([a.double() for a in loss_cases.case(name)], lo.loss_sums)


def _backward(dev, args, column):
    gs = lg.grad_sums_of(column, args[0].shape[0]).to(dev)
    return kb.ops.photometric_loss_backward(*args, gs)


# ---------------------------------------------------------------- 1. the raw wrapper, column by column
@pytest.mark.parametrize("name", list(loss_cases.CASES))
def test_raw_wrapper_against_fp64_autograd(dev, name):
    args = [a.to(dev) for a in loss_cases.case(name)]
    want = _want(name)
    for column in lg.COLUMNS:
        got = _backward(dev, args, column)
        assert got[0].dtype == got[1].dtype == got[2].dtype == torch.float32
        assert tuple(got[0].shape) == tuple(args[3].shape) and tuple(got[1].shape) == tuple(got[2].shape) == tuple(args[7].shape)
        lg.check_gates(f"{name} column {column}", got, want[column])


# ---------------------------------------------------------------- 2. the goldens through compute_loss(...)[0].backward()
@pytest.mark.parametrize("name", GOLDENS)
def test_compute_loss_backward_against_the_reference_gradients(dev, model, name):
    """The gradients the reference's own compute_loss gave in fp64 (tests/golden/gen_loss_grad_golden.py), reached through
    KBNetModel.compute_loss and autograd."""
    g = np.load(os.path.join(GOLDEN_DIR, f"grad_loss_{name}.npz"))
    args = [a.to(dev) for a in loss_cases.case(name)]
    for i in (3, 7, 8):
        args[i].requires_grad_(True)
    loss, info = model.compute_loss(*args)
    assert loss.requires_grad and not info["image01"].requires_grad and not info["image02"].requires_grad
    assert abs(float(loss.detach()) - float(g["loss"])) <= 2e-5 * abs(float(g["loss"]))     # the forward's own gate
    loss.backward()
    want = [torch.from_numpy(g[k]) for k in ("grad_output_depth", "grad_pose01", "grad_pose02")]
    lg.check_gates(f"{name} compute_loss", (args[3].grad, args[7].grad, args[8].grad), want)


def test_gradient_reaches_a_dof_leaf_through_pose_matrix(dev, model):
    """ops.pose_matrix is plain torch: the 6-vector the pose network emits gets its gradient by the chain rule.  The wiring is
    checked exactly (the dof gradient is torch's backward of ops.pose_matrix applied to the pose gradient this kernel gave); the
    translation entries ARE entries of the pose gradient (column 3), so they meet the pose gate against the oracle's fp64
    autograd through its own pose_matrix.  The rotation entries' distance is printed."""
    t = dict(zip(loss_cases.KEYS, kb.synthetic.make_triplet(2, 37, 45, "void", seed=71)))
    cpu = [t[k] for k in loss_cases.KEYS]
    a64 = [x.double() for x in cpu]
    a64[7].requires_grad_(True)
    a64[8].requires_grad_(True)
    m64 = [lo.pose_matrix(a64[7]), lo.pose_matrix(a64[8])]
    loss64 = lo.compute_loss(*a64[:7], *m64)["loss"]
    want = torch.autograd.grad(loss64, [a64[7], a64[8]] + m64)
    args = [x.to(dev) for x in cpu]
    args[7].requires_grad_(True)
    args[8].requires_grad_(True)
    mats = [kb.ops.pose_matrix(args[7]), kb.ops.pose_matrix(args[8])]
    for m in mats:
        m.retain_grad()
    loss, _ = model.compute_loss(*args[:7], *mats)
    loss.backward()
    for dof, m, w, wm, label in ((args[7], mats[0], want[0], want[2], "dof01"), (args[8], mats[1], want[1], want[3], "dof02")):
        got = dof.grad
        assert tuple(got.shape) == (2, 6) and bool(torch.isfinite(got).all()) and bool((got != 0).all()), (label, got)
        leaf = dof.detach().clone().requires_grad_(True)
        chain, = torch.autograd.grad(kb.ops.pose_matrix(leaf), leaf, grad_outputs=m.grad)
        assert torch.equal(got, chain), label
        scale = wm[:, :3].abs().amax(dim=(1, 2))
        trans = (got[:, 3:].double().cpu() - w[:, 3:]).abs().amax(dim=1) / scale
        rot = (got[:, :3].double().cpu() - w[:, :3]).abs().amax(dim=1) / w[:, :3].abs().amax(dim=1)
        print(f"{label}: translation {float(trans.max()):.3g} of the pose gradient's largest entry (gate {lg.POSE_REL}); "
              f"rotation {float(rot.max()):.3g} of its own largest entry")
        assert float(trans.max()) <= lg.POSE_REL, (label, trans)


# ---------------------------------------------------------------- 3. no side effects
def test_requires_grad_changes_no_bit_and_backward_repeats(dev):
    args = [a.to(dev) for a in loss_cases.case("everything_50x130")]
    plain = kb.ops.photometric_loss(*args, return_images=True)
    assert all(t.grad_fn is None and not t.requires_grad for t in plain)
    leaves = [a.clone() for a in args]
    for i in (3, 7, 8):
        leaves[i].requires_grad_(True)
    sums, w1, w2 = kb.ops.photometric_loss(*leaves, return_images=True)
    assert sums.grad_fn is not None and not w1.requires_grad and not w2.requires_grad
    assert all(torch.equal(a, b) for a, b in zip(plain, (sums, w1, w2)))
    with torch.no_grad():
        quiet = kb.ops.photometric_loss(*leaves, return_images=True)
    assert all(t.grad_fn is None and not t.requires_grad for t in quiet) and all(torch.equal(a, b) for a, b in zip(plain, quiet))

    gs = lg.grad_sums_of("random", 3).to(dev)
    first = torch.autograd.grad(sums, [leaves[3], leaves[7], leaves[8]], grad_outputs=gs, retain_graph=True)
    second = torch.autograd.grad(sums, [leaves[3], leaves[7], leaves[8]], grad_outputs=gs, retain_graph=True)
    assert torch.equal(first[0], second[0])
    for a, b in zip(first[1:], second[1:]):          # fp64 atomics reorder
        assert float((a.double() - b.double()).abs().max()) <= 1e-12 * float(a.double().abs().max())
    raw = kb.ops.photometric_loss_backward(*args, gs)
    assert torch.equal(raw[0], first[0])
    only_depth = torch.autograd.grad(sums, [leaves[3]], grad_outputs=gs)
    assert torch.equal(only_depth[0], first[0])


def _grad_t(dev, args, gs):
    """(grad_depth, the N x 2 x 12 fp64 buffer) of the raw wrapper: the pose gradients before their one rounding to fp32."""
    n, _, h, w = args[0].shape
    out = (torch.empty((n, 1, h, w), device=dev), torch.empty((n, 2, 12), device=dev, dtype=torch.float64))
    kb.ops.photometric_loss_backward(*args, gs, out=out)
    torch.cuda.synchronize()
    return out[0].cpu(), out[1].cpu()


def _same_frame(label, got, want):
    """Bit-identical depth gradient; pose sums equal to 1e-12 relative to the frame's largest (the atomics reorder)."""
    assert torch.equal(got[0], want[0]), label
    assert float((got[1] - want[1]).abs().max()) <= 1e-12 * float(want[1].abs().max()), label


# ---------------------------------------------------------------- 4. frames are independent
def test_frames_are_independent_and_permute(dev):
    cpu = loss_cases.build(loss_cases.FAMILIES, 4, 50, 130, "kitti", seed=81)
    args = [a.to(dev) for a in cpu]
    gs = (torch.rand(4, 8, dtype=torch.float64, generator=torch.Generator().manual_seed(5)) + 0.5).to(dev)
    gd, gt = _grad_t(dev, args, gs)
    assert bool(torch.isfinite(gd).all()) and bool(torch.isfinite(gt).all())
    for i in range(4):
        ad, at = _grad_t(dev, [a[i:i + 1].contiguous() for a in args], gs[i:i + 1].contiguous())
        _same_frame(f"frame {i} alone", (ad[0], at[0]), (gd[i], gt[i]))
    perm = torch.tensor([2, 0, 3, 1], device=dev)
    pd, pt = _grad_t(dev, [a[perm].contiguous() for a in args], gs[perm].contiguous())
    for j, i in enumerate(perm.tolist()):
        _same_frame(f"permuted frame {i}", (pd[j], pt[j]), (gd[i], gt[i]))


# ---------------------------------------------------------------- 5. poison stays in its frame
def _poison_image1(a):
    a[1][1, 1, 20, 70] = math.nan


def _poison_depth_inf_nan(a):
    a[3][1, 0, 7, 30] = math.inf          # inside tile (0, 0)
    a[3][1, 0, 15, 63] = math.nan         # the last pixel of tile (0, 0): in the halo of three other tiles


def _poison_depth_huge(a):
    a[3][1, 0, 24, 100] = 1e30


def _poison_pose01_nan(a):
    a[7][1, 1, 2] = math.nan


def _poison_pose01_huge(a):
    a[7][1, :3, 3] = 1e30


#          poison                  the columns of frame 1 that do not read it
POISONS = {
    "image1_nan":    (_poison_image1, (1, 3, 4, 5, 6, 7)),
    "depth_inf_nan": (_poison_depth_inf_nan, (5,)),
    "depth_1e30":    (_poison_depth_huge, (5,)),
    "pose01_nan":    (_poison_pose01_nan, (1, 3, 4, 5, 6, 7)),
    "pose01_1e30":   (_poison_pose01_huge, (1, 3, 4, 5, 6, 7)),
}


@pytest.mark.parametrize("poison", list(POISONS))
def test_poison_in_one_frame_stays_in_that_frame(dev, poison):
    """The inputs of tests/test_loss_gpu.py's poison table (and NaN in pose01) in frame 1 of 3: the launch succeeds, frames 0 and 2
    get the gradients they get without the poison, and in frame 1 the columns that do not read the poisoned tensor keep finite
    gradients inside the gates."""
    edit, untouched = POISONS[poison]
    cpu = loss_cases.build(("general_camera",), 3, 50, 130, "kitti", seed=53)
    dirty_cpu = [a.clone() for a in cpu]
    edit(dirty_cpu)
    clean, dirty = [a.to(dev) for a in cpu], [a.to(dev) for a in dirty_cpu]
    gs = lg.grad_sums_of("random", 3).to(dev)
    cd, ct = _grad_t(dev, clean, gs)          # synchronises: raises if the kernel faulted
    dd, dt = _grad_t(dev, dirty, gs)
    assert bool(torch.isfinite(cd).all()) and bool(torch.isfinite(ct).all())
    for i in (0, 2):
        _same_frame(f"{poison} frame {i}", (dd[i], dt[i]), (cd[i], ct[i]))
    want = lg.autograd_columns([a.double() for a in cpu], lo.loss_sums, columns=untouched)
    for column in untouched:
        got = kb.ops.photometric_loss_backward(*dirty, lg.grad_sums_of(column, 3).to(dev))
        frame1 = [g[1:2] for g in got]
        assert all(bool(torch.isfinite(g).all()) for g in frame1), (poison, column)
        if poison in ("image1_nan", "pose01_nan", "pose01_1e30"):       # the clean frame's gradient is the right answer there
            lg.check_gates(f"{poison} frame 1 column {column}", frame1, [w[1:2] for w in want[column]])


# ---------------------------------------------------------------- 6. guarded buffers
@pytest.mark.parametrize("name", ["general_camera_13x40", "everything_50x130"])
def test_outputs_stay_inside_guarded_buffers(dev, name):
    args = [a.to(dev) for a in loss_cases.case(name)]
    n, _, h, w = args[0].shape
    guard, sentinel = 4096, -12345.0
    big_d = torch.full((guard + n * h * w + guard,), sentinel, device=dev)
    big_t = torch.full((guard + n * 24 + guard,), sentinel, device=dev, dtype=torch.float64)
    gd = big_d[guard:guard + n * h * w].view(n, 1, h, w)
    gt = big_t[guard:guard + n * 24].view(n, 2, 12)
    gd.fill_(math.nan)
    gt.fill_(math.nan)
    got = kb.ops.photometric_loss_backward(*args, lg.grad_sums_of("random", n).to(dev), out=(gd, gt))
    torch.cuda.synchronize()
    assert got[0].data_ptr() == gd.data_ptr()
    for big in (big_d, big_t):
        assert bool((big[:guard] == sentinel).all()) and bool((big[-guard:] == sentinel).all())
    assert not bool(torch.isnan(gd).any()) and not bool(torch.isnan(gt).any())       # every element was overwritten
    lg.check_gates(f"{name} guarded", got, _want(name)["random"])


# ---------------------------------------------------------------- 7. one full-size run
@pytest.mark.slow
def test_full_size_against_fp32_autograd_on_the_device(dev):
    """1 x 352 x 1216 against the oracle's fp32 autograd on the device (fp64 on the CPU is not affordable in a test here):
    relative L2 of the depth gradient <= 1e-3, the gate the feature's issue fixed from the oracle's fp32-against-fp64 distance on
    the small cases (<= 8.8e-5).

    THIS GATE IS NOT MET, and not by the oracle either.  Measured on an MI355X: 1.16e-3 (pose gradients 4.8e-4 and 4.4e-5 of their
    largest entry, gate 5e-3).  On the same input the oracle's own fp32 autograd is 1.52e-3 from its fp64 autograd (CPU), 47 of
    428 032 pixels outside the per-pixel gate (cap 428), and 10 pixels hold 90 % of the squared error, 100 pixels 99.95 %: every
    one of them has a sample position within 6e-5 pixels of an integer, which fp32 (rounding W 2^-23 = 1.4e-4 at W = 1216, ten
    times that of the small cases) puts in the next cell, where the bilinear gradient reads other taps.  The relative L2 weighs
    those few pixels in full, where the per-pixel gate with its cap sets them aside; smoother images (make_triplet radius 8 / 16:
    1.09e-3 / 8.2e-4 for the oracle's fp32) do not change the picture.  The gate stays as the issue states it."""
    *frames, v01, v02 = kb.synthetic.make_triplet(1, 352, 1216, "kitti", seed=91)
    args = [a.to(dev) for a in frames + [kb.ops.pose_matrix(v01), kb.ops.pose_matrix(v02)]]
    gs = lg.grad_sums_of("random", 1).to(dev)
    got = kb.ops.photometric_loss_backward(*args, gs)
    want = lg.autograd(args, gs.float(), lo.loss_sums)
    rel = float((got[0].double() - want[0].double()).norm() / want[0].double().norm())
    pose = [float((g.double() - w.double()).abs().max() / w.double().abs().max()) for g, w in zip(got[1:], want[1:])]
    print(f"full size: relative L2 of the depth gradient {rel:.3g}; pose gradients {pose[0]:.3g} {pose[1]:.3g} of their largest entry")
    assert rel <= 1e-3 and max(pose) <= lg.POSE_REL
