"""CPU: the yardstick of the objective's gradient, and the host side of the backward's public surface.

  * tests/loss_oracle.py under torch.autograd in fp64 IS the reference's gradient: held to 1e-9 (relative to the frame's largest
    entry) against gradients the reference's own functions gave (tests/golden/gen_loss_grad_golden.py)
  * tests/loss_grad_oracle.py, the closed-form restatement the kernel is written against, equals that autograd to 1e-9 on every
    case of loss_cases.CASES, column by column of the N x 8 sums
  * ops.photometric_loss_backward and kbn_photometric_loss_backward reject what the forward rejects, a data argument that
    requires grad is an error that names it, and the header, the binding and the ABI number agree
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import kbnet_amd as kb
from conftest import GOLDEN_DIR

import loss_cases
import loss_grad_oracle as lg
import loss_oracle as lo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDENS = ("everything_37x45", "two_plane_50x130")
EXACT = 1e-9


@functools.lru_cache(maxsize=None)
def _case64(name):
    args = [a.double() for a in loss_cases.case(name)]
    return args, lg.autograd_columns(args, lo.loss_sums)


def _frame_rel(got, want):
    """max |got - want| of every frame over the frame's largest |want|; exact zeros against zeros give 0."""
    dims = tuple(range(1, want.dim()))
    err, scale = (got - want).abs().amax(dim=dims), want.abs().amax(dim=dims)
    return float(torch.where(err == 0, torch.zeros_like(err), err / scale).max())


# ---------------------------------------------------------------- the yardstick against the reference
@pytest.mark.parametrize("name", GOLDENS)
def test_oracle_autograd_is_the_references_gradient(name):
    g = np.load(os.path.join(GOLDEN_DIR, f"grad_loss_{name}.npz"))
    assert os.path.getsize(os.path.join(GOLDEN_DIR, f"grad_loss_{name}.npz")) < 1 << 20
    args = [a.double() for a in loss_cases.case(name)]
    for i in (3, 7, 8):
        args[i].requires_grad_(True)
    out = lo.compute_loss(*args)
    for k in ("loss_color", "loss_structure", "loss_sparse_depth", "loss_smoothness", "loss"):
        assert abs(float(out[k].detach()) - float(g[k])) <= EXACT * abs(float(g[k])), (name, k)
    grads = torch.autograd.grad(out["loss"], [args[3], args[7], args[8]])
    for got, key in zip(grads, ("grad_output_depth", "grad_pose01", "grad_pose02")):
        want = torch.from_numpy(g[key])
        rel = _frame_rel(got, want)
        print(f"{name} {key}: {rel:.2e}")
        assert tuple(got.shape) == tuple(want.shape) and rel <= EXACT, (name, key, rel)
    assert bool((torch.from_numpy(g["grad_pose01"])[:, 3] == 0).all()) and bool((torch.from_numpy(g["grad_pose02"])[:, 3] == 0).all())


# ---------------------------------------------------------------- the restatement against the yardstick
@pytest.mark.parametrize("name", list(loss_cases.CASES))
def test_closed_form_backward_is_the_oracles_autograd(name):
    args, want = _case64(name)
    worst = 0.0
    for column in lg.COLUMNS:
        got = lg.backward(args, lg.grad_sums_of(column, args[0].shape[0]))
        for g, w, label in zip(got, want[column], ("depth", "pose01", "pose02")):
            rel = _frame_rel(g, w)
            worst = max(worst, rel)
            assert rel <= EXACT, (name, column, label, rel)
        assert bool((got[1][:, 3] == 0).all()) and bool((got[2][:, 3] == 0).all())
        if column == 5:          # sum v depends on nothing differentiable
            assert all(bool((g == 0).all()) for g in got) and all(bool((w == 0).all()) for w in want[column])
    print(f"{name}: closed form against autograd, worst {worst:.2e}")


def test_stretch_weights_count_every_output_pixel():
    for size in (3, 4, 5, 13, 37, 45, 50, 70, 100, 130):
        wgt = lg.stretch_weights(size)
        assert wgt.numel() == size - 2 and float(wgt.sum()) == size and float(wgt.min()) >= 1


# ---------------------------------------------------------------- host-side checks of the public surface (no GPU needed)
def _cpu_args(n=1, h=8, w=12):
    i0, i1, i2, depth, sparse, validity, k, v01, v02 = kb.synthetic.make_triplet(n, h, w, "void", seed=2)
    return [i0, i1, i2, depth, sparse, validity, k, kb.ops.pose_matrix(v01), kb.ops.pose_matrix(v02)]


def test_backward_wrapper_rejects_what_the_forward_rejects():
    a = _cpu_args()
    gs = torch.ones(1, 8, dtype=torch.float64)
    with pytest.raises(kb._lib.KbnError, match="no CPU fallback"):
        kb.ops.photometric_loss_backward(*a, gs)
    for i, bad in ((1, a[1][:, :, :-1]), (3, a[3][:, :, :, :-1]), (5, torch.cat([a[5], a[5]])), (6, a[6][:, :2]), (7, a[7][:, :3])):
        b = list(a)
        b[i] = bad
        with pytest.raises(kb._lib.KbnError, match="must be"):
            kb.ops.photometric_loss_backward(*b, gs)
    with pytest.raises(kb._lib.KbnError, match="3 x 3"):
        kb.ops.photometric_loss_backward(*[t[:, :, :2] if t.dim() == 4 else t for t in a], gs)
    with pytest.raises(kb._lib.KbnError, match="must be a tensor"):
        kb.ops.photometric_loss_backward(*a[:8], None, gs)


@pytest.mark.parametrize("index, name", [(0, "image0"), (1, "image1"), (2, "image2"), (4, "sparse_depth"), (5, "validity_map"), (6, "intrinsics")])
def test_data_that_requires_grad_is_an_error_that_names_it(index, name):
    m = kb.modules.KBNetModel.from_config(kb.kitti_config().narrow(), device=torch.device("cpu"))
    a = _cpu_args()
    a[index] = a[index].clone().requires_grad_(True)
    a[3] = a[3].clone().requires_grad_(True)
    for call in (kb.ops.photometric_loss, m.compute_loss):
        with pytest.raises(kb._lib.KbnError, match=rf"{name} requires grad"):
            call(*a)
    with torch.no_grad():          # no graph is asked for: the forward's usual answer to CPU tensors
        with pytest.raises(kb._lib.KbnError, match="no CPU fallback"):
            kb.ops.photometric_loss(*a)


def test_the_backward_entry_point_checks_its_arguments():
    """Null pointers and sizes below 3 x 3: KBN_ERR_INVALID_ARGUMENT; more tiles than a grid holds: KBN_ERR_UNSUPPORTED; both
    before anything is launched."""
    lib = kb._lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    ok = [p] * 12
    call = lambda ptrs, n, h, w: lib.kbn_photometric_loss_backward(*ptrs, n, h, w, None)
    assert call(ok, 1, 2, 8) == call(ok, 1, 8, 2) == call(ok, 0, 8, 8) == call(ok, -1, 8, 8) == kb._lib.KBN_ERR_INVALID_ARGUMENT
    for i in range(12):
        assert call(ok[:i] + [None] + ok[i + 1:], 1, 8, 8) == kb._lib.KBN_ERR_INVALID_ARGUMENT, i
    assert call(ok, 2 ** 31 - 1, 2 ** 20, 2 ** 20) == kb._lib.KBN_ERR_UNSUPPORTED


def test_header_binding_and_abi_number_agree():
    header = open(os.path.join(ROOT, "include", "kbnet_hip.h")).read()
    assert int(re.search(r"#define KBN_ABI_VERSION (\d+)", header).group(1)) == kb._lib.ABI_VERSION == 11
    assert kb._lib.load().kbn_version() == 11
    decl = re.search(r"int kbn_photometric_loss_backward\((.*?)\);", header, flags=re.S).group(1)
    params = [p.strip() for p in decl.split(",")]
    res, args = kb._lib.SIGNATURES["kbn_photometric_loss_backward"]
    assert res is ctypes.c_int and len(params) == len(args) == 16
    for p, a in zip(params, args):
        assert (a is ctypes.c_void_p) == ("*" in p or "kbn_stream_t" in p) and (a is ctypes.c_int) == p.startswith("int "), (p, a)
    assert [p.split()[-1].lstrip("*") for p in params[9:12]] == ["grad_sums", "grad_depth", "grad_proj"]
    assert callable(kb.ops.photometric_loss_backward)
