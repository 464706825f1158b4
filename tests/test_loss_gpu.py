"""GPU: kbn_photometric_loss_forward / ops.photometric_loss / KBNetModel.compute_loss against the golden vectors captured from
the reference (fp64 evaluation) and against tests/loss_oracle.py in fp64.

Gates
  terms   the four terms and the loss: 2e-5 relative to the fp64 value (TIGHT, the bound of test_eval_metrics_golden, which has
          the same fp32-per-pixel / fp64-across-pixels structure); NaN where the reference has NaN.
  images  image01 / image02 (values in [0, 1]): max abs error <= 3 x the fp32-to-fp64 distance of the reference itself (recorded
          in the fixture, or measured with the oracle in fp32) AND <= 1e-4.
  sums    the N x 8 sums of ops.photometric_loss one by one (pair 01 and pair 02 apart): 2e-5 relative to loss_oracle.loss_sums in
          fp64; a sum that is exactly 0 in fp64 is compared absolutely against 0.

The inputs of tests/loss_cases.py (per-frame general cameras, depth on both sides of the camera, weighted validity, textured
images) are the ones tests/test_loss_power_cpu.py proves able to tell a wrong kernel from a right one at these gates.

    python -m pytest tests -m gpu -q
"""
import glob
import math
import os

import numpy as np
import pytest
import torch

import kbnet_amd as kb
from conftest import GOLDEN_DIR, load_golden

import loss_cases
import loss_oracle as lo

pytestmark = pytest.mark.gpu

TOL = 1e-4
TIGHT = 2e-5
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "loss_*.npz")))
INPUTS = ("image0", "image1", "image2", "output_depth", "sparse_depth", "validity_map", "intrinsics", "pose01", "pose02")
SCALARS = ("loss_color", "loss_structure", "loss_sparse_depth", "loss_smoothness", "loss")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need a visible MI355X (run with -m gpu on a GPU box)")
    kb._lib.load()   # a missing extension is an error on a GPU box, never a skip
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev):
    return kb.modules.KBNetModel.from_config(kb.kitti_config().narrow(), dev)


def _rel(a, b):
    a, b = float(a), float(b)
    if math.isnan(b):
        return 0.0 if math.isnan(a) else math.inf
    return abs(a - b) / abs(b)


def _triplet(n, h, w, kind, seed, outside=False):
    """make_triplet with the pose vectors turned into matrices; `outside`: a rotation that throws most samples off the image."""
    *frames, v01, v02 = kb.synthetic.make_triplet(n, h, w, kind, seed=seed)
    if outside:
        v01[:, :3] = torch.tensor([0.03, 0.65, 0.02])
        v02[:, :3] = torch.tensor([-0.6, -0.05, 0.03])
    return frames + [kb.ops.pose_matrix(v01), kb.ops.pose_matrix(v02)]


def _check(label, info, want64, image_dist):
    """The two gates; prints every figure before it asserts."""
    figures = {k: _rel(info[k], want64[k]) for k in SCALARS}
    images = {k: float((info[k].double().cpu() - want64[k]).abs().max()) for k in ("image01", "image02")}
    print(label, " ".join(f"{k} {v:.2e}" for k, v in figures.items()),
          " ".join(f"{k} {v:.2e} (fp32 reference {image_dist[k]:.2e})" for k, v in images.items()))
    for k, v in figures.items():
        assert v <= TIGHT, (label, k, v)
    for k, v in images.items():
        assert v <= 3 * image_dist[k] and v <= TOL, (label, k, v, image_dist[k])


def _check_sums(label, got, want64):
    """ops.photometric_loss against the fp64 sums, one by one; prints the worst figure before it asserts."""
    got = got.double().cpu()
    assert tuple(got.shape) == tuple(want64.shape) and want64.dtype == torch.float64
    figures = {}
    for i in range(got.shape[0]):
        for j in range(8):
            g, w = float(got[i, j]), float(want64[i, j])
            if w == 0.0:
                figures[(i, j)] = abs(g)           # nothing to be relative to: the sum itself, against the same 2e-5
            else:
                figures[(i, j)] = _rel(g, w)
    worst = max(figures, key=figures.get)
    print(label, f"sums: worst {figures[worst]:.2e} at frame {worst[0]} sum {worst[1]}",
          "worst per sum " + " ".join(f"{max(v for (i, j), v in figures.items() if j == k):.2e}" for k in range(8)))
    for key, v in figures.items():
        assert v <= TIGHT, (label, key, v)


def _against_oracle(label, model, dev, args):
    want64 = lo.compute_loss(*[a.double() for a in args])
    own32 = lo.compute_loss(*args)
    dist = {k: float((own32[k].double() - want64[k]).abs().max()) for k in ("image01", "image02")}
    loss, info = model.compute_loss(*[a.to(dev) for a in args])
    assert loss is info["loss"] and loss.dtype == torch.float32 and loss.dim() == 0 and loss.device.type == "cuda"
    _check(label, info, want64, dist)
    assert all(_rel(a, b) <= TIGHT for a, b in zip(info["per_frame"].flatten().cpu(), want64["per_frame"].flatten()))
    return info


@pytest.mark.parametrize("name", CASES)
def test_loss_golden(dev, model, name):
    g = load_golden(name)
    loss, info = model.compute_loss(*[g[k].to(dev) for k in INPUTS])
    assert set(info) == {"loss_color", "loss_structure", "loss_sparse_depth", "loss_smoothness", "loss", "image01", "image02", "per_frame"}
    assert info["per_frame"].dtype == torch.float64 and tuple(info["per_frame"].shape) == (g["image0"].shape[0], 4)
    _check(name, info, g["ref64"], {k: float(g["dist"][k]) for k in ("image01", "image02")})
    if name == "loss_novalid":
        assert math.isnan(float(loss)) and math.isnan(float(info["per_frame"][1, 2])) and not math.isnan(float(info["per_frame"][0, 2]))


@pytest.mark.parametrize("name", CASES)
def test_pose_matrix_golden(dev, name):
    g = load_golden(name)
    for p in ("pose01", "pose02"):
        got = kb.ops.pose_matrix(g[p + "_vector"].to(dev))
        assert got.is_cuda and got.dtype == torch.float32
        assert float((got.double().cpu() - g[p + "_fp64"]).abs().max()) <= TIGHT * float(g[p + "_fp64"].abs().max())


@pytest.mark.parametrize("kind,shape", [("kitti", (352, 1216)), ("void", (480, 640))])
def test_loss_full_size_vs_oracle(dev, model, kind, shape):
    _against_oracle(f"{kind} 2x{shape[0]}x{shape[1]}", model, dev, _triplet(2, *shape, kind, seed=3))


def test_batch_32_frames_equal_themselves_alone(dev):
    """Frame i of a 32-frame launch gives the sums it gives alone (fp64 atomics arrive in any order: 1e-12, not bits)."""
    base = _triplet(4, 352, 1216, "kitti", seed=6)
    args = [a.repeat(8, *([1] * (a.dim() - 1))) for a in base]
    v = torch.from_numpy(np.random.Generator(np.random.Philox(9)).random((2, 32, 6))).float()
    v = (v - 0.5) * torch.tensor([0.04, 0.04, 0.04, 1.0, 1.0, 1.0])          # a pose of its own for every frame
    args[7], args[8] = kb.ops.pose_matrix(v[0]), kb.ops.pose_matrix(v[1])
    args = [a.to(dev) for a in args]
    sums = kb.ops.photometric_loss(*args)
    assert tuple(sums.shape) == (32, 8) and sums.dtype == torch.float64
    worst = 0.0
    for i in range(32):
        alone = kb.ops.photometric_loss(*[a[i:i + 1] for a in args])
        worst = max(worst, float(((sums[i] - alone[0]).abs() / alone[0].abs()).max()))
    print(f"batch 32 vs alone: worst relative difference of a sum {worst:.2e}")
    assert worst <= 1e-12
    assert float((sums[:4] - sums[4:8]).abs().max()) > 0       # other poses, other sums


def test_sums_are_rewritten_and_independent_of_the_image_outputs(dev):
    args = [a.to(dev) for a in _triplet(2, 70, 100, "void", seed=8)]
    lib = kb._lib.load()
    sums = torch.full((2, 8), 1e30, device=dev, dtype=torch.float64)       # stale contents must not survive
    ptrs = [a.contiguous().data_ptr() for a in args]
    call = lambda: kb._lib.check(lib.kbn_photometric_loss_forward(*ptrs, sums.data_ptr(), None, None, 2, 70, 100,
                                                                  torch.cuda.current_stream().cuda_stream), "loss")
    call()
    first = sums.clone()
    call()
    assert float(((sums - first).abs() / first.abs()).max()) <= 1e-12
    plain = kb.ops.photometric_loss(*args)
    with_images, w1, w2 = kb.ops.photometric_loss(*args, return_images=True)
    assert float(((plain - first).abs() / first.abs()).max()) <= 1e-12
    assert float(((with_images - plain).abs() / plain.abs()).max()) <= 1e-12
    assert w1.shape == args[0].shape and w2.shape == args[0].shape


def test_loss_accepts_strided_views_and_another_stream(dev):
    args = _triplet(2, 33, 47, "kitti", seed=10)
    want = kb.ops.photometric_loss(*[a.to(dev) for a in args])
    padded = [torch.nn.functional.pad(a, (0, 3)).to(dev)[..., :a.shape[-1]] for a in args]      # non-contiguous views
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = kb.ops.photometric_loss(*padded)
    s.synchronize()
    assert float(((got - want).abs() / want.abs()).max()) <= 1e-12


def test_forward_then_compute_loss_end_to_end(dev):
    """model.forward on a narrow config, then compute_loss on ITS depth, against the oracle fed the same depth."""
    cfg = kb.kitti_config().narrow()
    m = kb.modules.KBNetModel.from_config(cfg, dev)
    m.load_state_dicts(*kb.synthetic.make_state_dicts(cfg, seed=0, gain=kb.synthetic.PARITY_GAIN["kitti"]))
    i0, i1, i2, _, sparse, validity, k, p01, p02 = _triplet(2, 64, 96, "kitti", seed=12)
    depth = m.forward(i0.to(dev), sparse.to(dev), validity.to(dev), k.to(dev))
    torch.cuda.synchronize()
    assert tuple(depth.shape) == (2, 1, 64, 96) and bool(torch.isfinite(depth).all())
    # the network's depths (1.5-100 m) need not suit the synthetic translation; keep every point in front of the camera
    for p in (p01, p02):
        p[:, :3, 3] *= min(1.0, 0.5 * float(depth.min()) / float(p[:, :3, 3].abs().max()))
    _against_oracle("end to end 2x64x96", m, dev, [i0, i1, i2, depth.cpu(), sparse, validity, k, p01, p02])


@pytest.mark.slow
@pytest.mark.parametrize("shape", [(3, 3), (3, 64), (17, 3), (37, 45), (64, 96), (353, 1217)])
@pytest.mark.parametrize("seed", [21, 22, 23])
@pytest.mark.parametrize("outside", [False, True])
def test_loss_size_sweep(dev, model, shape, seed, outside):
    args = _triplet(2, *shape, "kitti" if seed % 2 else "void", seed=seed, outside=outside)
    _against_oracle(f"{shape} seed {seed} outside {outside}", model, dev, args)


# ---------------------------------------------------------------- the inputs make_triplet does not produce (tests/loss_cases.py)
@pytest.mark.parametrize("name", list(loss_cases.CASES))
def test_loss_cases_vs_oracle(dev, model, name):
    args = loss_cases.case(name)
    _against_oracle(name, model, dev, args)
    _check_sums(name, kb.ops.photometric_loss(*[a.to(dev) for a in args]), lo.loss_sums(*[a.double() for a in args]))


def test_sums_of_a_frame_without_a_valid_point_are_zero(dev):
    """The fixture whose frame 1 has no valid point: its sums 4 and 5 are exactly 0 in fp64 and take _check_sums' absolute branch."""
    g = load_golden("loss_novalid")
    want = lo.loss_sums(*[g[k].double() for k in INPUTS])
    assert float(want[1, 4]) == 0.0 and float(want[1, 5]) == 0.0
    _check_sums("loss_novalid", kb.ops.photometric_loss(*[g[k].to(dev) for k in INPUTS]), want)


def test_frame_order_permutes_the_rows(dev):
    """A permutation of the frames of `everything` (every frame its own camera, poses, depth pattern and validity) permutes the
    rows of the sums (fp64 atomics arrive in any order: 1e-12) and the warped images, those bit for bit."""
    args = [a.to(dev) for a in loss_cases.build(loss_cases.FAMILIES, 5, 50, 130, "kitti", seed=51)]
    perm = torch.tensor([3, 0, 4, 1, 2], device=dev)
    sums, w1, w2 = kb.ops.photometric_loss(*args, return_images=True)
    psums, p1, p2 = kb.ops.photometric_loss(*[a[perm].contiguous() for a in args], return_images=True)
    worst = float(((psums - sums[perm]).abs() / sums[perm].abs()).max())
    print(f"frame order: worst relative difference of a sum {worst:.2e}")
    assert worst <= 1e-12
    assert torch.equal(p1, w1[perm]) and torch.equal(p2, w2[perm])
    assert float((sums[0] - sums[1]).abs().min()) > 0             # the rows differ: a permutation that is ignored would show


def test_batch_32_frames_32_cameras_vs_oracle(dev):
    """32 frames, 32 cameras, 64 poses: frames spread over the batch against the fp64 oracle of that frame alone (sums at TIGHT,
    images as _check gates them), and every frame against itself alone (1e-12)."""
    cpu = loss_cases.build(("general_camera", "weighted_validity"), 32, 100, 200, "kitti", seed=52)
    assert len({tuple(k.flatten().tolist()) for k in cpu[6]}) == 32
    args = [a.to(dev) for a in cpu]
    sums, w1, w2 = kb.ops.photometric_loss(*args, return_images=True)
    assert tuple(sums.shape) == (32, 8) and sums.dtype == torch.float64
    for i in (0, 9, 22, 31):
        one = [a[i:i + 1] for a in cpu]
        want64, own32 = lo.compute_loss(*[a.double() for a in one]), lo.compute_loss(*one)
        _check_sums(f"batch 32, frame {i}", sums[i:i + 1], lo.loss_sums(*[a.double() for a in one]))
        for k, got in (("image01", w1), ("image02", w2)):
            d, ref = float((got[i:i + 1].double().cpu() - want64[k]).abs().max()), float((own32[k].double() - want64[k]).abs().max())
            print(f"batch 32, frame {i} {k} {d:.2e} (fp32 reference {ref:.2e})")
            assert d <= 3 * ref and d <= TOL, (i, k, d, ref)
    worst = 0.0
    for i in range(32):
        alone = kb.ops.photometric_loss(*[a[i:i + 1] for a in args])
        worst = max(worst, float(((sums[i] - alone[0]).abs() / alone[0].abs()).max()))
    print(f"batch 32 cameras vs alone: worst relative difference of a sum {worst:.2e}")
    assert worst <= 1e-12


# ---------------------------------------------------------------- non-finite and huge values stay where they are
def _poison_image1(a):
    a[1][1, 1, 20, 70] = math.nan


def _poison_depth_inf_nan(a):
    a[3][1, 0, 7, 30] = math.inf          # inside tile (0, 0)
    a[3][1, 0, 15, 63] = math.nan         # the last pixel of tile (0, 0): in the halo of three other tiles


def _poison_depth_huge(a):
    a[3][1, 0, 24, 100] = 1e30


def _poison_sparse(a):
    y, x = [int(v[0]) for v in torch.nonzero(a[5][1, 0] == 1, as_tuple=True)]
    a[4][1, 0, y, x] = math.nan


def _poison_pose01(a):
    a[7][1, :3, 3] = 1e30


#          poison                  argument  sums of frame 1 it may change   warped images of frame 1 it may change
POISONS = {
    "image1_nan":    (_poison_image1, (0, 2), ("image01",)),
    "depth_inf_nan": (_poison_depth_inf_nan, (0, 1, 2, 3, 4, 6, 7), ("image01", "image02")),
    "depth_1e30":    (_poison_depth_huge, (0, 1, 2, 3, 4, 6, 7), ("image01", "image02")),
    "sparse_nan":    (_poison_sparse, (4,), ()),
    "pose01_1e30":   (_poison_pose01, (0, 2), ("image01",)),
}


@pytest.mark.parametrize("poison", list(POISONS))
def test_poison_in_one_frame_stays_in_that_frame_and_in_its_sums(dev, poison):
    """NaN, Inf and 1e30 in frame 1 of 3: the launch succeeds, frames 0 and 2 do not notice, and in frame 1 only the sums (and warped
    images) that read the poisoned tensor change.  Sample positions that come out NaN, infinite or huge are clamped into the image
    (csrc/loss.hip, `Addressing`); every read stays inside the tensors.  Where the poison does not reach the sample positions
    (image1, sparse_depth) the oracle is defined too, and a sum is NaN exactly where the fp64 oracle's is."""
    edit, may_change, images_may_change = POISONS[poison]
    cpu = loss_cases.build(("general_camera",), 3, 50, 130, "kitti", seed=53)
    clean = [a.to(dev) for a in cpu]
    dirty_cpu = [a.clone() for a in cpu]
    edit(dirty_cpu)
    dirty = [a.to(dev) for a in dirty_cpu]
    assert sum(not torch.equal(a, b) for a, b in zip(cpu, dirty_cpu)) == 1
    assert all(torch.equal(a[[0, 2]], b[[0, 2]]) for a, b in zip(cpu, dirty_cpu))

    lib = kb._lib.load()
    out = {}
    for label, args in (("clean", clean), ("dirty", dirty)):
        sums = torch.full((3, 8), 1e30, device=dev, dtype=torch.float64)
        w1, w2 = torch.empty_like(args[0]), torch.empty_like(args[0])
        rc = lib.kbn_photometric_loss_forward(*[a.data_ptr() for a in args], sums.data_ptr(), w1.data_ptr(), w2.data_ptr(), 3, 50, 130,
                                              torch.cuda.current_stream().cuda_stream)
        assert rc == kb._lib.KBN_OK, (label, rc)
        torch.cuda.synchronize()          # raises if the kernel faulted
        out[label] = (sums.cpu(), {"image01": w1.cpu(), "image02": w2.cpu()})
    (csums, cimg), (dsums, dimg) = out["clean"], out["dirty"]
    assert bool(torch.isfinite(csums).all())

    for i in (0, 2):
        assert float(((dsums[i] - csums[i]).abs() / csums[i].abs()).max()) <= 1e-12, (poison, i)
        assert all(torch.equal(dimg[k][i], cimg[k][i]) for k in dimg), (poison, i)
    for j in range(8):
        if j not in may_change:
            assert abs(float(dsums[1, j]) - float(csums[1, j])) <= 1e-12 * abs(float(csums[1, j])), (poison, j, dsums[1], csums[1])
    for k in dimg:
        if k not in images_may_change:
            assert torch.equal(dimg[k][1], cimg[k][1]), (poison, k)
    changed = [j for j in range(8) if not float(dsums[1, j]) == float(csums[1, j])]
    print(f"{poison}: sums of frame 1 that changed {changed}; clean {csums[1].tolist()} poisoned {dsums[1].tolist()}")
    assert changed, poison                                                       # the poison was read

    if poison in ("image1_nan", "sparse_nan"):
        want = lo.loss_sums(*[a.double() for a in dirty_cpu])
        for j in range(8):
            g, w = float(dsums[1, j]), float(want[1, j])
            assert math.isnan(g) == math.isnan(w), (poison, j, g, w)
            assert _rel(g, w) <= TIGHT, (poison, j, g, w)


# ---------------------------------------------------------------- the nearest stretch of the SSIM scores, length by length
STRETCH_LENGTHS = (4, 5, 6, 7, 15, 16, 17, 18, 31, 33, 63, 64, 65, 66, 127, 128, 129, 130, 257)


@pytest.mark.slow
@pytest.mark.parametrize("length", STRETCH_LENGTHS)
@pytest.mark.parametrize("thin", ["rows", "columns"])
def test_ssim_stretch_lengths(dev, model, length, thin):
    """Thin frames (L, 3) and (3, L): one SSIM score across, L - 2 along, each weighed by the number of pixels the nearest stretch
    copies it to (ssim_axis_weight); tests/test_loss_oracle_cpu.py checks that count on the host for every length to 2048."""
    shape = (length, 3) if thin == "rows" else (3, length)
    args = _triplet(2, *shape, "void" if length % 2 else "kitti", seed=60 + length)
    _against_oracle(f"stretch {shape}", model, dev, args)
    _check_sums(f"stretch {shape}", kb.ops.photometric_loss(*[a.to(dev) for a in args]), lo.loss_sums(*[a.double() for a in args]))
