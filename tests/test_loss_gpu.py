"""GPU: kbn_photometric_loss_forward / ops.photometric_loss / KBNetModel.compute_loss against the golden vectors captured from
the reference (fp64 evaluation) and against tests/loss_oracle.py in fp64.

Gates
  terms   the four terms and the loss: 2e-5 relative to the fp64 value (TIGHT, the bound of test_eval_metrics_golden, which has
          the same fp32-per-pixel / fp64-across-pixels structure); NaN where the reference has NaN.
  images  image01 / image02 (values in [0, 1]): max abs error <= 3 x the fp32-to-fp64 distance of the reference itself (recorded
          in the fixture, or measured with the oracle in fp32) AND <= 1e-4.

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
