"""CPU: tests/loss_oracle.py (the restatement of the objective's forward value that the GPU tests compare the kernel with)
against the golden vectors captured from the reference (tests/golden/gen_loss_golden.py), and the host-side argument checks of
ops.photometric_loss / ops.pose_matrix / KBNetModel.compute_loss.

Each fixture stores the reference's fp32 outputs, the same functions evaluated in fp64 and the distance between the two.  The
oracle's fp64 run must reproduce the fp64 outputs (1e-12), and its fp32 run may be no farther from them than twice the
reference's own fp32 run is."""
import glob
import math
import os
import sys

import numpy as np
import pytest
import torch

import kbnet_amd as kb
from conftest import GOLDEN_DIR, load_golden

import loss_oracle as lo

CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "loss_*.npz")))
INPUTS = ("image0", "image1", "image2", "output_depth", "sparse_depth", "validity_map", "intrinsics", "pose01", "pose02")
SCALARS = ("loss_color", "loss_structure", "loss_sparse_depth", "loss_smoothness", "loss")
REFERENCE_SRC = "/root/reference/src"


def _rel(a, b):
    a, b = float(a), float(b)
    if math.isnan(b):
        return 0.0 if math.isnan(a) else math.inf
    return abs(a - b) / abs(b)


def test_the_fixtures_cover_the_cases():
    assert {"loss_even", "loss_odd", "loss_3x3", "loss_3x4", "loss_identity", "loss_outside", "loss_behind", "loss_novalid",
            "loss_general_camera", "loss_two_plane", "loss_weighted_validity", "loss_textured"} <= set(CASES)
    for name in CASES:
        assert os.path.getsize(os.path.join(GOLDEN_DIR, name + ".npz")) < 1 << 20


@pytest.mark.parametrize("name", CASES)
def test_oracle_fp64_reproduces_the_reference(name):
    g = load_golden(name)
    out = lo.compute_loss(*[g[k].double() for k in INPUTS])
    for k in SCALARS:
        assert _rel(out[k], g["ref64"][k]) <= 1e-12, k
    for k in ("image01", "image02"):
        assert float((out[k] - g["ref64"][k]).abs().max()) <= 1e-12, k
    want = torch.stack([g["ref64"][k] for k in SCALARS[:4]])
    got = out["per_frame"].mean(0)
    assert all(_rel(a, b) <= 1e-12 for a, b in zip(got, want))


@pytest.mark.parametrize("name", CASES)
def test_oracle_fp32_is_as_close_as_the_reference_fp32(name):
    g = load_golden(name)
    out = lo.compute_loss(*[g[k] for k in INPUTS])
    assert out["loss"].dtype == torch.float32
    for k in SCALARS:
        d = _rel(out[k], g["ref64"][k])
        print(f"{name} {k}: oracle fp32 {d:.2e}, reference fp32 {float(g['dist'][k]):.2e}, bit-equal {bool(out[k] == g['ref32'][k])}")
        assert d <= 2 * float(g["dist"][k]), k
    for k in ("image01", "image02"):
        d = float((out[k].double() - g["ref64"][k]).abs().max())
        print(f"{name} {k}: oracle fp32 {d:.2e}, reference fp32 {float(g['dist'][k]):.2e}, bit-equal {torch.equal(out[k], g['ref32'][k])}")
        assert d <= 2 * float(g["dist"][k]), k


def test_the_special_cases_are_what_they_claim():
    g = load_golden("loss_identity")
    assert torch.equal(g["image1"], g["image0"]) and torch.equal(g["pose01"][0], torch.eye(4))
    # not exactly image0 even in fp64: the 1e-7 added to z moves a point at 2.5 m by 4e-8 of its image coordinate
    assert float((g["ref64"]["image01"] - g["image0"].double()).abs().max()) < 1e-6
    g = load_golden("loss_novalid")
    assert float(g["validity_map"][1].sum()) == 0 and math.isnan(float(g["ref32"]["loss_sparse_depth"])) and math.isnan(float(g["ref32"]["loss"]))
    out = lo.compute_loss(*[g[k] for k in INPUTS])
    assert math.isnan(float(out["per_frame"][1, 2])) and not math.isnan(float(out["per_frame"][0, 2]))


@pytest.mark.parametrize("name", CASES)
def test_pose_matrix_matches_the_reference(name):
    g = load_golden(name)
    for p in ("pose01", "pose02"):
        v = g[p + "_vector"]
        assert torch.equal(lo.pose_matrix(v), g[p]), p
        assert float((lo.pose_matrix(v.double()) - g[p + "_fp64"]).abs().max()) <= 1e-15
        assert float((kb.ops.pose_matrix(v).double() - g[p + "_fp64"]).abs().max()) <= 2e-5 * float(g[p + "_fp64"].abs().max())
        assert float((kb.ops.pose_matrix(v.double()) - g[p + "_fp64"]).abs().max()) <= 1e-15


def _reference_outputs(net_utils, losses, inputs, dtype):
    """The reference's functions in the order of its compute_loss, in `dtype` (it builds its meshgrid in torch's default dtype)."""
    torch.set_default_dtype(dtype)
    try:
        i0, i1, i2, depth, sparse, validity, k, p01, p02 = [t.to(dtype) for t in inputs]
        ones = torch.ones_like(sparse)
        pts = net_utils.backproject_to_camera(depth, k, i0.shape)
        warped = [net_utils.grid_sample(im, net_utils.project_to_pixel(pts, p, k, i0.shape), i0.shape) for im, p in ((i1, p01), (i2, p02))]
        terms = [sum(losses.color_consistency_loss_func(x, i0, ones) for x in warped),
                 sum(losses.structural_consistency_loss_func(x, i0, ones) for x in warped),
                 losses.sparse_depth_consistency_loss_func(depth, sparse, validity), losses.smoothness_loss_func(depth, i0)]
        return terms, warped
    finally:
        torch.set_default_dtype(torch.float32)


@pytest.mark.skipif(not os.path.isdir(REFERENCE_SRC), reason="needs the reference checkout (build container only)")
@pytest.mark.parametrize("kind,shape", [("kitti", (352, 1216)), ("void", (480, 640))])
def test_oracle_against_the_imported_reference_full_size(kind, shape):
    sys.path.insert(0, REFERENCE_SRC)
    try:
        import losses
        import net_utils
    finally:
        sys.path.remove(REFERENCE_SRC)
    *frames, v01, v02 = kb.synthetic.make_triplet(2, *shape, kind, seed=3)
    inputs = frames + [net_utils.pose_matrix(v01), net_utils.pose_matrix(v02)]      # both precisions start from the fp32 matrices
    terms32, warp32 = _reference_outputs(net_utils, losses, inputs, torch.float32)
    terms64, warp64 = _reference_outputs(net_utils, losses, inputs, torch.float64)
    o32, o64 = lo.compute_loss(*inputs), lo.compute_loss(*[t.double() for t in inputs])
    for i, name in enumerate(SCALARS[:4]):
        assert _rel(o64[name], terms64[i]) <= 1e-12, name
        own, ref = _rel(o32[name], terms64[i]), _rel(terms32[i], terms64[i])
        print(f"{kind} {name}: oracle fp32 {own:.2e}, reference fp32 {ref:.2e}")
        assert own <= 2 * ref, name
    for i, name in enumerate(("image01", "image02")):
        assert float((o64[name] - warp64[i]).abs().max()) <= 1e-12
        own, ref = float((o32[name].double() - warp64[i]).abs().max()), float((warp32[i].double() - warp64[i]).abs().max())
        print(f"{kind} {name}: oracle fp32 {own:.2e}, reference fp32 {ref:.2e}")
        assert own <= 2 * ref, name


@pytest.mark.parametrize("name", CASES)
def test_frame_sums_are_the_terms_taken_apart(name):
    """lo.loss_sums (what the GPU tests gate ops.photometric_loss against, sum by sum) recombines into per_frame."""
    g = load_golden(name)
    args = [g[k].double() for k in INPUTS]
    sums, out = lo.loss_sums(*args), lo.compute_loss(*args)
    assert tuple(sums.shape) == (args[0].shape[0], 8) and sums.dtype == torch.float64
    assert lo.loss_sums(*[g[k] for k in INPUTS]).dtype == torch.float32
    got = kb.ops.loss_terms(sums, *args[0].shape[2:])
    assert all(_rel(a, b) <= 1e-12 for a, b in zip(got.flatten(), out["per_frame"].flatten()))
    if name in ("loss_general_camera", "loss_two_plane", "loss_weighted_validity", "loss_textured"):
        assert float((sums[:, 0] - sums[:, 1]).abs().min()) > 0 and float((sums[:, 2] - sums[:, 3]).abs().min()) > 0


def test_the_new_fixtures_are_what_they_claim():
    k = load_golden("loss_general_camera")["intrinsics"]
    assert bool(((k[:, 0, 0] / k[:, 1, 1] - 1).abs() >= 0.05).all()) and bool((k[:, 0, 1] != 0).all()) and not torch.equal(k[0], k[1])
    g = load_golden("loss_two_plane")
    step = (g["output_depth"][..., :, 1:] - g["output_depth"][..., :, :-1]).abs()
    assert float(step.max()) > 5 and float(step.median()) < 0.1
    assert set(load_golden("loss_weighted_validity")["validity_map"].unique().tolist()) == {0.0, 0.25, 1.0}
    smooth, rough = load_golden("loss_odd")["image0"], load_golden("loss_textured")["image0"]
    tv = lambda im: float((im[..., :, 1:] - im[..., :, :-1]).abs().mean())
    assert tv(rough) > 2 * tv(smooth)


# ---------------------------------------------------------------- the nearest stretch of the SSIM scores, restated on the host
def nearest_src_index(dst, in_size, out_size):
    """csrc/kbn_common.h nearest_src_index in numpy float32, operation for operation; `dst`: an int array."""
    if in_size == out_size:
        return dst
    if out_size == 2 * in_size:
        return dst >> 1
    scale = np.float32(in_size) / np.float32(out_size)
    s = np.floor(dst.astype(np.float32) * scale).astype(np.int64)
    return np.minimum(s, in_size - 1)


def ssim_axis_weight(s, size):
    """csrc/loss.hip ssim_axis_weight: how many of the `size` output pixels take score `s` of the (size - 2)-long axis, searched
    as the kernel searches them: d = s .. s + 3, d < size."""
    cnt = np.zeros_like(s)
    for k in range(4):
        d = s + k
        cnt += (d < size) & (nearest_src_index(np.minimum(d, size - 1), size - 2, size) == s)
    return cnt


def test_nearest_stretch_of_the_ssim_scores_for_every_length():
    """The kernel's index and weight against interpolate(mode='nearest') in fp32 and fp64, for every length from 3 to 2048; and the
    fact the weight's four-pixel search rests on: an output pixel is at most 2 past its source."""
    for size in range(3, 2049):
        d = np.arange(size)
        mine = nearest_src_index(d, size - 2, size)
        assert ((d - mine >= 0) & (d - mine <= 2)).all(), size
        weights = ssim_axis_weight(np.arange(size - 2), size)
        assert weights.sum() == size and weights.min() >= 1, size
        for dtype in (torch.float32, torch.float64):
            src = torch.arange(size - 2, dtype=dtype).reshape(1, 1, size - 2)
            want = torch.nn.functional.interpolate(src, size=size, mode="nearest").flatten().long()
            assert want.tolist() == mine.tolist(), (size, dtype)
            assert torch.bincount(want, minlength=size - 2).tolist() == weights.tolist(), (size, dtype)
        for dtype in (torch.float32, torch.float64) if size in (3, 4, 5, 17, 130, 257, 2048) else ():
            src = torch.arange(size - 2, dtype=dtype).reshape(1, 1, size - 2, 1).expand(1, 1, size - 2, 3).contiguous()   # 2-D, as the loss
            want = torch.nn.functional.interpolate(src, size=(size, 5), mode="nearest")[0, 0, :, 0].long()
            assert want.tolist() == mine.tolist(), (size, dtype)


# ---------------------------------------------------------------- host-side checks of the public surface (no GPU needed)
def _cpu_args(n=1, h=8, w=12):
    i0, i1, i2, depth, sparse, validity, k, v01, v02 = kb.synthetic.make_triplet(n, h, w, "void", seed=2)
    return [i0, i1, i2, depth, sparse, validity, k, kb.ops.pose_matrix(v01), kb.ops.pose_matrix(v02)]


def test_photometric_loss_rejects_cpu_tensors():
    with pytest.raises(kb._lib.KbnError, match="no CPU fallback"):
        kb.ops.photometric_loss(*_cpu_args())


def test_photometric_loss_rejects_mismatched_shapes_and_small_frames():
    a = _cpu_args()
    for i, bad in ((1, a[1][:, :, :-1]), (3, a[3][:, :, :, :-1]), (5, torch.cat([a[5], a[5]])), (6, a[6][:, :2]), (7, a[7][:, :3])):
        b = list(a)
        b[i] = bad
        with pytest.raises(kb._lib.KbnError, match="must be"):
            kb.ops.photometric_loss(*b)
    with pytest.raises(kb._lib.KbnError, match="3 x 3"):
        kb.ops.photometric_loss(*[t[:, :, :2] if t.dim() == 4 else t for t in a])
    with pytest.raises(kb._lib.KbnError, match="must be a tensor"):
        kb.ops.photometric_loss(*a[:8], None)
    with pytest.raises(kb._lib.KbnError):
        kb.ops.pose_matrix(torch.zeros(2, 5))


def test_compute_loss_argument_errors():
    m = kb.modules.KBNetModel.from_config(kb.kitti_config().narrow(), device=torch.device("cpu"))
    a = _cpu_args()
    with pytest.raises(kb._lib.KbnError, match="missing image0"):
        m.compute_loss()
    with pytest.raises(kb._lib.KbnError, match="missing pose02"):
        m.compute_loss(*a[:8])
    with pytest.raises(kb._lib.KbnError, match="no CPU fallback"):
        m.compute_loss(*a)
    with pytest.raises(kb._lib.KbnError, match="3 x 3"):
        m.compute_loss(*[t[:, :, :2] if t.dim() == 4 else t for t in a])
    with pytest.raises(kb._lib.KbnError, match="must be"):
        m.compute_loss(*a[:6], a[6][:, :2], *a[7:])
    with pytest.raises(kb._lib.KbnError):
        m.train()


def test_the_entry_point_checks_its_arguments():
    """Null pointers, sizes below 3 x 3 and one image output without the other: KBN_ERR_INVALID_ARGUMENT before anything is launched."""
    import ctypes
    lib = kb._lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    ok = [p] * 10 + [None, None]
    call = lambda ptrs, n, h, w: lib.kbn_photometric_loss_forward(*ptrs, n, h, w, None)
    assert call(ok, 1, 2, 8) == call(ok, 1, 8, 2) == call(ok, 0, 8, 8) == kb._lib.KBN_ERR_INVALID_ARGUMENT
    assert call([p] * 10 + [p, None], 1, 8, 8) == kb._lib.KBN_ERR_INVALID_ARGUMENT
    for i in range(10):
        assert call(ok[:i] + [None] + ok[i + 1:], 1, 8, 8) == kb._lib.KBN_ERR_INVALID_ARGUMENT


def test_make_triplet_is_deterministic_and_in_range():
    a, b = kb.synthetic.make_triplet(2, 9, 11, "kitti", seed=4), kb.synthetic.make_triplet(2, 9, 11, "kitti", seed=4)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(a[0], kb.synthetic.make_triplet(2, 9, 11, "kitti", seed=5)[0])
    for im in a[:3]:
        assert im.shape == (2, 3, 9, 11) and 0.0 <= float(im.min()) and float(im.max()) <= 1.0
    depth, sparse, validity = a[3:6]
    lo_, hi_ = kb.synthetic.FRAME_STATS["kitti"][1]
    assert lo_ <= float(depth.min()) and float(depth.max()) <= hi_
    assert torch.equal(validity, (sparse > 0).float()) and bool((validity.sum(dim=(1, 2, 3)) >= 1).all())
    assert a[7].shape == (2, 6)
