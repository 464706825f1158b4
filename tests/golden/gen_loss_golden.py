#!/usr/bin/env python3
"""Generate the golden vectors of the objective's forward value by RUNNING THE REFERENCE on CPU.

Run in the build container only (needs /root/reference):

    python tests/golden/gen_loss_golden.py

It imports the reference's `net_utils` and `losses` (read-only), composes them the way its KBNetModel.compute_loss does
(src/kbnet_model.py:238-292: backproject_to_camera, project_to_pixel, grid_sample, the four loss functions, the weighted sum)
and writes `loss_*.npz` next to this script: the inputs, the reference's fp32 outputs (`ref32::*`), the same functions evaluated
in fp64 (`ref64::*`: the inputs cast up and torch's default dtype set to float64, because the reference builds its meshgrid and
its homogeneous rows in the default dtype), and `dist::*`, the distance between the two (relative for the scalars, max abs for
the images): the reference's own fp32 rounding, which the tests' elementwise bounds are multiples of.  Nothing of the
reference's source is stored: the fixtures are data.

Cases (inputs from synthetic.make_triplet, band-limited images of radius 4)
  loss_even       2 x 40 x 56 kitti, moderate motion
  loss_odd        2 x 37 x 45 void
  loss_3x3        1 x 3 x 3, loss_3x4  2 x 3 x 4: the smallest legal sizes (one SSIM score, two scores)
  loss_identity   pose01 = identity and image1 = image0: image01 = image0 up to rounding
  loss_outside    a rotation that throws most samples outside the image (border padding)
  loss_behind     a translation along z beyond the largest depth: every point behind the camera, none within 0.5 m of z = 0
                  (near z = 0 the sample position jumps from one border to the other and fp32 and fp64 disagree by a whole
                  image, so no fixture goes there: asserted below for every case)
  loss_novalid    frame 1 has no valid sparse point: the sparse-depth term and the loss are NaN

Cases from tests/loss_cases.py (the inputs make_triplet does not produce; see its docstring)
  loss_general_camera     3 x 37 x 45: every frame its own K (fx != fy, skew, principal point off the centre) and its own poses
  loss_two_plane          2 x 37 x 45: a near and a far plane in 11 x 11 cells, the camera between them.  The only case with points
                          on both sides of the camera; |z| > 0.1 holds for it like for every other
  loss_weighted_validity  2 x 24 x 40: validity in {0, 0.25, 1}
  loss_textured           2 x 37 x 45: images of radius 1
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, "/root/reference/src")

import kbnet_amd as kb  # noqa: E402
import loss_cases  # noqa: E402  (tests/)
import losses  # noqa: E402  (reference)
import net_utils  # noqa: E402  (reference)

torch.set_grad_enabled(False)
WEIGHTS = (0.15, 0.95, 0.60, 0.04)   # reference src/kbnet_model.py:198-201
SCALARS = ("loss_color", "loss_structure", "loss_sparse_depth", "loss_smoothness", "loss")


def reference_loss(image0, image1, image2, depth, sparse, validity, k, pose01, pose02):
    """The reference's functions in the order of its compute_loss; the dtype of the inputs must be torch's default dtype."""
    shape = image0.shape
    ones = torch.ones_like(sparse)
    points = net_utils.backproject_to_camera(depth, k, shape)
    xy01 = net_utils.project_to_pixel(points, pose01, k, shape)
    xy02 = net_utils.project_to_pixel(points, pose02, k, shape)
    z = [torch.matmul(torch.matmul(torch.nn.functional.pad(k, (0, 1, 0, 1)), p)[:, :3], points)[:, 2] for p in (pose01, pose02)]
    outside = [float(((xy[:, 0] < 0) | (xy[:, 0] > shape[3] - 1) | (xy[:, 1] < 0) | (xy[:, 1] > shape[2] - 1)).double().mean())
               for xy in (xy01, xy02)]
    image01 = net_utils.grid_sample(image1, xy01, shape)
    image02 = net_utils.grid_sample(image2, xy02, shape)
    color = losses.color_consistency_loss_func(image01, image0, ones) + losses.color_consistency_loss_func(image02, image0, ones)
    structure = losses.structural_consistency_loss_func(image01, image0, ones) + \
        losses.structural_consistency_loss_func(image02, image0, ones)
    sparse_term = losses.sparse_depth_consistency_loss_func(depth, sparse, validity)
    smooth = losses.smoothness_loss_func(depth, image0)
    loss = WEIGHTS[0] * color + WEIGHTS[1] * structure + WEIGHTS[2] * sparse_term + WEIGHTS[3] * smooth
    out = {"loss_color": color, "loss_structure": structure, "loss_sparse_depth": sparse_term, "loss_smoothness": smooth,
           "loss": loss, "image01": image01, "image02": image02}
    return out, outside, (min(float(t.abs().min()) for t in z), [float(t.min()) for t in z], [float(t.max()) for t in z])


def evaluate(inputs):
    """(ref32, ref64, dist, fraction outside, closest |z|) of one case; `inputs`: fp32 tensors, poses as 4 x 4 matrices."""
    r32, _, _ = reference_loss(*inputs)
    torch.set_default_dtype(torch.float64)
    try:
        r64, outside, zinfo = reference_loss(*[t.double() for t in inputs])
    finally:
        torch.set_default_dtype(torch.float32)
    dist = {}
    for name in SCALARS:
        a, b = float(r32[name]), float(r64[name])
        dist[name] = 0.0 if (np.isnan(a) and np.isnan(b)) else abs(a - b) / abs(b)
    for name in ("image01", "image02"):
        dist[name] = float((r32[name].double() - r64[name]).abs().max())
    return r32, r64, dist, outside, zinfo


def save(name, vectors, inputs, r32, r64, dist, matrices64):
    keys = ("image0", "image1", "image2", "output_depth", "sparse_depth", "validity_map", "intrinsics", "pose01", "pose02")
    flat = {k: t.numpy() for k, t in zip(keys, inputs)}
    flat["pose01_vector"], flat["pose02_vector"] = vectors[0].numpy(), vectors[1].numpy()
    flat["pose01_fp64"], flat["pose02_fp64"] = matrices64[0].numpy(), matrices64[1].numpy()
    for grp, d in (("ref32", r32), ("ref64", r64)):
        for k, v in d.items():
            flat[f"{grp}::{k}"] = v.numpy()
    for k, v in dist.items():
        flat[f"dist::{k}"] = np.float64(v)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **flat)
    size = os.path.getsize(path)
    assert size < 1 << 20, (name, size)
    return size


def case(name, n, h, w, kind, seed, edit=None, radius=4, both_sides=False):
    i0, i1, i2, depth, sparse, validity, k, v01, v02 = kb.synthetic.make_triplet(n, h, w, kind, seed=seed, radius=radius)
    t = {"image0": i0, "image1": i1, "image2": i2, "depth": depth, "sparse": sparse, "validity": validity, "k": k, "v01": v01, "v02": v02}
    if edit:
        edit(t)
    vectors = (t["v01"], t["v02"])
    poses = [net_utils.pose_matrix(v) for v in vectors]
    torch.set_default_dtype(torch.float64)
    try:
        matrices64 = [net_utils.pose_matrix(v.double()) for v in vectors]
    finally:
        torch.set_default_dtype(torch.float32)
    inputs = (t["image0"], t["image1"], t["image2"], t["depth"], t["sparse"], t["validity"], t["k"], poses[0], poses[1])
    r32, r64, dist, outside, (closest, zmin, zmax) = evaluate(inputs)
    # no fixture near z = 0 (see the module docstring): points stay clearly in front of the camera, or (loss_behind, which
    # asserts its own 0.5 m) clearly behind it; `both_sides` (loss_two_plane alone) has points on either side, none near z = 0
    assert closest > 0.1 and (both_sides or min(zmin) > 0 or max(zmax) < 0), (name, closest, zmin, zmax)
    assert not both_sides or (min(zmin) < 0 < max(zmax)), (name, zmin, zmax)
    size = save(name, vectors, inputs, r32, r64, dist, matrices64)
    print(f"{name}: {size / 1024:.0f} KiB  outside {outside[0]:.3f} / {outside[1]:.3f}  z in [{min(zmin):.2f}, {max(zmax):.2f}]  "
          + "  ".join(f"{k} {float(r64[k]):.6g} (fp32 {dist[k]:.1e})" for k in SCALARS)
          + f"  image01 {dist['image01']:.1e}  image02 {dist['image02']:.1e}")
    return outside, zmax


def main():
    case("loss_even", 2, 40, 56, "kitti", 11)
    case("loss_odd", 2, 37, 45, "void", 12)
    case("loss_3x3", 1, 3, 3, "void", 13)
    case("loss_3x4", 2, 3, 4, "kitti", 14)

    def identity(t):
        t["v01"] = torch.zeros_like(t["v01"])
        t["image1"] = t["image0"].clone()
    case("loss_identity", 2, 24, 40, "kitti", 15, identity)

    def outside(t):
        t["v01"][:, :3] = torch.tensor([0.03, 0.65, 0.02])     # ~37 degrees about y: most of the view leaves the image,
                                                                # and with the 40 degree half field of view no ray reaches 90
        t["v02"][:, :3] = torch.tensor([-0.7, -0.05, 0.03])
    out, _ = case("loss_outside", 2, 32, 48, "kitti", 16, outside)
    assert min(out) > 0.5, out

    def behind(t):
        far = float(t["depth"].max())
        t["v01"][:, 5] = -(far + 2.0)                           # every point ends up behind the camera
        t["v02"][:, 5] = -(far + 5.0)
    _, zmax = case("loss_behind", 2, 24, 40, "void", 17, behind)
    assert max(zmax) < -0.5, zmax

    def novalid(t):
        t["sparse"][1] = 0
        t["validity"][1] = 0
    case("loss_novalid", 2, 24, 40, "kitti", 18, novalid)

    def family(name, seed):
        return lambda t: loss_cases.apply(t, (name,), seed)
    case("loss_general_camera", 3, 37, 45, "void", 41, family("general_camera", 41))
    case("loss_two_plane", 2, 37, 45, "kitti", 42, family("two_plane", 42), both_sides=True)
    case("loss_weighted_validity", 2, 24, 40, "kitti", 43, family("weighted_validity", 43))
    case("loss_textured", 2, 37, 45, "void", 44, radius=loss_cases.radius(("textured",)))


if __name__ == "__main__":
    main()
