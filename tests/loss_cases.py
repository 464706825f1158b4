"""Argument lists of KBNetModel.compute_loss that synthetic.make_triplet does not produce, shared by the CPU and the GPU loss
tests and by tests/golden/gen_loss_golden.py: test infrastructure, never imported by the package.

make_triplet gives every frame the same symmetric camera (fx == fy, no skew, the principal point at the frame centre), a smooth
depth wholly in front of the camera, a validity of 0 or 1 and images box-filtered with radius 4.  A kernel that reads frame 0's
camera for every frame, swaps fx with fy or drops K^-1's off-diagonal entries computes the same numbers on such inputs.  The
families below are edits of make_triplet's output (make_triplet itself feeds committed fixtures and stays as it is):

  general_camera     every frame its own K: fx != fy by more than 5 %, a skew of 1-3 pixels, the principal point 1.25-3.75 pixels
                     off the centre by a non-integer amount; both pose vectors of every frame its own, 0.015-0.04 rad about each
                     of the three axes
  two_plane          depth = a near (2 m) and a far (12 m) plane in a checkerboard of 11 x 11 cells (11 divides neither 16 nor
                     64: the steps fall at varying places inside the 64 x 16 tiles) + 0.3 m of the smooth depth; both poses move
                     the camera 4.5-5 m forward, between the planes.  Asserted: 20-80 % of the points are behind the camera and
                     no |z| is below 0.1 (the rule of gen_loss_golden.py: near z = 0 the sample position jumps between borders)
  weighted_validity  validity in {0, 0.25, 1}: a quarter-weight point on about 3 % of the pixels, each with a sparse depth
  textured           images box-filtered with radius 1 instead of 4 (an argument of make_triplet, see `build`)
  everything         all four

CASES is the table both test files parametrise over: one case inside a single 64 x 16 tile, the others over several tiles with
ragged last tiles in both directions.
"""
import numpy as np
import torch

import kbnet_amd as kb

import loss_oracle as lo

FAMILIES = ("general_camera", "two_plane", "weighted_validity", "textured")
KEYS = ("image0", "image1", "image2", "depth", "sparse", "validity", "k", "v01", "v02")

#        name                          families                  n   h    w   kind    seed
CASES = {
    "general_camera_13x40":    dict(families=("general_camera",), n=2, h=13, w=40, kind="void", seed=31),
    "general_camera_70x100":   dict(families=("general_camera",), n=3, h=70, w=100, kind="kitti", seed=32),
    "two_plane_37x45":         dict(families=("two_plane",), n=2, h=37, w=45, kind="void", seed=33),
    "two_plane_50x130":        dict(families=("two_plane",), n=2, h=50, w=130, kind="kitti", seed=34),
    "weighted_validity_37x45": dict(families=("weighted_validity",), n=2, h=37, w=45, kind="kitti", seed=35),
    "textured_70x100":         dict(families=("textured",), n=2, h=70, w=100, kind="void", seed=36),
    "everything_37x45":        dict(families=FAMILIES, n=3, h=37, w=45, kind="void", seed=37),
    "everything_50x130":       dict(families=FAMILIES, n=3, h=50, w=130, kind="kitti", seed=38),
}


def _rng(seed):
    return np.random.Generator(np.random.Philox(seed))


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def general_camera(t, seed):
    n, _, h, w = t["image0"].shape
    g = _rng(seed + 1000)
    k = t["k"].double().numpy().copy()
    f = k[:, 0, 0].copy()
    k[:, 0, 0] = f * (1.02 + 0.25 * g.random(n))
    k[:, 1, 1] = f * (0.70 + 0.22 * g.random(n))
    k[:, 0, 1] = (1.0 + 2.0 * g.random(n)) * np.where(g.random(n) < 0.5, -1.0, 1.0)
    for col in (0, 1):
        k[:, col, 2] += (1.25 + 2.5 * g.random(n)) * np.where(g.random(n) < 0.5, -1.0, 1.0)
    t["k"] = _f32(k)
    for name in ("v01", "v02"):
        v = t[name].double().numpy().copy()
        v[:, :3] = (0.015 + 0.025 * g.random((n, 3))) * np.where(g.random((n, 3)) < 0.5, -1.0, 1.0)
        t[name] = _f32(v)
    k = t["k"]
    assert bool(((k[:, 0, 0] / k[:, 1, 1] - 1).abs() >= 0.05).all()) and bool((k[:, 0, 1] != 0).all())
    off = torch.stack([k[:, 0, 2] - 0.5 * (w - 1), k[:, 1, 2] - 0.5 * (h - 1)], 1)
    assert bool((off.abs() > 1).all()) and bool(((off - off.round()).abs() > 0.01).all()), off
    if n > 1:
        assert len({tuple(m.flatten().tolist()) for m in k}) == n, "every frame a camera of its own"


def camera_z(t):
    """fp64 z of every point in the two neighbour cameras: N x 2 x HW."""
    d, k = t["depth"].double(), t["k"].double()
    h, w = d.shape[2:]
    pts = lo.backproject(d, k)
    k4 = torch.zeros(k.shape[0], 4, 4, dtype=torch.float64)
    k4[:, :3, :3] = k
    k4[:, 3, 3] = 1
    return torch.stack([torch.matmul(torch.matmul(k4, lo.pose_matrix(t[v].double()))[:, :3], pts)[:, 2] for v in ("v01", "v02")], 1)


def two_plane(t, seed):
    n, _, h, w = t["image0"].shape
    d = t["depth"].double()
    lo_, hi_ = d.amin(dim=(1, 2, 3), keepdim=True), d.amax(dim=(1, 2, 3), keepdim=True)
    smooth = 0.3 * (d - lo_) / (hi_ - lo_).clamp_min(1e-12)
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    near = ((xs // 11 + ys // 11) % 2 == 0)[None, None]
    t["depth"] = (torch.where(near, 2.0, 12.0) + smooth).float()
    g = _rng(seed + 2000)
    for name, forward in (("v01", 4.5), ("v02", 5.0)):
        v = t[name].clone()
        v[:, 3:5] *= 0.3 / max(float(v[:, 3:5].abs().max()), 0.3)        # at most 0.3 m sideways
        v[:, 5] = -_f32(forward + 0.2 * g.random(n))                       # the scene moves towards the camera: the camera moves forward
        t[name] = v
    z = camera_z(t)
    behind = float((z < 0).double().mean())
    assert 0.2 <= behind <= 0.8 and float(z.abs().min()) >= 0.1, (behind, float(z.abs().min()))


def weighted_validity(t, seed):
    g = _rng(seed + 3000)
    shape = tuple(t["validity"].shape)
    quarter = torch.from_numpy(g.random(shape) < 0.03) & (t["validity"] == 0)
    quarter.reshape(shape[0], -1)[:, 0] = True                               # never a frame without a quarter-weight point
    noisy = (t["depth"].double() * (1.0 + 0.01 * torch.from_numpy(g.standard_normal(shape))) * 256.0).round() / 256.0
    t["sparse"] = torch.where(quarter, noisy.float(), t["sparse"])
    t["validity"] = torch.where(quarter, 0.25, t["validity"])
    for v in t["validity"]:
        assert {0.0, 0.25, 1.0} == set(v.unique().tolist())


def apply(t, families, seed):
    """Edits the dict `t` (KEYS -> make_triplet's tensors) in place.  `textured` is make_triplet's radius and is not applied here.
    two_plane comes after general_camera: it asserts its z rule on the cameras the case ends up with."""
    assert set(families) <= set(FAMILIES), families
    if "general_camera" in families:
        general_camera(t, seed)
    if "weighted_validity" in families:
        weighted_validity(t, seed)
    if "two_plane" in families:
        two_plane(t, seed)
    return t


def radius(families):
    return 1 if "textured" in families else 4


def build(families, n, h, w, kind, seed):
    """-> the nine arguments of compute_loss as CPU fp32 tensors, the poses as 4 x 4 matrices (loss_oracle.pose_matrix, which equals
    the reference's bit for bit on the fixtures)."""
    t = dict(zip(KEYS, kb.synthetic.make_triplet(n, h, w, kind, seed=seed, radius=radius(families))))
    apply(t, families, seed)
    return [t[k] for k in KEYS[:7]] + [lo.pose_matrix(t["v01"]), lo.pose_matrix(t["v02"])]


def case(name):
    return build(**CASES[name])
