"""CPU: how far ops.pose_matrix is from the reference's form.  |r| is sqrt((r0 r0 + r1 r1) + r2 r2) with every product and sum rounded on
its own -- the arithmetic of pose_from_dof in csrc/posenet.hip, so that the head kernel has fixed bits to reproduce -- where the
reference takes torch.norm (src/net_utils.py:1556-1562), whose rounding of the sum is torch's own and differs between the CPU and
the device.

Bounds, from the formats (u = 2^-24, the unit roundoff): every term of the sum carries its square's rounding and at most two sums',
(1 + u)^3, so the fp32 sum is within 3 u (relative) of the exact one; the square root halves that and rounds once more: 2.5 u from the
exact norm, for any order of the three terms, so two such forms are at most 5 u <= 5 ulp apart (observed: 1.85 u, 2 ulp).  cos, sin
and the axis move by no more than the angle does, 5 u |r|: matrices within 20 u max(1, |r|) (a few u more for the entries' own sums).
"""
import torch

import kbnet_amd as kb


def _vectors(scale, n=20000, seed=3):
    g = torch.Generator().manual_seed(seed)
    return scale * torch.randn(n, 6, generator=g)


def _reference_form(v):
    """ops.pose_matrix with the reference's norm, in the dtype of v."""
    r = v[:, :3]
    angle = torch.norm(r.unsqueeze(1), 2, 2, True)[:, 0]
    axis = r / (angle + 1e-7)
    ca, sa = torch.cos(angle[:, 0]), torch.sin(angle[:, 0])
    c = 1 - ca
    x, y, z = axis[:, 0], axis[:, 1], axis[:, 2]
    rows = [x * x * c + ca, x * y * c - z * sa, z * x * c + y * sa, x * y * c + z * sa, y * y * c + ca, y * z * c - x * sa,
            z * x * c - y * sa, y * z * c + x * sa, z * z * c + ca]
    return torch.stack(rows, dim=1).reshape(-1, 3, 3)


def test_angle_is_within_the_formats_bound_of_the_exact_norm_and_of_torch_norm():
    for scale in (1e-2, 1.0, 30.0):
        r = _vectors(scale)[:, :3]
        ours = torch.sqrt((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2])
        ref = torch.norm(r.unsqueeze(1), 2, 2, True)[:, 0, 0]
        ulps = (ours.view(torch.int32) - ref.view(torch.int32)).abs()
        exact = torch.sqrt((r.double() ** 2).sum(1))
        rel = float(((ours.double() - exact).abs() / exact).max())
        print(f"scale {scale:g}: {int((ulps > 0).sum())} of {len(r)} angles differ from torch.norm, at most {int(ulps.max())} ulp; "
              f"from the exact norm {rel * 2 ** 24:.2f} x 2^-24")
        assert int(ulps.max()) <= 5
        assert rel <= 2.5 * 2.0 ** -24


def test_matrix_is_within_the_angles_distance_of_the_reference_form():
    for scale in (1e-2, 1.0, 30.0):
        v = _vectors(scale)
        m = kb.ops.pose_matrix(v)
        tol = 20 * 2.0 ** -24 * max(1.0, float(v[:, :3].norm(dim=1).max()))
        assert float((m[:, :3, :3] - _reference_form(v)).abs().max()) <= tol
        assert float((m[:, :3, :3].double() - _reference_form(v.double())).abs().max()) <= tol                         # both are the rotation
        assert torch.equal(m[:, :3, 3], v[:, 3:]) and torch.equal(m[:, 3], torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(len(v), 4))
        assert torch.equal(m, kb.ops.pose_matrix(v.clone()))
