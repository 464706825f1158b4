"""GPU: the pose head (csrc/posenet.hip, kbn_pose_head_forward) against ops.pose_matrix over many pose vectors.

ops.pose_matrix evaluates |r| as sqrt((r0 r0 + r1 r1) + r2 r2), every product and sum an operation of its own, as pose_from_dof in the
kernel does.  With torch.linalg.vector_norm in its place the two differed by 1 ulp of the angle for about one vector in nine
(profiles/r08/resnet_pose.md): a rule the model tests, with a handful of vectors each, met only by chance.

    python -m pytest tests -m gpu -q
"""
import pytest
import torch

import kbnet_amd as kb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need a visible MI355X (run with -m gpu on a GPU box)")
    kb._lib.load()   # a missing extension is an error on a GPU box, never a skip
    return torch.device("cuda:0")


def test_pose_head_equals_pose_matrix_over_a_sweep(dev):
    """4096 pose vectors at each of two sizes through the head kernel alone (1 x 1 latents, identity weight): the matrix equals
    ops.pose_matrix of the kernel's own dof, evaluated on the device, bit for bit for EVERY one of them.  A handful of model
    forwards cannot show a rule that fails for one vector in nine (torch's own norm rounds the angle's sum another way than
    sqrt((r0 r0 + r1 r1) + r2 r2); ops.pose_matrix spells the sum out)."""
    g = torch.Generator().manual_seed(1)
    weight = torch.eye(6, device=dev).view(6, 6, 1, 1).contiguous()
    for scale in (1.0, 100.0):                               # |dof| about 1e-2 (what the networks give) and about 1
        latent = (scale * torch.randn(4096, 6, 1, 1, generator=g)).to(dev)
        pose, dof = kb.ops.pose_head(latent, weight, return_dof=True)
        bad = int((pose != kb.ops.pose_matrix(dof)).flatten(1).any(1).sum())
        print(f"pose_head sweep, scale {scale:g}: {bad} / 4096 frames differ from ops.pose_matrix(dof)")
        assert bad == 0
        assert len({tuple(r) for r in dof[:64].cpu().tolist()}) == 64
