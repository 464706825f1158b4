"""GPU: the pose networks' implicit-GEMM convs (csrc/pose_igemm.h and its three kernels) reproduce, bit for bit, the outputs
pinned in tests/golden/pose_conv_digests.json: one SHA-256 per case of tools/pose_conv_digest.py (its case list is imported,
not copied).  The file was written by the build that preceded csrc/pose_igemm.h, so a refactor of these kernels that changes
any output bit fails here.

Regenerating the file is legitimate in one situation only: a pull request that INTENDS to change these kernels' summation
order (another K chunk, split-K, another tile), says so, and is gated by the tolerance tests (test_posenet_gpu.py,
test_resnet_pose_gpu.py, test_posenet_backward_gpu.py).  Then, on the GPU box:

    python tools/pose_conv_digest.py --write tests/golden/pose_conv_digests.json

    python -m pytest tests -m gpu -q
"""
import importlib.util
import json
import os

import pytest
import torch

import kbnet_amd as kb

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("pose_conv_digest", os.path.join(os.path.dirname(HERE), "tools", "pose_conv_digest.py"))
tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tool)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need a visible MI355X (run with -m gpu on a GPU box)")
    kb._lib.load()   # a missing extension is an error on a GPU box, never a skip
    return torch.device("cuda:0")


def test_pose_convs_reproduce_the_pinned_digests(dev):
    with open(os.path.join(HERE, "golden", "pose_conv_digests.json")) as f:
        want = json.load(f)
    got = tool.digests(dev)
    assert list(got) == list(want)                       # the case list and the file go together
    assert len(set(got.values())) == len(got)            # no two cases hash the same bytes
    wrong = [name for name in got if got[name] != want[name]]
    assert not wrong, wrong
