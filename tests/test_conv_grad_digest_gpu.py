"""GPU: the conv gradients of the three trainable networks reproduce, bit for bit, the outputs pinned in
tests/golden/conv_grad_digests.json: one SHA-256 per case of the gradient list of tools/pose_conv_digest.py (`--grad`; the list is
imported, not copied) -- both weight-gradient entry points at every (kernel size, stride), filter tile and split, conv2d_backward_data,
the recorded conv nodes, and one backward through each trainable model.  The file was written with the library built from the commit
that preceded csrc/conv_bwd_weight.hip and the one recorded conv node of ops.py (that commit's libkbnet_hip.so through KBN_LIB_PATH, as
the tool's docstring describes), so a refactor of these gradients that changes any output bit fails here.

Regenerating the file is legitimate in one situation only: a pull request that INTENDS to change a summation order of these gradients
(another split plan, another tile, a four-parity-class data gradient), says so, and is gated by the tolerance tests
(test_posenet_backward_gpu.py, test_resnet_pose_backward_gpu.py, test_kbnet_backward_gpu.py and the *_train_gpu.py files).  Then, on
the GPU box:

    python tools/pose_conv_digest.py --grad --write tests/golden/conv_grad_digests.json

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


def test_conv_gradients_reproduce_the_pinned_digests(dev):
    with open(os.path.join(HERE, "golden", "conv_grad_digests.json")) as f:
        want = json.load(f)
    got = tool.digests(dev, grad=True)
    assert list(got) == list(want)                       # the case list and the file go together
    assert len(set(got.values())) == len(got)            # no two cases hash the same bytes
    wrong = [name for name in got if got[name] != want[name]]
    assert not wrong, wrong
