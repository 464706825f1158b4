"""CPU: the switches of the pose network's training path that need no GPU -- what they set, what they refuse."""
import pytest
import torch

import kbnet_amd as kb
KbnError = kb._lib.KbnError

CPU = torch.device("cpu")
NARROW = [8, 16, 16, 32, 32, 24, 40]


def test_requires_grad_sets_every_parameter_and_defaults_stay_off():
    m = kb.modules.PoseNetModel(device=CPU, n_filters=NARROW)
    assert len(m.parameters()) == 22 and not any(p.requires_grad for p in m.parameters())
    assert m.batch_norm_mode == "running"
    assert m.requires_grad_(True) is m and all(p.requires_grad for p in m.parameters())
    assert m.requires_grad_(False) is m and not any(p.requires_grad for p in m.parameters())
    assert m.requires_grad_() is m and all(p.requires_grad for p in m.parameters())
    assert not m.encoder.training and not m.encoder.conv1.batch_norm.training      # the modules stay in eval mode
    with pytest.raises(KbnError, match="inference only"):
        m.train()


def test_set_batch_norm_takes_two_modes():
    m = kb.modules.PoseNetModel(device=CPU, n_filters=NARROW)
    assert m.set_batch_norm("batch") is m and m.batch_norm_mode == "batch"
    assert m.set_batch_norm() is m and m.batch_norm_mode == "running"
    for bad in ("train", "eval", None, True):
        with pytest.raises(KbnError):
            m.set_batch_norm(bad)
    assert m.batch_norm_mode == "running"
    assert not m.encoder.conv1.batch_norm.training


def test_resnet_pose_networks_have_no_backward_yet():
    r = kb.posenet_resnet.ResNetPoseNetModel(n_layer=18, device=CPU, n_filters=[8, 8, 16, 16, 32], decoder_filters=[16, 16])
    with pytest.raises(KbnError, match="posenet"):
        r.requires_grad_(True)
    assert not any(p.requires_grad for p in r.parameters())
    r.requires_grad_(False)


def test_the_new_operators_refuse_cpu_tensors():
    x, g, v = torch.zeros(1, 2, 4, 4), torch.zeros(1, 3, 2, 2), torch.ones(3)
    for fn in (lambda: kb.ops.conv2d_s2_backward_weight([x], g, 3),
               lambda: kb.ops.conv2d_s2_backward_data(g, torch.zeros(16), (2,), 3, 4, 4),
               lambda: kb.ops.pack_conv2d_s2_backward_data_weight(torch.zeros(3, 2, 3, 3)),
               lambda: kb.ops.batch_norm_stats(x),
               lambda: kb.ops.batch_norm_act(g, v, v, v, v),
               lambda: kb.ops.batch_norm_act_backward(g, g, v, v, v, v),
               lambda: kb.ops.conv2d_s2([x], torch.zeros(3, 2, 3, 3))):
        with pytest.raises(KbnError):
            fn()
