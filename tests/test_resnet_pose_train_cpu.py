"""CPU: the switches of the ResNet pose networks' training path that need no GPU -- what they set, what they refuse."""
import pytest
import torch

import kbnet_amd as kb
KbnError = kb._lib.KbnError

CPU = torch.device("cpu")
NARROW = dict(n_filters=[8, 12, 16, 16, 32], decoder_filters=[16, 16])


def test_the_default_model_still_refuses_and_names_the_switch():
    r = kb.posenet_resnet.ResNetPoseNetModel(n_layer=18, device=CPU, **NARROW)
    with pytest.raises(KbnError, match="posenet") as e:
        r.requires_grad_(True)
    assert "trainable=True" in str(e.value)
    assert not any(p.requires_grad for p in r.parameters())
    assert r.requires_grad_(False) is r
    with pytest.raises(KbnError, match="trainable=True"):
        r.set_batch_norm("batch")
    assert r.batch_norm_mode == "running"


@pytest.mark.parametrize("n_layer, count", [(18, 8), (34, 16)])
def test_trainable_accepts_requires_grad_and_returns_self(n_layer, count):
    r = kb.posenet_resnet.ResNetPoseNetModel(n_layer=n_layer, device=CPU, trainable=True, **NARROW)
    params = r.parameters()
    # conv1, per block two convs with BatchNorm2d and a projection, two decoder layers, the head
    assert len(params) == 3 + count * 7 + 2 * 3 + 1 and not any(p.requires_grad for p in params)
    assert r.requires_grad_(True) is r and all(p.requires_grad for p in r.parameters())
    assert r.requires_grad_(False) is r and not any(p.requires_grad for p in r.parameters())
    assert r.requires_grad_() is r and all(p.requires_grad for p in r.parameters())
    assert not r.encoder.training and not r.encoder.conv1.batch_norm.training and not r.decoder.training
    with pytest.raises(KbnError, match="inference only"):
        r.train()
    assert not r.encoder.training


def test_set_batch_norm_takes_two_modes():
    r = kb.posenet_resnet.ResNetPoseNetModel(n_layer=18, device=CPU, trainable=True, **NARROW)
    assert r.batch_norm_mode == "running"
    assert r.set_batch_norm("batch") is r and r.batch_norm_mode == "batch"
    assert r.set_batch_norm() is r and r.batch_norm_mode == "running"
    for bad in ("train", "eval", None, True):
        with pytest.raises(KbnError):
            r.set_batch_norm(bad)
    assert r.batch_norm_mode == "running"
    assert not r.encoder.blocks2[0].conv1.batch_norm.training


def test_load_pose_model_passes_trainable_through(tmp_path):
    path = str(tmp_path / "pose.pth")
    src = kb.posenet_resnet.ResNetPoseNetModel(n_layer=18, device=CPU, **NARROW)
    src.save_model(path, step=7)
    plain = kb.modules.load_pose_model(path, device=CPU)
    with pytest.raises(KbnError, match="posenet"):
        plain.requires_grad_(True)
    m = kb.modules.load_pose_model(path, device=CPU, trainable=True)
    assert isinstance(m, kb.posenet_resnet.ResNetPoseNetModel) and m.n_layer == 18
    assert m.requires_grad_(True) is m and all(p.requires_grad for p in m.parameters())
    assert torch.equal(m.encoder.blocks2[0].projection.conv.weight, src.encoder.blocks2[0].projection.conv.weight)
    assert tuple(m.encoder.blocks2[0].projection.conv.weight.shape) == (12, 8, 1, 1)
    # the seven-conv network ignores the flag: it always has its backward pass
    path7 = str(tmp_path / "pose7.pth")
    kb.modules.PoseNetModel(device=CPU, n_filters=[8, 16, 16, 32, 32, 24, 40]).save_model(path7)
    p = kb.modules.load_pose_model(path7, device=CPU, trainable=False)
    assert isinstance(p, kb.modules.PoseNetModel) and p.requires_grad_(True) is p


def test_return_inner_on_the_fused_path_raises():
    image = torch.zeros(1, 3, 32, 32)
    for trainable in (False, True):
        r = kb.posenet_resnet.ResNetPoseNetModel(n_layer=18, device=CPU, trainable=trainable, **NARROW)
        with pytest.raises(KbnError, match="return_inner"):
            r.forward(image, image, return_inner=True)
    r.requires_grad_(True)
    with torch.no_grad():
        with pytest.raises(KbnError, match="return_inner"):
            r.forward(image, image, return_all=True, return_inner=True)


def test_an_image_that_requires_grad_is_named():
    r = kb.posenet_resnet.ResNetPoseNetModel(n_layer=18, device=CPU, trainable=True, **NARROW).requires_grad_(True)
    image = torch.zeros(1, 3, 32, 32)
    with pytest.raises(KbnError, match="image1"):
        r.forward(image, image.clone().requires_grad_(True))


def test_the_new_operators_refuse_cpu_tensors():
    x, g, w3, w1 = torch.zeros(1, 2, 4, 4), torch.zeros(1, 3, 4, 4), torch.zeros(3, 2, 3, 3), torch.zeros(3, 2, 1, 1)
    g2 = torch.zeros(1, 3, 2, 2)
    for fn in (lambda: kb.ops.conv2d_backward_weight([x], g, 3, 1),
               lambda: kb.ops.conv2d_backward_weight([x], g2, 1, 2),
               lambda: kb.ops.pack_conv2d_backward_data_weight(w3, 1),
               lambda: kb.ops.pack_conv2d_backward_data_weight(w1, 2),
               lambda: kb.ops.conv2d_backward_data(g, torch.zeros(16), 2, 3, 1, 4, 4),
               lambda: kb.ops.conv2d_backward_data(g2, torch.zeros(6), 2, 1, 2, 4, 4),
               lambda: kb.ops.conv2d_pose([x], w3, 1),
               lambda: kb.ops.conv2d_pose([x], w1.requires_grad_(True), 2),
               lambda: kb.ops.maxpool3x3s2_backward(x, torch.zeros(1, 2, 2, 2)),
               lambda: kb.ops.maxpool3x3s2(x.clone().requires_grad_(True)),
               lambda: kb.ops.add_act(x, x, 0.2),
               lambda: kb.ops.add_act(x.clone().requires_grad_(True), x, None),
               lambda: kb.ops.add_act_backward(x, x, 0.0)):
        with pytest.raises(KbnError):
            fn()
