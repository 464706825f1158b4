"""CPU (no kernel runs): KBNetModel's `trainable` switch, what it refuses at construction, and what stays as it was."""
import dataclasses

import pytest
import torch

import kbnet_amd as kb
KbnError = kb._lib.KbnError

CPU = torch.device("cpu")


def _model(cfg, **kw):
    return kb.modules.KBNetModel.from_config(cfg, CPU, **kw)


def test_the_switch_changes_no_parameter_and_no_key():
    cfg = kb.kitti_config().narrow()
    plain, m = _model(cfg), _model(cfg, trainable=True)
    assert [tuple(p.shape) for p in plain.parameters()] == [tuple(p.shape) for p in m.parameters()]
    for a, b in zip(plain.modules(), m.modules()):
        assert list(a.state_dict()) == list(b.state_dict())
    assert m.parameters() is not m.parameters() and all(isinstance(p, torch.nn.Parameter) for p in m.parameters())
    direct = kb.modules.KBNetModel(3, 2, [5, 7], [9], 3, 8, [8, 16, 32, 64, 64], [4, 8, 16, 32, 32], [0, 1, 2, 3], [32, 16, 16, 8, 4],
                                   device=CPU, trainable=True)
    assert direct._has_backward and not plain._has_backward


def test_requires_grad_and_train():
    cfg = kb.kitti_config().narrow()
    m = _model(cfg, trainable=True)
    assert m.requires_grad_(False) is m and not any(p.requires_grad for p in m.parameters())
    assert m.requires_grad_(True) is m and all(p.requires_grad for p in m.parameters())
    with pytest.raises(KbnError, match="inference only"):
        m.train()
    assert all(mod.training is False for top in m.modules() for mod in top.modules())
    plain = _model(cfg)
    with pytest.raises(KbnError, match="trainable=True"):
        plain.requires_grad_(True)
    assert plain.requires_grad_(False) is plain
    with pytest.raises(KbnError, match="inference only"):
        plain.train()


@pytest.mark.parametrize("change, word", [(dict(deconv_type="transpose"), "deconv_type"), (dict(activation_func="elu"), "elu"),
                                          (dict(activation_func="sigmoid"), "sigmoid")])
def test_construction_refuses_what_is_not_differentiated(change, word):
    cfg = dataclasses.replace(kb.kitti_config().narrow(), **change)
    _model(cfg)                                  # the inference model takes it
    with pytest.raises(KbnError, match=word):
        _model(cfg, trainable=True)


@pytest.mark.parametrize("change", [dict(activation_func="relu"), dict(activation_func="linear"), dict(resolutions_backprojection=(0, 2)),
                                    dict(resolutions_backprojection=(0,)),
                                    dict(resolutions_backprojection=(0, 1, 2, 3, 4), n_filters_encoder_image=(8, 16, 32, 32, 32),
                                         n_filters_encoder_depth=(4, 8, 16, 16, 16))])
def test_construction_takes_every_supported_form(change):
    assert _model(dataclasses.replace(kb.void_config().narrow(), **change), trainable=True)._has_backward


def test_cpu_tensors_are_refused_on_the_recorded_path_too():
    """No CPU path: the recorded forward fails loudly at its first kernel, and data that requires grad before that."""
    m = _model(kb.kitti_config().narrow(), trainable=True)
    frames = kb.synthetic.make_frames(1, 17, 19)
    with pytest.raises(KbnError, match="image"):
        m.forward(frames[0].clone().requires_grad_(True), *frames[1:])
    with pytest.raises(KbnError, match="out="):
        m.forward(*frames, out=torch.empty(1, 1, 17, 19))
    with pytest.raises(KbnError, match="return_logits"):
        m.forward(*frames, return_logits=True)
    with pytest.raises(RuntimeError):
        m.forward(*frames)
    with torch.no_grad():
        with pytest.raises(KbnError, match="return_inner"):
            m.forward(*frames, return_inner=True)


def test_activation_names_are_shared_with_the_oracle():
    import kbnet_grad_oracle as kgo
    assert kgo.activation_names is kb.kbnet_train.activation_names
    names = kb.kbnet_train.activation_names((0, 1, 2, 3))
    assert names[:6] == ["s2d.pool_convs.0", "s2d.pool_convs.1", "s2d.pool_convs.2", "s2d.conv", "conv0_image", "conv0_depth"]
    assert names[6:10] == ["level0.conv_image", "level0.conv_depth", "level0.proj_depth", "level0.conv_fused"]
    assert names[-2:] == ["deconv0.deconv", "deconv0.conv"]
