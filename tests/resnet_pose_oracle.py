"""CPU restatement of the ResNet-18/34 pose network's eval-mode forward in plain torch, for the tests (the role tests/posenet_oracle.py
has for the seven-conv network): reference src/posenet_model.py:55-112, src/networks.py:674-996 and 1992-2075, src/net_utils.py:51-141
and 572-667.

    x = cat[image0, image1]                                         6 channels
    cba(x, k, s) = act(conv_{k, stride s, padding k // 2}(x) * scale + shift)       scale, shift: BatchNorm2d.eval(), eps = 1e-5
    conv1 = cba(x, 7, 2);   pool = max_pool(conv1, 3, stride 2, padding 1: padding never wins)
    stages blocks2 .. blocks5, [2, 2, 2, 2] or [3, 4, 6, 3] blocks; the first block of blocks3 .. blocks5 has stride 2:
        h = cba(x, 3, s);  g = cba(h, 3, 1)  (WITH its activation);  X = x, or conv_{1 x 1, stride s}(x) when shape or channels differ
        x = act(g + X)
    decoder: cba(x, 3, 2) for every hidden layer, map = conv_{1 x 1}(x), dof = 0.01 * mean_hw(map), pose = ops.pose_matrix(dof)

Runs in the dtype of its inputs (posenet_oracle.to64 for the fp64 form); the fp32 form rounds the two multiply-adds of the affine once
each, as posenet_oracle does.  The keyword arguments are the MISTAKES tests/test_resnet_pose_cpu.py plants; their defaults are the network.
`names(n_layer, n_hidden)` lists the layer outputs in the order `forward` and ResNetPoseNetModel.forward(return_all=True) give them.
"""
import torch
import torch.nn.functional as F

import kbnet_amd as kb

from posenet_oracle import EPS, _fma, strip

BLOCKS = {18: (2, 2, 2, 2), 34: (3, 4, 6, 3)}


def names(n_layer=18, n_hidden=2):
    out = ["conv1", "pool"]
    for stage, count in enumerate(BLOCKS[n_layer], 2):
        out += [f"blocks{stage}.{b}" for b in range(count)]
    return out + [f"decoder{i}" for i in range(n_hidden)]


def _cba(x, sd, prefix, stride, eps, slope, act=True):
    w = sd[prefix + ".conv.weight"]
    y = F.conv2d(x, w, None, stride=stride, padding=w.shape[-1] // 2)
    g, b = sd[prefix + ".batch_norm.weight"], sd[prefix + ".batch_norm.bias"]
    mean, var = sd[prefix + ".batch_norm.running_mean"], sd[prefix + ".batch_norm.running_var"]
    scale = g * torch.rsqrt(var + eps)
    shift = _fma(-mean, scale, b)
    y = _fma(y, scale.view(1, -1, 1, 1), shift.view(1, -1, 1, 1))
    return _act(y, slope) if act else y


def _act(y, slope):
    return y if slope is None else F.leaky_relu(y, slope)


def forward(image0, image1, sd_encoder, sd_decoder, n_layer=18, eps=EPS, slope=0.20, skip_projection=False, conv2_act=True,
            final_act=True, pool_pad_zero=False, stage1_stride=1):
    """dict: 'layers' (see `names`), 'map' (N x 6 x h x w), 'dof' (N x 6), 'pose' (N x 4 x 4)."""
    enc, dec = strip(sd_encoder), strip(sd_decoder)
    x = _cba(torch.cat([image0, image1], dim=1), enc, "conv1", 2, eps, slope)
    layers = [x]
    if pool_pad_zero:
        x = F.max_pool2d(F.pad(x, (1, 1, 1, 1), value=0.0), 3, stride=2, padding=0)
    else:
        x = F.max_pool2d(x, 3, stride=2, padding=1)
    layers.append(x)
    for stage, count in enumerate(BLOCKS[n_layer], 2):
        for b in range(count):
            stride = (2 if stage > 2 else stage1_stride) if b == 0 else 1
            prefix = f"blocks{stage}.{b}"
            h = _cba(x, enc, prefix + ".conv1", stride, eps, slope)
            g = _cba(h, enc, prefix + ".conv2", 1, eps, slope, act=conv2_act)
            if tuple(x.shape[1:]) != tuple(g.shape[1:]):
                g = g if skip_projection else g + F.conv2d(x, enc[prefix + ".projection.conv.weight"], None, stride=stride)
            else:
                g = g + x
            x = _act(g, slope) if final_act else g
            layers.append(x)
    hidden = sorted({int(k.split(".")[1]) for k in dec})
    for i in hidden[:-1]:
        x = _cba(x, dec, f"conv.{i}", 2, eps, slope)
        layers.append(x)
    pmap = F.conv2d(x, dec[f"conv.{hidden[-1]}.conv.weight"])
    dof = 0.01 * pmap.mean(dim=(2, 3))
    return {"layers": layers, "map": pmap, "dof": dof, "pose": kb.ops.pose_matrix(dof)}
