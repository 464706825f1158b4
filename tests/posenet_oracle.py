"""CPU restatement of the pose network's eval-mode forward in plain torch, for the tests (the role tests/loss_oracle.py has for the
loss): reference src/posenet_model.py:95-112, src/networks.py:536-671 and 1992-2075, src/net_utils.py:120-141.

    x = cat[image0, image1]                                         6 channels
    seven times:  x = leaky_relu(conv_{k, stride 2, padding k // 2}(x) * scale + shift, 0.20)      k = 7, 5, 3, 3, 3, 3, 3
                  scale = g * rsqrt(var + eps),  shift = b - mean * scale      (BatchNorm2d.eval(), eps = 1e-5)
                  In fp32 the two multiply-adds (the shift, and x * scale + shift) round ONCE each, as torch's CPU BatchNorm2d
                  does in eval mode (fused multiply-adds): with that the fp32 form equals the reference bit for bit.
    map = conv_{1 x 1}(x)   6 channels;   dof = 0.01 * mean_hw(map);   pose = ops.pose_matrix(dof)

Runs in the dtype of its inputs: hand it fp32 tensors for the fp32 form, `.double()` ones (see `to64`) for the fp64 form.  The
keyword arguments are the MISTAKES tests/test_posenet_cpu.py plants to prove the gates can see them; their defaults are the
network.
"""
import torch
import torch.nn.functional as F

import kbnet_amd as kb

KERNELS = (7, 5, 3, 3, 3, 3, 3)
EPS = 1e-5


def strip(sd):
    return {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}


def to64(*items):
    """Tensors and state dicts cast to fp64 (integer entries left alone)."""
    def one(x):
        if isinstance(x, dict):
            return {k: (v.double() if v.is_floating_point() else v) for k, v in x.items()}
        return x.double()
    return tuple(one(x) for x in items)


def affine(sd, i, eps=EPS):
    g, b = sd[f"conv{i}.batch_norm.weight"], sd[f"conv{i}.batch_norm.bias"]
    mean, var = sd[f"conv{i}.batch_norm.running_mean"], sd[f"conv{i}.batch_norm.running_var"]
    scale = g * torch.rsqrt(var + eps)
    return scale, _fma(-mean, scale, b)


def _fma(a, b, c):
    """a * b + c with ONE rounding in fp32 (through fp64: the product of two fp32 values is exact there); plain in fp64."""
    if a.dtype == torch.float32:
        return (a.double() * b.double() + c.double()).float()
    return a * b + c


def forward(image0, image1, sd_encoder, sd_decoder, eps=EPS, slope=0.20, pad1=None, factor=0.01):
    """dict: 'layers' (the seven activations), 'map' (N x 6 x h x w), 'dof' (N x 6), 'pose' (N x 4 x 4)."""
    sd_encoder, sd_decoder = strip(sd_encoder), strip(sd_decoder)
    x = torch.cat([image0, image1], dim=1)
    layers = []
    for i, k in enumerate(KERNELS, 1):
        pad = k // 2 if (i > 1 or pad1 is None) else pad1
        y = F.conv2d(x, sd_encoder[f"conv{i}.conv.weight"], None, stride=2, padding=pad)
        scale, shift = affine(sd_encoder, i, eps)
        y = _fma(y, scale.view(1, -1, 1, 1), shift.view(1, -1, 1, 1))
        x = F.leaky_relu(y, slope)
        layers.append(x)
    pmap = F.conv2d(x, sd_decoder["conv.conv.weight"])
    dof = factor * pmap.mean(dim=(2, 3))
    return {"layers": layers, "map": pmap, "dof": dof, "pose": kb.ops.pose_matrix(dof)}


# ---- the gate (tests/test_hip_parity.py, test_intermediate_tensors_elementwise_full_size): |a - b| <= 1e-4 |b| + floor ----
def rms(t):
    return float(t.double().pow(2).mean().sqrt())


def gate_fraction(a, b, floor):
    """max over the elements of |a - b| / (1e-4 |b| + floor): <= 1 passes."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(((a - b).abs() / (1e-4 * b.abs() + floor)).max())


def layer_floor(b):
    return 1e-4 * rms(b)


def dof_floor(pmap):
    """dof (and the translation column) average the 6-channel map and scale it by 0.01: the floor follows that tensor."""
    return 1e-4 * 0.01 * rms(pmap)
