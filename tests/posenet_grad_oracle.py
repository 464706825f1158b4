"""CPU restatement of the pose network with BOTH BatchNorm modes, differentiable, in plain torch: the yardstick of the pose
network's backward pass (the role tests/loss_grad_oracle.py has for the loss).  tests/posenet_oracle.py's structure with a
`batch_norm='running' | 'batch'` switch; run it in fp64 under torch.autograd.

    x = cat[image0, image1]
    seven times:  u = conv_{k, stride 2, padding k // 2}(x)
                  running: mean, var = the running statistics (constants)
                  batch:   mean, var = the statistics of u over N, H, W (biased variance), functions of u;
                           running <- 0.9 running + 0.1 (mean, var N H W / (N H W - 1)), num_batches_tracked + 1
                  z = (u - mean) * rsqrt(var + eps) * g + b;   x = z where z > 0, slope z elsewhere (the slope branch AT 0, as
                  torch.nn.functional.leaky_relu differentiates)
    dof = 0.01 * mean_hw(conv_{1 x 1}(x));   pose = ops.pose_matrix(dof)

The keyword arguments of `forward` and of the two hand-written conv gradients are the MISTAKES tests/test_posenet_grad_power_cpu.py
plants to prove that the gate sees them; their defaults are the network.
"""
import torch
import torch.nn.functional as F

import kbnet_amd as kb
import posenet_oracle as po

KERNELS = po.KERNELS
EPS = po.EPS
MOMENTUM = 0.1
FILTERS = [8, 16, 16, 32, 32, 24, 40]     # the narrow network of the goldens (tests/golden/gen_posenet_grad_golden.py)
WG_CHUNK = 32                             # output pixels per K chunk of the weight-gradient kernel

# The gate: |a - b| <= TOL |b| + TOL rms(b) per tensor, against fp64.  TOL = 3 x the worst fraction the oracle's own fp32 autograd
# shows against its fp64 autograd over the cases of the GPU tests, rounded up to one digit (measured and asserted in
# tests/test_posenet_grad_oracle_cpu.py; DESIGN section 8e has the figures); its ceiling is the loss backward's 1e-3.
TOL = 2e-4


def leaky(z, slope, slope_at_zero=False, mask=None):
    """`mask`: the branch of every element (True: the identity) instead of the sign of z -- see `forward`."""
    if slope is None:
        return z
    if mask is None:
        mask = (z >= 0) if slope_at_zero else (z > 0)
    return torch.where(mask, z, slope * z)


def batch_norm_act(u, g, b, mean, var, eps=EPS, slope=0.20, batch=False, detach_stats=False, slope_at_zero=False, mask=None):
    """-> (y, mean, biased var, z): on the batch's own statistics with `batch`, on the given ones without."""
    if batch:
        mean = u.mean(dim=(0, 2, 3))
        var = u.var(dim=(0, 2, 3), unbiased=False)
        if detach_stats:
            mean, var = mean.detach(), var.detach()
    scale = g * torch.rsqrt(var + eps)
    z = u * scale.view(1, -1, 1, 1) + (b - mean * scale).view(1, -1, 1, 1)
    return leaky(z, slope, slope_at_zero, mask), mean, var, z


def forward(image0, image1, sd_encoder, sd_decoder, batch_norm="running", eps=EPS, slope=0.20, factor=0.01, detach_stats=False,
            biased_running_var=False, slope_at_zero=False, masks=None):
    """dict: 'layers', 'pre' (the seven pre-activations z), 'dof', 'pose', and 'running': the running statistics after this
    forward (batch mode: updated).  `masks`: seven boolean tensors, the activation branch of every element (True: z > 0) as the
    run under test took it.  A pre-activation that fp32 and fp64 put on opposite sides of 0 changes that element's gradient by
    the factor `slope`, which is no error of either: with `masks` the fp64 network is differentiated on the branches of the
    run it is compared with (see `kink_check` for what a caller must assert about the elements that differ)."""
    assert batch_norm in ("running", "batch")
    sd_encoder, sd_decoder = po.strip(sd_encoder), po.strip(sd_decoder)
    x = torch.cat([image0, image1], dim=1)
    layers, running, pres = [], {}, []
    for i, k in enumerate(KERNELS, 1):
        pre = f"conv{i}.batch_norm."
        u = F.conv2d(x, sd_encoder[f"conv{i}.conv.weight"], None, stride=2, padding=k // 2)
        x, mean, var, z = batch_norm_act(u, sd_encoder[pre + "weight"], sd_encoder[pre + "bias"], sd_encoder[pre + "running_mean"],
                                         sd_encoder[pre + "running_var"], eps, slope, batch_norm == "batch", detach_stats, slope_at_zero,
                                         None if masks is None else masks[i - 1])
        pres.append(z.detach())
        if batch_norm == "batch":
            count = u.shape[0] * u.shape[2] * u.shape[3]
            assert count > 1
            unbias = 1.0 if biased_running_var else count / (count - 1.0)
            running[pre + "running_mean"] = ((1 - MOMENTUM) * sd_encoder[pre + "running_mean"] + MOMENTUM * mean).detach()
            running[pre + "running_var"] = ((1 - MOMENTUM) * sd_encoder[pre + "running_var"] + MOMENTUM * unbias * var).detach()
            running[pre + "num_batches_tracked"] = sd_encoder[pre + "num_batches_tracked"] + 1
        else:
            for key in ("running_mean", "running_var", "num_batches_tracked"):
                running[pre + key] = sd_encoder[pre + key]
        layers.append(x)
    pmap = F.conv2d(x, sd_decoder["conv.conv.weight"])
    dof = factor * pmap.mean(dim=(2, 3))
    return {"layers": layers, "pre": pres, "map": pmap, "dof": dof, "pose": kb.ops.pose_matrix(dof), "running": running}


KINK_BAND = 1e-4     # of rms(z): ten times the fp32 forward's own error (layers agree with fp64 to about 1e-5 of |b| + rms(b))
KINK_SHARE = 1e-5    # of a layer's elements: a handful in the largest map of the tests


def kink_check(masks, pres):
    """What must hold before `masks` may replace the signs of the fp64 pre-activations `pres`: the elements whose branch differs
    are few (at most one, or KINK_SHARE of the layer) and every one of them lies within KINK_BAND rms(z) of 0 in fp64 -- they
    sit AT the kink.  A kernel with a wrong mask fails here.  -> the number of such elements."""
    total = 0
    for i, (m, z) in enumerate(zip(masks, pres), 1):
        differ = m.cpu() != (z > 0)
        count = int(differ.sum())
        assert count <= max(1, int(KINK_SHARE * z.numel())), (i, count, z.numel())
        if count:
            assert float(z[differ].abs().max()) < KINK_BAND * po.rms(z), (i, float(z[differ].abs().max()), po.rms(z))
        total += count
    return total


KINK_NEAR = 5e-6     # of rms(z): where an fp32 run may land on the other side of 0 (half the forward's own 1e-5 error)


def kink_room(pres):
    """The property a model case's seed is picked for: no activation has more fp64 pre-activations within KINK_NEAR rms(z) of 0
    than kink_check lets flip, so an fp32 run's few branch flips cannot exceed kink_check's share by bad luck.  -> the largest count."""
    worst = 0
    for i, z in enumerate(pres, 1):
        count = int((z.double().abs() < KINK_NEAR * po.rms(z)).sum())
        assert count <= max(1, int(KINK_SHARE * z.numel())), (i, count, z.numel())
        worst = max(worst, count)
    return worst


def trainable(key):
    return key.endswith("conv.weight") or key.endswith("batch_norm.weight") or key.endswith("batch_norm.bias")


def gradients(image0, image1, sd_encoder, sd_decoder, cotangent, dtype=torch.float64, **kw):
    """Gradients of L = sum(pose * cotangent) by torch.autograd in `dtype` -> dict: 'enc::<key>' / 'dec::<key>' for every
    trainable parameter, 'dof', 'pose', and 'run::<key>' for the running statistics after the forward."""
    def cast(sd, leaf):
        out = {}
        for k, v in po.strip(sd).items():
            v = v.detach().to(dtype) if v.is_floating_point() else v.detach().clone()
            out[k] = v.requires_grad_(True) if leaf and trainable(k) else v
        return out
    enc, dec = cast(sd_encoder, True), cast(sd_decoder, True)
    out = forward(image0.to(dtype), image1.to(dtype), enc, dec, **kw)
    (out["pose"] * cotangent.to(dtype)).sum().backward()
    res = {"dof": out["dof"].detach(), "pose": out["pose"].detach(), "pre": out["pre"]}
    for grp, sd in (("enc", enc), ("dec", dec)):
        for k, v in sd.items():
            if trainable(k):
                res[f"{grp}::{k}"] = v.grad
    for k, v in out["running"].items():
        res["run::" + k] = v
    return res


def pose_gradients(image0, image1, sd_encoder, sd_decoder, grad_pose, **kw):
    """`gradients` for a given d loss / d pose (N x 4 x 4): the chain behind a loss's own backward."""
    return gradients(image0, image1, sd_encoder, sd_decoder, grad_pose, **kw)


# ---- the two conv gradients written out (what the kernels of csrc/posenet_backward.hip compute), with their planted mistakes ----
def conv_backward_data(g, weight, height, width, pad=None, swap_parity=False):
    """d conv_{k, stride 2, padding k // 2} / d input in gather form: input pixel (iy, ix) takes tap (ky, kx) of output pixel
    ((iy + pad - ky) / 2, (ix + pad - kx) / 2) where both are whole and inside the map.  `swap_parity`: the parity test of the rows
    run on the column tap and the other way round."""
    oc, cin, k, _ = weight.shape
    pad = k // 2 if pad is None else pad
    n, _, oh, ow = g.shape
    dx = torch.zeros(n, cin, height, width, dtype=g.dtype)
    iy, ix = torch.arange(height), torch.arange(width)
    for ky in range(k):
        for kx in range(k):
            ty, tx = iy + pad - (kx if swap_parity else ky), ix + pad - (ky if swap_parity else kx)
            ok_y = (ty >= 0) & (ty % 2 == 0) & (ty // 2 < oh)
            ok_x = (tx >= 0) & (tx % 2 == 0) & (tx // 2 < ow)
            if not ok_y.any() or not ok_x.any():
                continue
            oy, ox = (iy[ok_y] + pad - ky), (ix[ok_x] + pad - kx)
            oy, ox = torch.div(oy, 2, rounding_mode="floor").clamp(0, oh - 1), torch.div(ox, 2, rounding_mode="floor").clamp(0, ow - 1)
            contrib = torch.einsum("nohw,oc->nchw", g[:, :, oy][:, :, :, ox], weight[:, :, ky, kx])
            dx[:, :, iy[ok_y][:, None], ix[ok_x][None, :]] += contrib
    return dx


def conv_backward_weight(x, g, k, drop_last_chunk=False):
    """d conv / d weight (OIHW).  `drop_last_chunk`: without the last PARTIAL chunk of WG_CHUNK output pixels of the batch, in
    (frame, oy, ox) order -- a K loop that stops at the last whole chunk."""
    n, oc, oh, ow = g.shape
    if drop_last_chunk:
        m = n * oh * ow
        keep = (m // WG_CHUNK) * WG_CHUNK
        flat = g.permute(1, 0, 2, 3).reshape(oc, m).clone()
        flat[:, keep:] = 0
        g = flat.reshape(oc, n, oh, ow).permute(1, 0, 2, 3)
    return torch.nn.grad.conv2d_weight(x, (oc, x.shape[1], k, k), g.contiguous(), stride=2, padding=k // 2)


# ---- the gate ----
def fraction(a, b):
    """max over the elements of |a - b| / (|b| + rms(b)): <= TOL passes."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    if b.numel() == 0:
        return 0.0
    return float(((a - b).abs() / (b.abs() + po.rms(b))).max())


def passes(a, b, tol=None):
    return fraction(a, b) <= (TOL if tol is None else tol)
