"""CPU restatement of the ResNet-18/34 pose network with BOTH BatchNorm modes, differentiable, in plain torch: the yardstick of
ResNetPoseNetModel(trainable=True)'s backward pass (the role tests/posenet_grad_oracle.py has for the seven-conv network).
tests/resnet_pose_oracle.py's structure with a `batch_norm='running' | 'batch'` switch; run it in fp64 under torch.autograd.

    cba(x, k, s) = act(batch_norm(conv_{k, stride s, padding k // 2}(x)))      running or batch statistics, as posenet_grad_oracle
    conv1 = cba(cat[image0, image1], 7, 2);   pool = max_pool(conv1, 3, stride 2, padding 1), a window's gradient to its FIRST maximum
    every block:  h = cba(x, 3, s);  a = cba(h, 3, 1);  X = x, or conv_{1 x 1, stride s}(x) when shape or channels differ
                  y = act(a + X)           (the activation twice on the main path, reference src/net_utils.py:643-667)
    decoder: cba(x, 3, 2) per hidden layer, dof = 0.01 * mean_hw(conv_{1 x 1}(x)), pose = ops.pose_matrix(dof)

`masks` (name -> bool tensor) and `pool_indices` replace the branch of every activation and the argmax of every pool window by the
ones the run under test took; `kink_check` is what a caller must assert before it may do so.  The other keyword arguments of
`forward` are the MISTAKES tests/test_resnet_pose_grad_power_cpu.py plants; their defaults are the network.
"""
import torch
import torch.nn.functional as F

import kbnet_amd as kb
import posenet_grad_oracle as pgo
import posenet_oracle as po
from resnet_pose_oracle import BLOCKS

EPS = po.EPS
MOMENTUM = pgo.MOMENTUM
FILTERS = [8, 12, 16, 16, 32]        # the narrow network of the goldens: 8 -> 12 at stride 1 puts the 1 x 1 stride-1 projection in blocks2.0
DECODER_FILTERS = [16, 16]

# The gate: |a - b| <= TOL |b| + TOL rms(b) per tensor, against fp64.  TOL = 3 x the worst fraction the oracle's own fp32 autograd
# shows against its fp64 autograd (same masks, same pool indices) over the model cases of the GPU tests, rounded up to one digit
# (measured and asserted in tests/test_resnet_pose_grad_oracle_cpu.py; DESIGN section 8f has the figures); ceiling 1e-3.
TOL = 8e-4

KINK_BAND = pgo.KINK_BAND
KINK_SHARE = pgo.KINK_SHARE
fraction = pgo.fraction


def passes(a, b, tol=None):
    return fraction(a, b) <= (TOL if tol is None else tol)


def activation_names(n_layer=18, n_hidden=2):
    """Every activation of the network, in forward order: the keys of `masks` and of the 'pre' a forward returns."""
    out = ["conv1"]
    for stage, count in enumerate(BLOCKS[n_layer], 2):
        for b in range(count):
            out += [f"blocks{stage}.{b}.conv1", f"blocks{stage}.{b}.conv2", f"blocks{stage}.{b}"]
    return out + [f"decoder{i}" for i in range(n_hidden)]


def pool_argmax(x, last=False):
    """Flat index (iy * W + ix) of the maximum of every 3 x 3 stride-2 padding-1 window of x: the FIRST in row-major order (what
    torch.nn.functional.max_pool2d returns and routes the gradient to), or with `last` the last one."""
    n, c, h, w = x.shape
    oh, ow = (h + 1) // 2, (w + 1) // 2
    cols = F.unfold(F.pad(x, (1, 1, 1, 1), value=float("-inf")), 3, stride=2).reshape(n, c, 9, oh * ow)
    tap = 8 - cols.flip(2).argmax(dim=2) if last else cols.argmax(dim=2)
    oy = torch.arange(oh).repeat_interleave(ow).view(1, 1, -1)
    ox = torch.arange(ow).repeat(oh).view(1, 1, -1)
    iy, ix = 2 * oy - 1 + tap // 3, 2 * ox - 1 + tap % 3
    return (iy * w + ix).reshape(n, c, oh, ow)


def pool(x, indices):
    """The pool as a gather at `indices` (pool_argmax's form): autograd then routes every window's gradient there."""
    return x.flatten(2).gather(2, indices.flatten(2)).reshape(indices.shape)


def forward(image0, image1, sd_encoder, sd_decoder, n_layer=18, batch_norm="running", eps=EPS, slope=0.20, masks=None, pool_indices=None,
            drop_skip_grad=False, drop_projection_grad=False, conv2_act_in_backward=True, pool_last_max=False, detach_stats=False,
            biased_running_var=False):
    """dict: 'layers' (resnet_pose_oracle.names order), 'pre' (name -> the pre-activation z, detached, `activation_names` order),
    'pool_in' (the pool's input, detached), 'pool_indices' (the argmax it used), 'map', 'dof', 'pose', 'running' (the running
    statistics after this forward: updated in batch mode)."""
    assert batch_norm in ("running", "batch")
    enc, dec = po.strip(sd_encoder), po.strip(sd_decoder)
    batch = batch_norm == "batch"
    pres, running = {}, {}

    def act(z, name, in_backward=True):
        pres[name] = z.detach()
        y = pgo.leaky(z, slope, mask=None if masks is None else masks[name])
        return y if in_backward else z + (y - z).detach()

    def bn(u, sd, grp, prefix):
        pre = prefix + ".batch_norm."
        _, mean, var, z = pgo.batch_norm_act(u, sd[pre + "weight"], sd[pre + "bias"], sd[pre + "running_mean"], sd[pre + "running_var"],
                                             eps, None, batch, detach_stats)
        if batch:
            count = u.shape[0] * u.shape[2] * u.shape[3]
            assert count > 1
            unbias = 1.0 if biased_running_var else count / (count - 1.0)
            running[grp + pre + "running_mean"] = ((1 - MOMENTUM) * sd[pre + "running_mean"] + MOMENTUM * mean).detach()
            running[grp + pre + "running_var"] = ((1 - MOMENTUM) * sd[pre + "running_var"] + MOMENTUM * unbias * var).detach()
            running[grp + pre + "num_batches_tracked"] = sd[pre + "num_batches_tracked"] + 1
        else:
            for key in ("running_mean", "running_var", "num_batches_tracked"):
                running[grp + pre + key] = sd[pre + key]
        return z

    def cba(x, sd, grp, prefix, stride, name, in_backward=True):
        w = sd[prefix + ".conv.weight"]
        return act(bn(F.conv2d(x, w, None, stride=stride, padding=w.shape[-1] // 2), sd, grp, prefix), name, in_backward)

    x = cba(torch.cat([image0, image1], dim=1), enc, "enc::", "conv1", 2, "conv1")
    layers = [x]
    pool_in = x.detach()
    if pool_indices is None:
        pool_indices = pool_argmax(pool_in, last=pool_last_max)
    x = pool(x, pool_indices)
    layers.append(x)
    for stage, count in enumerate(BLOCKS[n_layer], 2):
        for b in range(count):
            stride = 2 if (stage > 2 and b == 0) else 1
            prefix = f"blocks{stage}.{b}"
            h = cba(x, enc, "enc::", prefix + ".conv1", stride, prefix + ".conv1")
            a = cba(h, enc, "enc::", prefix + ".conv2", 1, prefix + ".conv2", conv2_act_in_backward)
            if tuple(x.shape[1:]) != tuple(a.shape[1:]):
                wp = enc[prefix + ".projection.conv.weight"]
                skip = F.conv2d(x, wp.detach(), None, stride=stride) + 0.0 * wp.sum() if drop_projection_grad else \
                    F.conv2d(x, wp, None, stride=stride)
            else:
                skip = x
            x = act(a + (skip.detach() if drop_skip_grad else skip), prefix)
            layers.append(x)
    hidden = sorted({int(k.split(".")[1]) for k in dec})
    for i in hidden[:-1]:
        x = cba(x, dec, "dec::", f"conv.{i}", 2, f"decoder{i}")
        layers.append(x)
    pmap = F.conv2d(x, dec[f"conv.{hidden[-1]}.conv.weight"])
    dof = 0.01 * pmap.mean(dim=(2, 3))
    return {"layers": layers, "pre": pres, "pool_in": pool_in, "pool_indices": pool_indices, "map": pmap, "dof": dof,
            "pose": kb.ops.pose_matrix(dof), "running": running}


def kink_check(masks, pres, pool_indices=None, pool_in=None):
    """What must hold before `masks` / `pool_indices` may replace the fp64 network's own branches: per activation the elements
    whose branch differs from the sign of the fp64 pre-activation are at most max(1, KINK_SHARE numel) and lie within KINK_BAND
    rms(z) of 0; the pool windows whose index differs from the fp64 first maximum are as few, and the two candidates' fp64 values
    differ by less than KINK_BAND rms of the map.  A kernel with a wrong mask or a wrong routing fails here.  -> the count."""
    total = 0
    assert set(masks) == set(pres), sorted(set(masks) ^ set(pres))
    for name, z in pres.items():
        differ = masks[name].cpu() != (z > 0)
        count = int(differ.sum())
        assert count <= max(1, int(KINK_SHARE * z.numel())), (name, count, z.numel())
        if count:
            assert float(z[differ].abs().max()) < KINK_BAND * po.rms(z), (name, float(z[differ].abs().max()), po.rms(z))
        total += count
    if pool_indices is not None:
        own = pool_argmax(pool_in)
        differ = own != pool_indices.cpu()
        count = int(differ.sum())
        assert count <= max(1, int(KINK_SHARE * own.numel())), ("pool", count, own.numel())
        if count:
            gap = (pool(pool_in, own) - pool(pool_in, pool_indices.cpu())).abs()[differ].max()
            assert float(gap) < KINK_BAND * po.rms(pool_in), ("pool", float(gap), po.rms(pool_in))
        total += count
    return total


def trainable(key):
    return pgo.trainable(key)


def gradients(image0, image1, sd_encoder, sd_decoder, cotangent, dtype=torch.float64, **kw):
    """Gradients of L = sum(pose * cotangent) by torch.autograd in `dtype` -> dict: 'enc::<key>' / 'dec::<key>' for every trainable
    parameter the forward used (the projection of a block with the identity skip is ABSENT: its .grad is None), 'dof', 'pose',
    'pre', 'pool_in', 'pool_indices', and 'run::<enc|dec>::<key>' for the running statistics after the forward."""
    def cast(sd):
        out = {}
        for k, v in po.strip(sd).items():
            v = v.detach().to(dtype) if v.is_floating_point() else v.detach().clone()
            out[k] = v.requires_grad_(True) if trainable(k) else v
        return out
    enc, dec = cast(sd_encoder), cast(sd_decoder)
    out = forward(image0.to(dtype), image1.to(dtype), enc, dec, **kw)
    (out["pose"] * cotangent.to(dtype)).sum().backward()
    res = {"dof": out["dof"].detach(), "pose": out["pose"].detach(), "pre": out["pre"], "pool_in": out["pool_in"],
           "pool_indices": out["pool_indices"]}
    for grp, sd in (("enc", enc), ("dec", dec)):
        for k, v in sd.items():
            if trainable(k) and v.grad is not None:
                res[f"{grp}::{k}"] = v.grad
    for k, v in out["running"].items():
        res["run::" + k] = v
    return res


def gradient_keys(res):
    return [k for k in res if k.startswith(("enc::", "dec::"))]
