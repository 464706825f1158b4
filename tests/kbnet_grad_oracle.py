"""CPU restatement of the depth network, differentiable, in plain torch and in any dtype: the yardstick of KBNetModel's backward pass
(the role tests/resnet_pose_grad_oracle.py has for the pose networks).  oracle/kbnet_oracle.py's structure with the pixel grid and the
scaled intrinsics in the dtype of the run (that file builds them in fp32), a way to impose the activations' branches, and the
pre-activation of every layer kept; run it in fp64 under torch.autograd.  In fp32 its forward is oracle/kbnet_oracle.kbnet_forward bit
for bit (tests/test_kbnet_grad_oracle_cpu.py).

    d      = S2D(cat[sparse_depth, validity])             pyramid (data) -> 1 x 1 convs -> conv3x3(cat[., x])
    level  : KB   conv_image = conv3x3 s2 (image); conv_depth = conv3x3 s2 (cat[depth, coordinates]); z = act(proj_depth(depth));
                  conv_fused = conv1x1 s2 (cat[image, coordinates * z, fused]); skip = cat[conv_fused, conv_depth]
             plain conv_image = conv3x3 s2 (conv_fused or conv_image); conv_depth = conv3x3 s2 (conv_depth)
             level 4 listed: block 4 a second time (the reference's quirk), block 5 unused
    decoder: five times conv3x3(cat[conv3x3(nearest(x)), skip]); logits = conv3x3 (linear)
    depth  = d_min / (sigmoid(logits) + d_min / d_max)

`masks` (name -> bool tensor, kbnet_train.activation_names) replaces the sign test of every activation: the fp64 network is then
differentiated on the branches of the run it is compared with (posenet_grad_oracle.kink_check says what a caller must assert first).
The keyword switches of `forward` are the MISTAKES tests/test_kbnet_grad_power_cpu.py plants; their defaults are the network.
"""
import torch
import torch.nn.functional as F

import kbnet_amd as kb
import posenet_grad_oracle as pgo
from oracle import kbnet_oracle as orc

fraction, kink_check, kink_room, KINK_BAND, KINK_SHARE = pgo.fraction, pgo.kink_check, pgo.kink_room, pgo.KINK_BAND, pgo.KINK_SHARE
activation_names = kb.kbnet_train.activation_names      # the names are fixed in one place

# The gate: |a - b| <= TOL |b| + TOL rms(b) per tensor, against fp64.  TOL = 3 x the worst fraction the oracle's own fp32 autograd
# shows against its fp64 autograd over the cases of tests/kbnet_grad_cases.py, on the fp32 run's branches, rounded up to one digit
# (measured and asserted in tests/test_kbnet_grad_oracle_cpu.py; DESIGN section 8g has the figures); its ceiling is 1e-3.
TOL = 7e-5
# kbn_depth_map_backward alone: 3 x what torch's fp32 autograd of the same expression shows against fp64 on the operator test's
# inputs (logits in [-8, 8] and +-30, both depth ranges), measured and asserted in the same file.
DEPTH_MAP_TOL = 7e-7

MISTAKES = ("drop_skip_depth", "drop_fused_xyz", "xyz_without_act_grad", "resize_one_pixel", "resize_half_map",
            "depth_map_without_sigmoid_grad", "fused_slice_offset", "second_use_not_accumulated")


def act(pre, slope, mask=None):
    if slope is None:
        return pre
    if mask is None:
        mask = pre > 0
    return torch.where(mask, pre, slope * pre)


def nearest_map(size_in, size_out):
    """torch's own nearest index rule, read off F.interpolate instead of restated: -> size_out source indices."""
    src = torch.arange(size_in, dtype=torch.float64).view(1, 1, size_in, 1)
    return F.interpolate(src, size=(size_out, 1), mode="nearest").view(-1).long()


class _Resize(torch.autograd.Function):
    """F.interpolate(mode='nearest') with its backward written out as the scatter over the index map, so that a wrong map or a
    backward that takes one destination pixel per source pixel can be planted.  The forward is always torch's."""

    @staticmethod
    def forward(ctx, x, height, width, one_pixel, half_map):
        h, w = x.shape[2:]
        iy, ix = nearest_map(h, height), nearest_map(w, width)
        ctx.args = (h, w, iy, ix, one_pixel, half_map)
        return x[:, :, iy][:, :, :, ix]

    @staticmethod
    def backward(ctx, g):
        h, w, iy, ix, one_pixel, half_map = ctx.args
        if half_map:
            iy = (torch.arange(g.shape[2]) // 2).clamp(max=h - 1)
            ix = (torch.arange(g.shape[3]) // 2).clamp(max=w - 1)
        if one_pixel:      # the first destination pixel of every source pixel, not their sum
            fy = torch.tensor([int((iy == s).nonzero()[0]) for s in range(h)])
            fx = torch.tensor([int((ix == s).nonzero()[0]) for s in range(w)])
            return g[:, :, fy][:, :, :, fx], None, None, None, None
        rows = torch.zeros(g.shape[:2] + (h, g.shape[3]), dtype=g.dtype).index_add_(2, iy, g)
        return torch.zeros(g.shape[:2] + (h, w), dtype=g.dtype).index_add_(3, ix, rows), None, None, None, None


class _GradientTo(torch.autograd.Function):
    """`value` in the forward, bit for bit; in the backward the gradient goes to `through` as it is: a factor of the chain rule left out."""

    @staticmethod
    def forward(ctx, value, through):
        return value.detach().clone()

    @staticmethod
    def backward(ctx, g):
        return None, g


class _CatFused(torch.autograd.Function):
    """cat[image, xyz, fused] whose backward hands `fused` the slice that starts at xyz's offset: the three xyz channels forgotten."""

    @staticmethod
    def forward(ctx, image, xyz, fused):
        ctx.sizes = (image.shape[1], xyz.shape[1], fused.shape[1])
        return torch.cat([image, xyz, fused], dim=1)

    @staticmethod
    def backward(ctx, g):
        ci, cx, cf = ctx.sizes
        return g[:, :ci], g[:, ci:ci + cx], g[:, ci:ci + cf]


def pixel_grid(n, height, width, dtype):
    xs = torch.linspace(start=0.0, end=width - 1, steps=width, dtype=dtype)
    ys = torch.linspace(start=0.0, end=height - 1, steps=height, dtype=dtype)
    gy, gx = torch.meshgrid(ys, xs, indexing="ij")
    return torch.stack([gx, gy, torch.ones_like(gx)], dim=0).unsqueeze(0).repeat(n, 1, 1, 1)


def camera_coordinates(k, height, width):
    n = k.shape[0]
    return torch.matmul(torch.inverse(k), pixel_grid(n, height, width, k.dtype).view(n, 3, -1)).view(n, 3, height, width)


def scale_intrinsics(k, height0, width0, height1, width1):
    """The two ratios are fp32 numbers in every dtype of the run: the reference builds this matrix with dtype=torch.float32
    (src/networks.py:346-348) and the device path hands them to kbn_intrinsics_inverse as floats."""
    sx, sy = width1 / width0, height1 / height0
    return k * torch.tensor([[sx, 1.0, sx], [1.0, sy, sy], [1.0, 1.0, 1.0]], dtype=torch.float32).to(k.dtype).view(1, 3, 3)


def forward(image, sparse_depth, validity_map_depth, intrinsics, sd_s2d, sd_encoder, sd_decoder, cfg, masks=None,
            drop_skip_depth=False, drop_fused_xyz=False, xyz_without_act_grad=False, resize_one_pixel=False, resize_half_map=False,
            depth_map_without_sigmoid_grad=False, fused_slice_offset=False, second_use_not_accumulated=False):
    """-> dict: 'depth', 'logits', 'pre' (name -> the detached pre-activation of every activation, in forward order)."""
    s2d, enc, dec = orc.strip_prefix(sd_s2d), orc.strip_prefix(sd_encoder), orc.strip_prefix(sd_decoder)
    slope = orc.activation_slope(cfg.activation_func)
    assert slope is None or isinstance(slope, float), slope
    listed = tuple(cfg.resolutions_backprojection)
    pre = {}

    def conv(x, weight, stride, name):
        u = F.conv2d(x, weight, None, stride=stride, padding=weight.shape[-1] // 2)
        if name is None:
            return u
        pre[name] = u.detach()
        return act(u, slope, None if masks is None else masks[name])

    x = torch.cat([sparse_depth, validity_map_depth], dim=1)
    h = orc.s2d_pool_pyramid(x[:, 0:1], cfg.min_pools, cfg.max_pools)
    for i in range(cfg.n_convolution_sparse_to_dense_pool):
        h = conv(h, s2d[f"pool_convs.{i}.conv.weight"], 1, f"s2d.pool_convs.{i}")
    d = conv(torch.cat([h, x], dim=1), s2d["conv.conv.weight"], 1, "s2d.conv")

    n, _, h0, w0 = image.shape
    conv_image = conv(image, enc["conv0_image.conv.weight"], 1, "conv0_image")
    conv_depth = conv(d, enc["conv0_depth.conv.weight"], 1, "conv0_depth")
    conv_fused = None
    h1, w1 = (h0 + 1) // 2, (w0 + 1) // 2
    skips = []
    for level in range(5):
        hl, wl = conv_image.shape[-2:]
        name = f"level{level}"
        if level in listed:
            k_l = intrinsics if level == 0 else scale_intrinsics(intrinsics, h0, w0, h1, w1)     # Q1: always the level-1 ratio
            coords = camera_coordinates(k_l, hl, wl)
            p = f"calibrated_backprojection{min(level, 3) + 1}."                                  # Q3: level 4 is block 4 again
            weights = {k: enc[p + k] for k in ("conv_image.conv_block.0.conv.weight", "conv_depth.conv_block.0.conv.weight",
                                               "proj_depth.conv.weight", "conv_fused.conv.weight")}
            if level == 4 and second_use_not_accumulated:
                weights = {k: v.detach() for k, v in weights.items()}
            image_in, depth_in, fused_in = conv_image, conv_depth, conv_fused
            conv_image = conv(image_in, weights["conv_image.conv_block.0.conv.weight"], 2, name + ".conv_image")
            conv_depth = conv(torch.cat([depth_in, coords], dim=1), weights["conv_depth.conv_block.0.conv.weight"], 2, name + ".conv_depth")
            u = F.conv2d(depth_in, weights["proj_depth.conv.weight"])
            pre[name + ".proj_depth"] = u.detach()
            z = act(u, slope, None if masks is None else masks[name + ".proj_depth"])
            if xyz_without_act_grad:
                z = _GradientTo.apply(z, u)
            xyz = coords * z
            if drop_fused_xyz:
                xyz = xyz.detach()
            if fused_in is None:
                cat = torch.cat([image_in, xyz], dim=1)
            elif fused_slice_offset:
                cat = _CatFused.apply(image_in, xyz, fused_in)
            else:
                cat = torch.cat([image_in, xyz, fused_in], dim=1)
            conv_fused = conv(cat, weights["conv_fused.conv.weight"], 2, name + ".conv_fused")
            out = [conv_fused, conv_depth.detach() if drop_skip_depth and level < 4 else conv_depth]
        else:
            src = conv_fused if conv_fused is not None else conv_image
            conv_image = conv(src, enc[f"conv{level + 1}_image.conv_block.0.conv.weight"], 2, name + ".conv_image")
            conv_depth = conv(conv_depth, enc[f"conv{level + 1}_depth.conv_block.0.conv.weight"], 2, name + ".conv_depth")
            conv_fused = None
            out = [conv_image, conv_depth]
        skips.append(torch.cat(out, dim=1))
    y = skips.pop()
    for i in (4, 3, 2, 1, 0):
        shape = skips[i - 1].shape[2:4] if i else (h0, w0)
        up = _Resize.apply(y, int(shape[0]), int(shape[1]), resize_one_pixel, resize_half_map)
        y = conv(up, dec[f"deconv{i}.deconv.conv.conv.weight"], 1, f"deconv{i}.deconv")
        if i:
            y = torch.cat([y, skips[i - 1]], dim=1)
        y = conv(y, dec[f"deconv{i}.conv.conv.weight"], 1, f"deconv{i}.conv")
    logits = conv(y, dec["output0.conv.weight"], 1, None)
    s = torch.sigmoid(logits)
    if depth_map_without_sigmoid_grad:
        s = _GradientTo.apply(s, logits)
    depth = cfg.min_predict_depth / (s + cfg.min_predict_depth / cfg.max_predict_depth)
    assert list(pre) == activation_names(listed, cfg.n_convolution_sparse_to_dense_pool)
    return {"depth": depth, "logits": logits.detach(), "pre": pre}


GROUPS = ("s2d", "enc", "dec")


def gradients(image, sparse_depth, validity_map_depth, intrinsics, sd_s2d, sd_encoder, sd_decoder, cotangent, cfg, dtype=torch.float64,
              **kw):
    """Gradients of L = sum(depth * cotangent) by torch.autograd in `dtype` -> dict: 's2d::<key>' / 'enc::<key>' / 'dec::<key>' for
    every parameter the forward used (one it never touches is ABSENT, as its .grad stays None), 'depth', 'logits', 'pre'."""
    sds = [{k: v.detach().to(dtype).requires_grad_(True) for k, v in orc.strip_prefix(sd).items()} for sd in (sd_s2d, sd_encoder, sd_decoder)]
    out = forward(image.to(dtype), sparse_depth.to(dtype), validity_map_depth.to(dtype), intrinsics.to(dtype), *sds, cfg, **kw)
    (out["depth"] * cotangent.to(dtype)).sum().backward()
    res = {"depth": out["depth"].detach(), "logits": out["logits"], "pre": out["pre"]}
    for grp, sd in zip(GROUPS, sds):
        for k, v in sd.items():
            if v.grad is not None:
                res[f"{grp}::{k}"] = v.grad
    return res


def gradient_keys(res):
    return [k for k in res if k.startswith(tuple(g + "::" for g in GROUPS))]


def parameter_keys(sd_s2d, sd_encoder, sd_decoder):
    return [f"{grp}::{k}" for grp, sd in zip(GROUPS, (sd_s2d, sd_encoder, sd_decoder)) for k in orc.strip_prefix(sd)]


def masks_of(pre_or_inner):
    """name -> bool (True: the identity branch) from pre-activations or from the activations a device run returned."""
    return {k: (v > 0).cpu() for k, v in pre_or_inner.items()}


def check_kinks(masks, pre):
    """posenet_grad_oracle.kink_check over the named activations -> the number of elements on the other side of the kink."""
    names = list(pre)
    assert sorted(masks) == sorted(names)
    return kink_check([masks[k] for k in names], [pre[k] for k in names])
