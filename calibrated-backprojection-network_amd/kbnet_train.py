"""The recorded forward of the depth network: KBNetModel(trainable=True).forward with grad mode on and a parameter that requires
grad.  The reference layer by layer over the module tree of modules.py -- parameters and state_dict keys are those modules' --
every layer one differentiable node of ops.py:

  reference                                                here
  SparseToDensePool.forward     src/networks.py:2168-2196    _s2d: ops.s2d_pyramid (data), ops.conv2d_kbnet for the 1 x 1 convs and the 3 x 3
  KBNetEncoder.forward          src/networks.py:301-533      _encoder, level 4's re-use of calibrated_backprojection4 included (quirk Q3)
  CalibratedBackprojectionBlock src/net_utils.py:1343-1371   _kb_block: ops.conv2d_kbnet x 3, ops.kb_xyz (proj_depth and coordinates * z)
  DecoderBlock.forward          src/net_utils.py:1453-1487   _decoder_block: ops.resize_nearest, ops.conv2d_kbnet x 2 (the skip as inputs)
  MultiScaleDecoder.forward     src/networks.py:1855-1989    forward_recorded: the five blocks, output0 (linear)
  KBNetModel.forward            src/kbnet_model.py:163-184   forward_recorded: the input's concatenation, ops.depth_map

The convs run on the fp32 kernels of kbn_conv2d_forward with the activation in their epilogue; a concatenation is several inputs of
one conv (a skip is never materialised), the resized tensor and the latent's concatenation are.  Everything the reference
concatenates or re-uses accumulates through torch's own autograd.  What is not differentiated is refused at construction (`check`).
"""

from __future__ import annotations

from typing import Dict, List, Optional

import torch

from . import ops
from ._lib import KbnError


def check(deconv_type: str, activation_func: str):
    """What KBNetModel(trainable=True) refuses: the layers this backward pass does not differentiate."""
    from .modules import _post, activation_func as make_activation
    if deconv_type != "up":
        raise KbnError(f"KBNetModel(trainable=True): deconv_type 'up' only (the transposed conv has no backward pass here), got {deconv_type!r}")
    kind = _post(make_activation(activation_func))
    if kind is not None:
        raise KbnError(f"KBNetModel(trainable=True): activation_func 'leaky_relu', 'relu' or 'linear'; {kind!r} has no backward pass here")


def activation_names(resolutions_backprojection, n_pool_convs: int = 3) -> List[str]:
    """The name of every activation tensor of the recorded forward, in forward order: the keys of `return_inner` and of the masks of
    tests/kbnet_grad_oracle.py.  A KB level has four (proj_depth's is z), a plain level two; level 4 listed is block 4 again."""
    names = [f"s2d.pool_convs.{i}" for i in range(n_pool_convs)] + ["s2d.conv", "conv0_image", "conv0_depth"]
    for level in range(5):
        kb = level in resolutions_backprojection
        names += [f"level{level}.{what}" for what in (("conv_image", "conv_depth", "proj_depth", "conv_fused") if kb else ("conv_image", "conv_depth"))]
    for i in (4, 3, 2, 1, 0):
        names += [f"deconv{i}.deconv", f"deconv{i}.conv"]
    return names


def _packed_t(layer):
    """weight -> the data gradient's blob of a modules.Conv2d, from the cache on the layer (modules.data_gradient_blob)."""
    from .modules import data_gradient_blob
    return lambda weight: data_gradient_blob(layer, weight)


def _conv(layer, inputs, inner: Dict[str, torch.Tensor], name: Optional[str]):
    """A modules.Conv2d over the concatenation of `inputs` as one node; `name`: its key in `inner` (None: a linear layer)."""
    y = ops.conv2d_kbnet(inputs, layer.conv.weight, layer.stride, layer._slope, packed=layer.packed(), packed_t=_packed_t(layer))
    if name is not None:
        inner[name] = y
    return y


def _one(block, what: str):
    """The single conv of a VGGNetBlock (KBNet builds every block with one; stacked blocks are not differentiated here)."""
    convs = list(block.conv_block)
    if len(convs) != 1:
        raise KbnError(f"KBNetModel(trainable=True): {what} stacks {len(convs)} convs; the recorded path takes one per block")
    return convs[0]


def _s2d(s2d, x, inner):
    mins, maxs = s2d.min_pool_sizes, s2d.max_pool_sizes
    if s2d.len_pool_sizes <= 8:
        y = ops.s2d_pyramid(x, mins, maxs)
    else:   # as SparseToDensePool.forward: eight pools per launch, channel order of src/networks.py:2170-2189
        parts = [ops.s2d_pyramid(x, mins[i:i + 8], []) for i in range(0, len(mins), 8)]
        parts += [ops.s2d_pyramid(x, [], maxs[i:i + 8]) for i in range(0, len(maxs), 8)]
        y = torch.cat(parts, dim=1)
    for i, conv in enumerate(s2d.pool_convs):
        y = _conv(conv, [y], inner, f"s2d.pool_convs.{i}")
    return _conv(s2d.conv, [y, x], inner, "s2d.conv")


def _kb_block(blk, image, depth, coordinates, fused, inner, name):
    """reference src/net_utils.py:1343-1371 -> (conv_image, conv_depth, conv_fused)."""
    conv_image = _conv(_one(blk.conv_image, name + ".conv_image"), [image], inner, name + ".conv_image")
    conv_depth = _conv(_one(blk.conv_depth, name + ".conv_depth"), [depth, coordinates], inner, name + ".conv_depth")
    proj = blk.proj_depth
    xyz, z = ops.kb_xyz(depth, proj.conv.weight, coordinates, proj._slope, packed=proj.packed(), packed_t=_packed_t(proj))
    inner[name + ".proj_depth"] = z
    conv_fused = _conv(blk.conv_fused, [image, xyz] + ([] if fused is None else [fused]), inner, name + ".conv_fused")
    return conv_image, conv_depth, conv_fused


def _encoder(enc, image, depth, intrinsics, inner):
    """reference src/networks.py:301-533 -> (latent parts, skips), every skip the list of tensors the reference concatenates."""
    n, _, h0, w0 = image.shape
    h1, w1 = (h0 + 1) // 2, (w0 + 1) // 2
    kinv0 = ops.intrinsics_inverse(intrinsics, 1.0, 1.0)
    kinv1 = None
    conv_image = _conv(enc.conv0_image, [image], inner, "conv0_image")
    conv_depth = _conv(enc.conv0_depth, [depth], inner, "conv0_depth")
    conv_fused = None
    skips = []
    listed = enc.resolutions_backprojection
    if 4 in listed and 3 not in listed:
        raise AttributeError("'KBNetEncoder' object has no attribute 'calibrated_backprojection4'")   # as in the reference
    for level in range(5):
        h, w = conv_image.shape[2:]
        name = f"level{level}"
        if level in listed:
            if level > 0 and kinv1 is None:   # Q1: every deeper KB level scales K by the level-1 ratio (src/networks.py:342-343)
                kinv1 = ops.intrinsics_inverse(intrinsics, w1 / w0, h1 / h0)
            coordinates = ops.camera_coordinates(kinv0 if level == 0 else kinv1, h, w)
            blk = getattr(enc, f"calibrated_backprojection{min(level, 3) + 1}")   # Q3: level 4 calls block 4 again (:499-517)
            conv_image, conv_depth, conv_fused = _kb_block(blk, conv_image, conv_depth, coordinates, conv_fused, inner, name)
            out = [conv_fused, conv_depth]
        else:
            src = conv_fused if conv_fused is not None else conv_image
            conv_image = _conv(_one(getattr(enc, f"conv{level + 1}_image"), name + ".conv_image"), [src], inner, name + ".conv_image")
            conv_depth = _conv(_one(getattr(enc, f"conv{level + 1}_depth"), name + ".conv_depth"), [conv_depth], inner, name + ".conv_depth")
            conv_fused = None
            out = [conv_image, conv_depth]
        if level == 4:
            return out, skips
        skips.append(out)


def _decoder_block(blk, x, skip, shape, inner, name):
    """reference src/net_utils.py:1453-1487 with deconv_type 'up': resize to the skip's size (or `shape`), conv, conv over
    cat[., skip] -- the skip's tensors as further inputs of that conv."""
    if skip:
        shape = skip[0].shape[2:4]
    up = ops.resize_nearest(x, int(shape[0]), int(shape[1]))
    y = _conv(blk.deconv.conv, [up], inner, name + ".deconv")
    return _conv(blk.conv, [y] + list(skip), inner, name + ".conv")


def forward_recorded(model, image, sparse_depth, validity_map_depth, intrinsics, return_inner: bool = False):
    """KBNetModel.forward with autograd recording -> the N x 1 x H x W fp32 depth with a grad_fn; with `return_inner` also the dict
    name -> activation (activation_names) in forward order."""
    given = (("image", image, 3), ("sparse_depth", sparse_depth, 1), ("validity_map_depth", validity_map_depth, 1), ("intrinsics", intrinsics, None))
    for name, t, _ in given:
        if not isinstance(t, torch.Tensor):
            raise KbnError(f"KBNetModel.forward: {name} must be a tensor, got {type(t).__name__}")
        if t.requires_grad:
            raise KbnError(f"KBNetModel.forward: {name} requires grad, but it is data and gets no gradient (gradients exist for the "
                           "parameters); detach it")
    if image.dim() != 4 or sparse_depth.dim() != 4 or sparse_depth.shape != validity_map_depth.shape or \
            sparse_depth.shape[1] != 1 or image.shape[0] != sparse_depth.shape[0] or image.shape[2:] != sparse_depth.shape[2:]:
        raise KbnError("KBNetModel.forward: image N x C x H x W, sparse_depth and validity_map_depth N x 1 x H x W of one size")
    inner: Dict[str, torch.Tensor] = {}
    x = torch.cat([sparse_depth, validity_map_depth], dim=1)   # reference src/kbnet_model.py:161
    shape = x.shape[-2:]
    depth = _s2d(model.sparse_to_dense_pool, x, inner)
    latent, skips = _encoder(model.encoder, image.contiguous(), depth, intrinsics.contiguous(), inner)
    dec = model.decoder
    y = torch.cat(latent, dim=1)
    for i in (4, 3, 2, 1):
        y = _decoder_block(getattr(dec, f"deconv{i}"), y, skips[i - 1], None, inner, f"deconv{i}")
    d0 = dec.deconv0
    if d0.skip_channels:
        raise KbnError("KBNetModel(trainable=True): deconv0 takes no skip in KBNet's decoder")
    y = _decoder_block(d0, y, [], shape, inner, "deconv0")
    logits = _conv(dec.output0, [y], inner, None)
    out = ops.depth_map(logits, model.min_predict_depth, model.max_predict_depth)
    return (out, inner) if return_inner else out
