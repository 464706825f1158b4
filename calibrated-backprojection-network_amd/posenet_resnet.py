"""The pose networks the reference trains -- PoseNetModel(encoder_type='resnet18' | 'resnet34'), src/kbnet.py:221-226 -- eval-mode
forward, on the HIP kernels of csrc/conv_affine.hip and the head of csrc/posenet.hip.

  reference class                                           here
  net_utils.ResNetBlock       src/net_utils.py:572-667      ResNetBlock
  networks.ResNetEncoder      src/networks.py:674-996       ResNetEncoder
  networks.PoseDecoder        src/networks.py:1992-2075     ResNetPoseDecoder   (n_filters = [256, 256]: hidden layers)
  posenet_model.PoseNetModel  src/posenet_model.py:21-206   ResNetPoseNetModel  (its encoder_type 'resnet18' / 'resnet34')

Same constructor arguments and `state_dict()` keys as the reference, so `posenet-kitti.pth`, `posenet-void1500.pth` and every
`pose_model-*.pth` its training writes load with strict=True; `load_pose_model(path)` picks the class from the checkpoint's keys.
By default inference: BatchNorm2d uses its running statistics, nothing is recorded; no CPU path.

Training (reference src/kbnet.py:392-453) is an opt-in at construction, ResNetPoseNetModel(..., trainable=True): requires_grad_(True)
and set_batch_norm('batch') then work as on PoseNetModel and the forward runs layer by layer on the kernels of
csrc/posenet_backward.hip and csrc/conv_affine_backward.hip, recording autograd; `train()` still raises.

Launches per forward: conv1, the pool, per block conv1 and conv2 (conv2's epilogue adds the skip and applies the second
activation) plus a 1 x 1 projection launch in the four blocks whose input changes shape, two decoder convs and the head:
  ResNet-18   1 + 1 + 2 x 8 + 4 + 2 + 1 = 25        ResNet-34   1 + 1 + 2 x 16 + 4 + 2 + 1 = 41
"""

from __future__ import annotations

from typing import List, Optional

import torch

from . import ops
from ._lib import KbnError
from .posenet import PoseConv2d, PoseModelBase, PoseNetModel, _DecoderConv, _fused_slope, _state

RESNET_BLOCKS = {18: (2, 2, 2, 2), 34: (3, 4, 6, 3)}
RESNET_FILTERS = (16, 32, 64, 128, 256)
RESNET_DECODER_FILTERS = (256, 256)


class ResNetConv2d(PoseConv2d):
    """net_utils.Conv2d of kernel 1, 3 or 7 at stride 1 or 2 in eval mode, in one launch (ops.conv2d_affine): PoseConv2d's
    parameters, keys and caches, with conv2d_affine's packed weight.  Without batch norm (the projection) scale is 1, shift 0."""

    def __init__(self, in_channels, out_channels, kernel_size, stride, weight_initializer, slope, use_batch_norm=True):
        super().__init__(in_channels, out_channels, kernel_size, weight_initializer, slope)
        from .modules import _PackedBlob   # (modules.py imports this file at its end: not at the top)
        self.stride = stride
        self._packed = _PackedBlob(ops.pack_conv2d_affine_weight)
        if not use_batch_norm:
            del self.batch_norm

    def affine(self):
        if hasattr(self, "batch_norm"):
            return super().affine()
        w = self.conv.weight
        if self._scale is None or self._scale.device != w.device:
            self._scale = torch.ones(self.out_channels, device=w.device)
            self._shift = torch.zeros(self.out_channels, device=w.device)
        return self._scale, self._shift

    def conv_recorded(self, inputs: List[torch.Tensor]):
        """`run_unfused` (PoseConv2d's: conv, [batch statistics], BatchNorm + activation; the conv alone without batch norm)
        starts from this conv."""
        return ops.conv2d_pose(inputs, self.conv.weight, self.stride, packed=self.packed(), packed_t=self.packed_t)

    @torch.no_grad()
    def run(self, inputs: List[torch.Tensor], residual: Optional[torch.Tensor] = None, out=None):
        if self.training:
            raise KbnError("PoseNet on the HIP path is inference only: BatchNorm2d runs on its running statistics (call eval())")
        scale, shift = self.affine()
        return ops.conv2d_affine(inputs, self.packed(), scale, shift, self.out_channels, self.kernel_size, stride=self.stride,
                                 negative_slope=self.slope, residual=residual, out=out)


class ResNetBlock(torch.nn.Module):
    """reference net_utils.ResNetBlock (src/net_utils.py:572-667) with use_batch_norm=True, eval mode.  `activation_func` is the
    NAME (the reference's class takes the function its encoder made of the name).  act(act(bn(conv2(h))) + X): the activation
    runs twice on the main path, as in the reference.  `projection` exists, and is in the state dict, whether used or not."""

    def __init__(self, in_channels, out_channels, stride=1, weight_initializer="kaiming_uniform", activation_func="leaky_relu",
                 use_batch_norm=True, use_instance_norm=False, use_depthwise_separable=False):
        super().__init__()
        if use_instance_norm or not use_batch_norm or use_depthwise_separable:
            raise KbnError("ResNetBlock on the HIP path: use_batch_norm=True, no instance norm, no depthwise-separable convs")
        slope = _fused_slope(activation_func)
        self.in_channels, self.out_channels, self.stride = in_channels, out_channels, stride
        self.conv1 = ResNetConv2d(in_channels, out_channels, 3, stride, weight_initializer, slope)
        self.conv2 = ResNetConv2d(out_channels, out_channels, 3, 1, weight_initializer, slope)
        self.projection = ResNetConv2d(in_channels, out_channels, 1, stride, weight_initializer, None, use_batch_norm=False)

    def projects(self, x) -> bool:
        """The reference's test (src/net_utils.py:658-664): the output's shape or channel count differs from the input's."""
        h, w = x.shape[2:]
        return (-(-h // self.stride), -(-w // self.stride)) != (h, w) or self.in_channels != self.out_channels

    def run(self, x, out=None):
        h = self.conv1.run([x])
        skip = self.projection.run([x]) if self.projects(x) else x
        return self.conv2.run([h], residual=skip, out=out)

    def run_unfused(self, x, batch: bool, inner: Optional[dict] = None, name: str = ""):
        """`run` layer by layer (reference src/net_utils.py:643-667), recordable: conv1 and conv2 as conv, [batch statistics],
        BatchNorm + activation, the projection's conv where the block projects, then ops.add_act.  An identity skip never touches
        `projection`.  `inner`: a dict that receives the outputs of conv1 and conv2 under `name`.conv1 / `name`.conv2."""
        h = self.conv1.run_unfused([x], batch)
        a = self.conv2.run_unfused([h], batch)
        skip = self.projection.run_unfused([x], batch) if self.projects(x) else x
        if inner is not None:
            inner[name + ".conv1"], inner[name + ".conv2"] = h, a
        return ops.add_act(a, skip, self.conv2.slope)

    def forward(self, x):
        return self.run(x)


class ResNetEncoder(torch.nn.Module):
    """reference networks.ResNetEncoder (src/networks.py:674-996) for n_layer 18 or 34 with use_batch_norm=True, eval mode.
    `forward(x)` takes the concat like the reference and returns (latent, skips); `encode([image0, image1])` reads the two
    images in place."""

    def __init__(self, n_layer, input_channels=3, n_filters=[32, 64, 128, 256, 256], weight_initializer="kaiming_uniform",
                 activation_func="leaky_relu", use_batch_norm=False, use_instance_norm=False, use_depthwise_separable=False):
        super().__init__()
        if n_layer not in RESNET_BLOCKS:
            raise KbnError(f"ResNetEncoder on the HIP path: n_layer 18 or 34 (basic blocks), got {n_layer}")
        if use_instance_norm or not use_batch_norm or use_depthwise_separable:
            raise KbnError("ResNetEncoder on the HIP path: use_batch_norm=True, no instance norm, no depthwise-separable convs "
                           "(what the reference's PoseNetModel builds)")
        n_filters = list(n_filters)
        n_blocks = list(RESNET_BLOCKS[n_layer])
        n_blocks += [n_blocks[-1]] * (len(n_filters) - len(n_blocks) - 1)           # src/networks.py:722-725
        if len(n_filters) != len(n_blocks) + 1 or len(n_filters) > 7:
            raise KbnError(f"ResNetEncoder: five to seven filter counts, got {len(n_filters)}")
        self.n_layer = n_layer
        self.conv1 = ResNetConv2d(input_channels, n_filters[0], 7, 2, weight_initializer, _fused_slope(activation_func))
        cin = n_filters[0]
        self.stages = []
        for stage, (count, f) in enumerate(zip(n_blocks, n_filters[1:]), 2):
            blocks = []
            for b in range(count):
                blocks.append(ResNetBlock(cin, f, 2 if (b == 0 and stage > 2) else 1, weight_initializer, activation_func))
                cin = f
            setattr(self, f"blocks{stage}", torch.nn.Sequential(*blocks))
            self.stages.append(f"blocks{stage}")
        self.eval()

    def blocks(self):
        return [b for name in self.stages for b in getattr(self, name)]

    def encode(self, inputs: List[torch.Tensor], return_layers: bool = False):
        """The latent, or every layer output in order: conv1, the pool, every block."""
        outs = [self.conv1.run(list(inputs))]
        outs.append(ops.maxpool3x3s2(outs[-1]))
        for block in self.blocks():
            outs.append(block.run(outs[-1]))
        return outs if return_layers else outs[-1]

    def encode_unfused(self, inputs: List[torch.Tensor], batch: bool = False, inner: Optional[dict] = None):
        """`encode(..., return_layers=True)` layer by layer, recordable.  conv1 reads the images, which are data: its node
        launches no data gradient.  The pool is recorded when its input carries a gradient."""
        outs = [self.conv1.run_unfused(list(inputs), batch)]
        outs.append(ops.maxpool3x3s2(outs[-1]))
        for name in self.stages:
            for b, block in enumerate(getattr(self, name)):
                outs.append(block.run_unfused(outs[-1], batch, inner, f"{name}.{b}"))
        return outs

    def forward(self, x):
        outs = self.encode([x], return_layers=True)
        ends, at = [outs[0]], 1
        for name in self.stages:
            at += len(getattr(self, name))
            ends.append(outs[at])
        return ends[-1], ends[:-1]


class ResNetPoseDecoder(torch.nn.Module):
    """reference networks.PoseDecoder (src/networks.py:1992-2075) WITH hidden layers: 3 x 3 stride-2 convs (BatchNorm2d,
    activation), then the 1 x 1 conv to 6 channels, mean over H W, x 0.01, pose_matrix (ops.pose_head).  Keys conv.0 ... conv.n;
    posenet.PoseDecoder is the n_filters=[] form, whose single conv has the key `conv.conv.weight`."""

    def __init__(self, rotation_parameterization="axis", input_channels=256, n_filters=list(RESNET_DECODER_FILTERS),
                 weight_initializer="kaiming_uniform", activation_func="leaky_relu", use_batch_norm=True, use_instance_norm=False):
        super().__init__()
        if rotation_parameterization != "axis":
            raise KbnError(f"PoseDecoder: rotation_parameterization 'axis' only (the reference's pose_matrix knows no other), got "
                           f"{rotation_parameterization!r}")
        if not len(n_filters) or use_instance_norm or not use_batch_norm:
            raise KbnError("ResNetPoseDecoder on the HIP path: hidden layers with use_batch_norm=True (the decoder of the ResNet "
                           "encoder types); posenet.PoseDecoder is the decoder without hidden layers")
        self.rotation_parameterization = rotation_parameterization
        slope = _fused_slope(activation_func)
        layers, cin = [], input_channels
        for f in n_filters:
            layers.append(ResNetConv2d(cin, f, 3, 2, weight_initializer, slope))
            cin = f
        layers.append(_DecoderConv(cin, weight_initializer))
        self.conv = torch.nn.Sequential(*layers)
        self.eval()

    def hidden(self):
        return list(self.conv)[:-1]

    @torch.no_grad()
    def forward(self, x, return_dof: bool = False, return_layers: bool = False):
        outs = []
        for layer in self.hidden():
            x = layer.run([x])
            outs.append(x)
        res = ops.pose_head(x, self.conv[-1].conv.weight, return_dof=return_dof)
        return (res, outs) if return_layers else res


class ResNetPoseNetModel(PoseModelBase):
    """Inference counterpart of reference `PoseNetModel(encoder_type='resnet18' | 'resnet34')` (src/posenet_model.py:55-87), a
    sibling of PoseNetModel over the same base (device, checkpoint and re-pack plumbing).  'linear' (no activation; the
    reference's block cannot run it) is accepted as PoseNetModel does.  `encoder_type` names the reference's argument."""

    def __init__(self, n_layer=18, rotation_parameterization="axis", weight_initializer="xavier_normal",
                 activation_func="leaky_relu", device=torch.device("cuda"), n_filters=RESNET_FILTERS,
                 decoder_filters=RESNET_DECODER_FILTERS, trainable: bool = False):
        self.device = device
        self.n_layer = n_layer
        self.encoder = ResNetEncoder(n_layer, input_channels=6, n_filters=list(n_filters), weight_initializer=weight_initializer,
                                     activation_func=activation_func, use_batch_norm=True)
        self.decoder = ResNetPoseDecoder(rotation_parameterization=rotation_parameterization, input_channels=list(n_filters)[-1],
                                         n_filters=list(decoder_filters), weight_initializer=weight_initializer,
                                         activation_func=activation_func, use_batch_norm=True)
        self.encoder_type = f"resnet{n_layer}"
        self._has_backward = bool(trainable)     # requires_grad_(True) and set_batch_norm refuse without it
        self.batch_norm_mode = "running"
        self._place(device)

    def forward(self, image0, image1, return_all: bool = False, return_inner: bool = False):
        """`return_all` (extension): (pose, dof N x 6, layer outputs: conv1, the pool, every block, the decoder's hidden layers).

        Built with trainable=True, with grad mode on and a parameter that requires grad the pose carries a grad_fn: the network
        runs layer by layer (ResNetBlock.run_unfused, the kernels of csrc/posenet_backward.hip and csrc/conv_affine_backward.hip),
        the head in recorded torch operations; so it does under set_batch_norm('batch'), recorded or not.  Otherwise this is the
        fused eval-mode forward, nothing recorded.  `return_inner` (layer-by-layer path only): a fourth element, the dict
        blocks{s}.{b}.conv1 / .conv2 -> the outputs of every block's two convs (conv2's before the skip is added)."""
        if not isinstance(image0, torch.Tensor) or not isinstance(image1, torch.Tensor) or image0.dim() != 4 or \
                image0.shape[1] != 3 or image0.shape != image1.shape:
            raise KbnError("ResNetPoseNetModel.forward: image0 and image1 must be N x 3 x H x W tensors of one shape")
        record = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        batch = self.batch_norm_mode == "batch"
        if not record and not batch:
            if return_inner:
                raise KbnError("ResNetPoseNetModel.forward: return_inner exists on the layer-by-layer path only (a recorded forward or "
                               "set_batch_norm('batch')): the fused forward never materialises a block's inner activations")
            with torch.no_grad():
                layers = self.encoder.encode([image0, image1], return_layers=True)
                (pose, dof), hidden = self.decoder(layers[-1], return_dof=True, return_layers=True)
            return (pose, dof, layers + hidden) if return_all else pose
        if record:
            for t, name in ((image0, "image0"), (image1, "image1")):
                if t.requires_grad:
                    raise KbnError(f"ResNetPoseNetModel.forward: {name} requires grad, but it is data and gets no gradient (gradients "
                                   "exist for the parameters); detach it")
        inner = {}
        with torch.set_grad_enabled(record):
            layers = self.encoder.encode_unfused([image0, image1], batch, inner)
            x = layers[-1]
            for layer in self.decoder.hidden():
                x = layer.run_unfused([x], batch)
                layers.append(x)
            weight = self.decoder.conv[-1].conv.weight
            if record:
                pose, dof = ops.pose_head_recorded(x, weight)
            else:
                pose, dof = ops.pose_head(x, weight, return_dof=True)
        if return_inner:
            return pose, dof, layers, inner
        return (pose, dof, layers) if return_all else pose


def _strip(sd):
    return {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}


def _pose_layout(enc, dec):
    """('posenet', filters, None) or ('resnet18' | 'resnet34', filters, decoder filters) from two state dicts, else None."""
    def count(prefix):
        return len({k[len(prefix):].split(".")[0] for k in enc if k.startswith(prefix)})

    def width(key, sd=enc):
        return int(sd[key].shape[0])

    try:
        if any(k.startswith("blocks") for k in enc):
            blocks = tuple(count(f"blocks{s}.") for s in range(2, 6))
            n_layer = {v: k for k, v in RESNET_BLOCKS.items()}.get(blocks)
            if n_layer is None or count("blocks6.") or "conv1.conv.weight" not in enc:
                return None
            filters = [width("conv1.conv.weight")] + [width(f"blocks{s}.0.conv1.conv.weight") for s in range(2, 6)]
            last = max(int(k.split(".")[1]) for k in dec if k.startswith("conv.") and k.split(".")[1].isdigit())
            return f"resnet{n_layer}", filters, [width(f"conv.{i}.conv.weight", dec) for i in range(last)]
        convs = count("conv")
        if convs == 7 and "conv.conv.weight" in dec:
            return "posenet", [width(f"conv{i}.conv.weight") for i in range(1, 8)], None
    except (KeyError, ValueError, IndexError, AttributeError):
        pass
    return None


def load_pose_model(checkpoint_path, device=torch.device("cuda"), activation_func="leaky_relu", trainable: bool = False):
    """The restored pose model of a reference checkpoint (src/posenet_model.py:150-198), of the class its keys call for: a
    PoseNetModel for the seven-conv encoder, a ResNetPoseNetModel for ResNet-18 / 34 (told apart by the block counts of blocks2 ..
    blocks5); the widths come from the weight shapes.  A checkpoint does not record the activation: `activation_func`.
    `trainable`: ResNetPoseNetModel's argument (PoseNetModel always has its backward pass)."""
    ckpt = torch.load(checkpoint_path, map_location=device)
    if not isinstance(ckpt, dict) or "encoder_state_dict" not in ckpt or "decoder_state_dict" not in ckpt:
        raise KbnError(f"load_pose_model: {checkpoint_path} is no pose checkpoint (encoder_state_dict / decoder_state_dict); it holds "
                       f"{sorted(ckpt) if isinstance(ckpt, dict) else type(ckpt).__name__}")
    enc, dec = _strip(ckpt["encoder_state_dict"]), _strip(ckpt["decoder_state_dict"])
    layout = _pose_layout(enc, dec)
    if layout is None:
        raise KbnError(f"load_pose_model: {checkpoint_path} has neither the 'posenet' nor the 'resnet18' / 'resnet34' layout; "
                       f"encoder keys {sorted(enc)}, decoder keys {sorted(dec)}")
    kind, filters, decoder_filters = layout
    if kind == "posenet":
        model = PoseNetModel(device=device, activation_func=activation_func, n_filters=filters)
    else:
        model = ResNetPoseNetModel(int(kind[6:]), device=device, activation_func=activation_func, n_filters=filters,
                                   decoder_filters=decoder_filters, trainable=trainable)
    model.load_state_dicts(enc, dec)
    return model
