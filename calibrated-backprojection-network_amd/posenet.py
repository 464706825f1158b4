"""The reference's pose network, eval-mode forward, on the HIP kernels of csrc/posenet.hip.

  reference class                                           here
  networks.PoseEncoder        src/networks.py:536-671       PoseEncoder
  networks.PoseDecoder        src/networks.py:1992-2075     PoseDecoder
  posenet_model.PoseNetModel  src/posenet_model.py:21-206   PoseNetModel

Same constructor arguments, `forward(image0, image1)` and `state_dict()` keys as the reference, so a `pose_model-*.pth`
checkpoint loads with strict=True.  By default inference: BatchNorm2d uses its running statistics (a per-channel scale and shift
in the conv's epilogue), nothing is recorded, eight launches per forward: seven convs and the head.  No CPU path.

Training (reference src/kbnet.py:392-453) is switched on by PoseNetModel.requires_grad_(True) and, for the reference's train-mode
BatchNorm, set_batch_norm('batch'): the forward then runs layer by layer on the kernels of csrc/posenet_backward.hip and records
autograd (ops.conv2d_s2, ops.batch_norm_act); `train()` still raises and the torch modules stay in eval mode.
"""

from __future__ import annotations

from typing import List, Optional

import torch

from . import ops, optim
from ._lib import KbnError

POSENET_FILTERS = (16, 32, 64, 128, 256, 256, 256)
POSENET_KERNELS = (7, 5, 3, 3, 3, 3, 3)


def _fused_slope(activation_func: str) -> Optional[float]:
    """The reference's factory (src/net_utils.py:23-45: same substring tests, same order) narrowed to what the conv's epilogue
    fuses: max(v, slope v)."""
    if "linear" in activation_func:
        return None
    if "leaky_relu" in activation_func:
        return 0.20
    if "relu" in activation_func:
        return 0.0
    raise KbnError(f"PoseNet on the HIP path fuses leaky_relu, relu or linear into its convs, not {activation_func!r}")


def _init_weight(weight, weight_initializer):
    if weight_initializer == "kaiming_normal":
        torch.nn.init.kaiming_normal_(weight)
    elif weight_initializer == "xavier_normal":
        torch.nn.init.xavier_normal_(weight)
    elif weight_initializer == "xavier_uniform":
        torch.nn.init.xavier_uniform_(weight)
    elif weight_initializer != "kaiming_uniform":
        raise ValueError("Unsupported weight initializer: {}".format(weight_initializer))


def _state(*tensors):
    return tuple((t.data_ptr(), t._version, t.device) for t in tensors)


class _BareConv(torch.nn.Module):
    """Holds `conv.weight` under the reference's key (its net_utils.Conv2d wraps a torch.nn.Conv2d named `conv`)."""

    def __init__(self, in_channels, out_channels, kernel_size):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.empty(out_channels, in_channels, kernel_size, kernel_size), requires_grad=False)
        torch.nn.init.kaiming_uniform_(self.weight, a=5 ** 0.5)   # torch.nn.Conv2d's default: what 'kaiming_uniform' leaves in place


class PoseConv2d(torch.nn.Module):
    """net_utils.Conv2d(stride=2, use_batch_norm=True) in eval mode: conv, BatchNorm2d on its running statistics, activation, in
    one launch (ops.conv2d_s2_affine).  The packed weight (a modules._PackedBlob) and the scale / shift vectors are cached and
    rebuilt when a parameter or buffer changes (in place, replaced or moved)."""

    sync_group = None     # a kb.dist.BatchNormGroup once the model's sync_batch_norm has set one: 'batch' mode spans its ranks

    def __init__(self, in_channels, out_channels, kernel_size, weight_initializer, slope):
        super().__init__()
        self.in_channels, self.out_channels, self.kernel_size, self.stride = in_channels, out_channels, kernel_size, 2
        self.slope = slope
        self.conv = _BareConv(in_channels, out_channels, kernel_size)
        _init_weight(self.conv.weight, weight_initializer)
        self.batch_norm = torch.nn.BatchNorm2d(out_channels)
        for p in self.batch_norm.parameters():
            p.requires_grad_(False)
        from .modules import _PackedBlob   # (modules.py imports this file at its end: not at the top)
        self._packed = _PackedBlob(ops.pack_conv2d_s2_affine_weight)
        self._akey = self._scale = self._shift = None

    def packed(self):
        return self._packed.get(self.conv.weight)

    def packed_t(self, weight=None):
        """The weight as the data gradient of this (k, stride) reads it (ops.pack_conv2d_data_gradient_weight), re-packed when the
        weight changed.  A _PackedBlob like `_packed`, made on the first data gradient (modules.data_gradient_blob): refresh_packed
        re-packs it only once it exists and its weight has changed, which the next backward would do anyway."""
        from .modules import data_gradient_blob
        return data_gradient_blob(self, self.conv.weight if weight is None else weight)

    def affine(self):
        """scale = g * rsqrt(var + eps), shift = b - mean * scale (BatchNorm2d.eval()), fp32 on the weights' device."""
        bn = self.batch_norm
        key = _state(bn.weight, bn.bias, bn.running_mean, bn.running_var)
        if key != self._akey:
            with torch.no_grad():
                scale = bn.weight * torch.rsqrt(bn.running_var + bn.eps)
                shift = bn.bias - bn.running_mean * scale
            if self._scale is not None and self._scale.device == scale.device:
                self._scale.copy_(scale)
                self._shift.copy_(shift)
            else:
                self._scale, self._shift = scale.contiguous(), shift.contiguous()
            self._akey = key
        return self._scale, self._shift

    @torch.no_grad()
    def run(self, inputs: List[torch.Tensor], out=None):
        if self.training:
            raise KbnError("PoseNet on the HIP path is inference only: BatchNorm2d runs on its running statistics (call eval())")
        scale, shift = self.affine()
        return ops.conv2d_s2_affine(inputs, self.packed(), scale, shift, self.out_channels, self.kernel_size,
                                    negative_slope=self.slope, out=out)

    def conv_recorded(self, inputs: List[torch.Tensor]):
        """The bias-free conv alone, as a differentiable node."""
        return ops.conv2d_s2(inputs, self.conv.weight, packed=self.packed(), packed_t=self.packed_t)

    def run_unfused(self, inputs: List[torch.Tensor], batch: bool):
        """The layer as conv, [batch statistics], BatchNorm + activation: what the fused launch of `run` cannot be when the
        backward needs the conv's output or the statistics are the batch's own.  Recorded for autograd when grad mode is on and
        a parameter requires grad.  `batch`: normalise with the statistics of this batch and update the running ones as
        torch.nn.BatchNorm2d does in train mode (src/net_utils.py:103-104); the module's `training` flag stays False.  With a
        `sync_group` the batch is the frames of every rank of the group (ops.batch_norm_act_sync)."""
        u = self.conv_recorded(inputs)
        bn = getattr(self, "batch_norm", None)
        if bn is None:       # (posenet_resnet.ResNetConv2d without batch norm: the projection)
            return u
        group = self.sync_group
        if batch:
            count = u.shape[0] * u.shape[2] * u.shape[3]
            if count <= 1 and (group is None or group.world == 1):      # (more ranks, a frame each: the global count is 2 or more)
                raise KbnError(f"set_batch_norm('batch'): a {tuple(u.shape)} map has one value per channel, no batch statistics "
                               "(torch.nn.BatchNorm2d raises there too)")
        if batch and group is not None:      # the statistics of every rank's frames (PoseModelBase.sync_batch_norm)
            y, mean, _, unbiased = ops.batch_norm_act_sync(u, bn.weight, bn.bias, group, bn.eps, self.slope, return_stats=True)
            with torch.no_grad():
                bn.running_mean.mul_(1.0 - bn.momentum).add_(mean, alpha=bn.momentum)
                bn.running_var.mul_(1.0 - bn.momentum).add_(unbiased, alpha=bn.momentum)
                bn.num_batches_tracked.add_(1)
            return y
        if batch:
            mean, var = ops.batch_norm_stats(u.detach())
            with torch.no_grad():
                momentum = bn.momentum
                bn.running_mean.mul_(1.0 - momentum).add_(mean, alpha=momentum)
                bn.running_var.mul_(1.0 - momentum).add_(var, alpha=momentum * count / (count - 1.0))   # the UNBIASED variance
                bn.num_batches_tracked.add_(1)
        else:
            mean, var = bn.running_mean, bn.running_var
        return ops.batch_norm_act(u, bn.weight, bn.bias, mean, var, bn.eps, self.slope, batch)

    def forward(self, x):
        return self.run([x])


class PoseEncoder(torch.nn.Module):
    """reference networks.PoseEncoder (src/networks.py:536-671) with use_batch_norm=True, eval mode.  `forward(x)` takes the
    6-channel concat like the reference; `encode([image0, image1])` reads the two images in place."""

    def __init__(self, input_channels=6, n_filters=list(POSENET_FILTERS), weight_initializer="kaiming_uniform",
                 activation_func="leaky_relu", use_batch_norm=True, use_instance_norm=False):
        super().__init__()
        if use_instance_norm or not use_batch_norm:
            raise KbnError("PoseEncoder on the HIP path: use_batch_norm=True, use_instance_norm=False (what PoseNetModel builds)")
        if len(n_filters) != len(POSENET_KERNELS):
            raise KbnError(f"PoseEncoder has {len(POSENET_KERNELS)} layers, got {len(n_filters)} filter counts")
        slope = _fused_slope(activation_func)
        cin = input_channels
        for i, (f, k) in enumerate(zip(n_filters, POSENET_KERNELS), 1):
            setattr(self, f"conv{i}", PoseConv2d(cin, f, k, weight_initializer, slope))
            cin = f
        self.eval()

    def layers(self):
        return [getattr(self, f"conv{i}") for i in range(1, len(POSENET_KERNELS) + 1)]

    def encode(self, inputs: List[torch.Tensor], return_layers: bool = False):
        outs = []
        x = list(inputs)
        for layer in self.layers():
            outs.append(layer.run(x))
            x = [outs[-1]]
        return outs if return_layers else outs[-1]

    def encode_unfused(self, inputs: List[torch.Tensor], batch: bool = False, return_layers: bool = False):
        """`encode` through PoseConv2d.run_unfused: three launches a layer (four with batch statistics), recordable."""
        outs = []
        x = list(inputs)
        for layer in self.layers():
            outs.append(layer.run_unfused(x, batch))
            x = [outs[-1]]
        return outs if return_layers else outs[-1]

    def forward(self, x):
        return self.encode([x]), None


class _DecoderConv(torch.nn.Module):
    def __init__(self, in_channels, weight_initializer):
        super().__init__()
        self.conv = _BareConv(in_channels, 6, 1)
        _init_weight(self.conv.weight, weight_initializer)


class PoseDecoder(torch.nn.Module):
    """reference networks.PoseDecoder (src/networks.py:1992-2075) with n_filters=[]: 1 x 1 conv to 6 channels, mean over H W,
    x 0.01, pose_matrix -- one launch (ops.pose_head)."""

    def __init__(self, rotation_parameterization="axis", input_channels=256, n_filters=[], weight_initializer="kaiming_uniform",
                 activation_func="leaky_relu", use_batch_norm=False, use_instance_norm=False):
        super().__init__()
        if rotation_parameterization != "axis":
            raise KbnError(f"PoseDecoder: rotation_parameterization 'axis' only (the reference's pose_matrix knows no other), got "
                           f"{rotation_parameterization!r}")
        if len(n_filters) or use_batch_norm or use_instance_norm:
            raise KbnError("PoseDecoder on the HIP path has no hidden layers (n_filters=[]: the decoder of encoder_type='posenet')")
        self.rotation_parameterization = rotation_parameterization
        self.conv = _DecoderConv(input_channels, weight_initializer)
        self.eval()

    @torch.no_grad()
    def forward(self, x, return_dof: bool = False):
        return ops.pose_head(x, self.conv.conv.weight, return_dof=return_dof)


class PoseModelBase(object):
    """What the pose models share (PoseNetModel here, posenet_resnet.ResNetPoseNetModel): the device, checkpoint and re-pack
    plumbing of reference `PoseNetModel` (src/posenet_model.py:114-206) over `self.encoder`, `self.decoder` and `self.device`,
    which a subclass's constructor sets before it calls `_place(device)`."""

    def _place(self, device):
        self.data_parallel()
        self.to(device)
        self.eval()

    def modules(self):
        return (self.encoder, self.decoder)

    def refresh_packed(self):
        """Re-packs (in place) the blobs of weights that changed since they were packed, as KBNetModel.refresh_packed."""
        from .modules import packed_blobs
        for blob in packed_blobs(self):
            blob.refresh()

    def parameters(self):
        return list(self.encoder.parameters()) + list(self.decoder.parameters())

    _has_backward = False   # PoseNetModel: True; ResNetPoseNetModel: its `trainable` argument
    batch_norm_mode = "running"

    def requires_grad_(self, flag: bool = True):
        """Sets requires_grad on every parameter (conv weights, BatchNorm weights and biases, the head's weight)."""
        if flag and not self._has_backward:
            raise KbnError(f"{type(self).__name__}.requires_grad_: this model was built without a backward pass: encoder_type='posenet' "
                           "(PoseNetModel) always has one, ResNetPoseNetModel with trainable=True")
        for p in self.parameters():
            p.requires_grad_(bool(flag))
        return self

    def set_batch_norm(self, mode: str = "running"):
        """'running' (default): BatchNorm2d normalises with its running statistics, constants of the backward pass -- fine-tuning
        on frozen statistics.  'batch': what the reference's pose_model.train() does (src/kbnet.py:392-453): every layer normalises
        with the statistics of the batch, the gradient runs through them, and running_mean / running_var / num_batches_tracked are
        updated as torch.nn.BatchNorm2d updates them (momentum 0.1, unbiased variance), with gradients on or off.  A layer whose
        map holds one value per channel raises."""
        if not self._has_backward:
            raise KbnError(f"{type(self).__name__}.set_batch_norm: this model has no backward pass (ResNetPoseNetModel: build it with "
                           "trainable=True)")
        if mode not in ("running", "batch"):
            raise KbnError(f"{type(self).__name__}.set_batch_norm: 'running' or 'batch', got {mode!r}")
        self.batch_norm_mode = mode
        return self

    def sync_batch_norm(self, group=None):
        """`group` (a kb.dist.BatchNormGroup): in 'batch' mode every BatchNorm layer normalises with the statistics of the frames
        of ALL the group's ranks, its backward sums over them, and the running statistics follow the merged values, equal on every
        rank -- data-parallel training then computes what one process computes on the whole batch (the reference's DataParallel
        replicas each use their own shard's statistics).  Two small collectives a layer and pass; every rank must hold a frame and
        make the same forward and backward calls in the same order.  None (default): this rank's own frames, as before.  No effect
        in 'running' mode."""
        if not self._has_backward:
            raise KbnError(f"{type(self).__name__}.sync_batch_norm: this model has no backward pass (ResNetPoseNetModel: build it "
                           "with trainable=True)")
        from .dist import BatchNormGroup
        if group is not None and not isinstance(group, BatchNormGroup):
            raise KbnError(f"{type(self).__name__}.sync_batch_norm: a kb.dist.BatchNormGroup or None, got {type(group).__name__}")
        for net in self.modules():
            for layer in net.modules():
                if isinstance(layer, PoseConv2d):
                    layer.sync_group = group
        return self

    def train(self):
        raise KbnError("the HIP path is inference only through train() / eval(): the modules stay in eval mode.  PoseNetModel and "
                       "ResNetPoseNetModel(trainable=True) train through requires_grad_(True) and set_batch_norm('batch')")

    def eval(self):
        for m in self.modules():
            m.eval()

    def to(self, device):
        for m in self.modules():
            m.to(device)
        self.device = device

    def data_parallel(self):
        """A no-op, as KBNetModel.data_parallel: one process drives one GPU; checkpoints still carry the `module.` prefix."""
        return self

    def load_state_dicts(self, sd_encoder, sd_decoder):
        """Accepts keys with or without the DataParallel `module.` prefix."""
        for m, sd in zip(self.modules(), (sd_encoder, sd_decoder)):
            sd = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}
            m.load_state_dict(sd, strict=True)

    def restore_model(self, checkpoint_path, optimizer=None):
        """Loads a reference checkpoint (reference src/posenet_model.py:174-198); its non-empty `optimizer_state_dict` goes into
        `optimizer` when one is given, and an error of load_state_dict propagates (KBNetModel.restore_model)."""
        ckpt = torch.load(checkpoint_path, map_location=self.device)
        self.load_state_dicts(ckpt["encoder_state_dict"], ckpt["decoder_state_dict"])
        optim.load_checkpoint_state(optimizer, ckpt)
        return ckpt.get("train_step", 0), optimizer

    def save_model(self, checkpoint_path, step=0, optimizer=None):
        """Writes the reference's checkpoint layout (src/posenet_model.py:150-172), keys prefixed with `module.` like its
        DataParallel-wrapped modules produce."""
        pref = lambda sd: {"module." + k: v for k, v in sd.items()}
        torch.save({"train_step": step,
                    "optimizer_state_dict": optimizer.state_dict() if optimizer is not None else {},
                    "encoder_state_dict": pref(self.encoder.state_dict()),
                    "decoder_state_dict": pref(self.decoder.state_dict())}, checkpoint_path)


class PoseNetModel(PoseModelBase):
    """Inference counterpart of reference `PoseNetModel` (src/posenet_model.py:21-206): same constructor arguments and
    `forward(image0, image1)` -> N x 4 x 4, the pose KBNetModel.compute_loss takes as pose01 / pose02."""

    def __init__(self, encoder_type="posenet", rotation_parameterization="axis", weight_initializer="xavier_normal",
                 activation_func="leaky_relu", device=torch.device("cuda"), n_filters=POSENET_FILTERS):
        if encoder_type in ("resnet18", "resnet34"):
            raise KbnError(f"PoseNetModel on the HIP path implements encoder_type='posenet' only, not {encoder_type!r} "
                           "(the ResNet pose networks are posenet_resnet.ResNetPoseNetModel; modules.load_pose_model picks the class "
                           "from a checkpoint)")
        if encoder_type != "posenet":
            raise ValueError("Unsupported PoseNet encoder type: {}".format(encoder_type))
        self.device = device
        self.encoder_type = encoder_type      # 'posenet' here, 'resnet18' / 'resnet34' on the sibling: what load_pose_model found
        self.encoder = PoseEncoder(input_channels=6, n_filters=list(n_filters), weight_initializer=weight_initializer,
                                   activation_func=activation_func, use_batch_norm=True)
        self.decoder = PoseDecoder(rotation_parameterization=rotation_parameterization, weight_initializer=weight_initializer,
                                   input_channels=list(n_filters)[-1])
        self.batch_norm_mode = "running"
        self._place(device)

    _has_backward = True

    def forward(self, image0, image1, return_all: bool = False):
        """`return_all` (extension): (pose, dof N x 6, the seven layer outputs) instead of the pose alone.

        With grad mode on and a parameter that requires grad (`requires_grad_(True)`) the pose carries a grad_fn: every layer
        runs as conv, [batch statistics], BatchNorm + activation on the kernels of csrc/posenet_backward.hip's forward side, the
        head in recorded torch operations.  Otherwise, on running statistics, this is the fused eval-mode forward: eight
        launches, nothing recorded."""
        if not isinstance(image0, torch.Tensor) or not isinstance(image1, torch.Tensor) or image0.dim() != 4 or \
                image0.shape[1] != 3 or image0.shape != image1.shape:
            raise KbnError("PoseNetModel.forward: image0 and image1 must be N x 3 x H x W tensors of one shape")
        record = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        batch = self.batch_norm_mode == "batch"
        if not record and not batch:
            with torch.no_grad():
                layers = self.encoder.encode([image0, image1], return_layers=True)
                pose, dof = self.decoder(layers[-1], return_dof=True)
            return (pose, dof, layers) if return_all else pose
        if record:
            for t, name in ((image0, "image0"), (image1, "image1")):
                if t.requires_grad:
                    raise KbnError(f"PoseNetModel.forward: {name} requires grad, but it is data and gets no gradient (gradients "
                                   "exist for the parameters); detach it")
        with torch.set_grad_enabled(record):
            layers = self.encoder.encode_unfused([image0, image1], batch, return_layers=True)
            if record:
                pose, dof = ops.pose_head_recorded(layers[-1], self.decoder.conv.conv.weight)
            else:
                pose, dof = self.decoder(layers[-1], return_dof=True)
        return (pose, dof, layers) if return_all else pose
