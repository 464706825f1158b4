"""Host-side mirror of the reference's operator interface for the inference hot path.

Same class names, constructor arguments, `forward()` signatures and `state_dict()`
keys as the reference (so its checkpoints load and `kbnet_model.py` can use these as
drop-ins), but every `forward` is a sequence of HIP launches through the C ABI
(ops.py).  Inference by default: nothing is recorded for autograd (KBNetModel(trainable=True) is the opt-in, kbnet_train.py) and there
is no CPU path.

  reference class                              here
  net_utils.Conv2d            src/net_utils.py:51-141      Conv2d
  net_utils.UpConv2d          src/net_utils.py:441-499     UpConv2d
  net_utils.VGGNetBlock       src/net_utils.py:878-958     VGGNetBlock
  net_utils.CalibratedBackprojectionBlock :1269-1371       CalibratedBackprojectionBlock
  net_utils.DecoderBlock      src/net_utils.py:1377-1487   DecoderBlock
  networks.SparseToDensePool  src/networks.py:2078-2196    SparseToDensePool
  networks.KBNetEncoder       src/networks.py:24-533       KBNetEncoder
  networks.MultiScaleDecoder  src/networks.py:1605-1989    MultiScaleDecoder
  kbnet_model.KBNetModel      src/kbnet_model.py:24-186    KBNetModel
"""

from __future__ import annotations

import os
from typing import List, Optional

import torch

from . import _lib, ops, optim
from ._lib import KbnError
from .config import KBNetConfig


# ------------------------------------------------------------------- activations
def activation_func(activation_fn: str):
    """Same factory contract as reference src/net_utils.py:23-45 (same substring tests, same order, same modules).  The kernels
    fuse LeakyReLU (slope 0.20 from this factory), ReLU (slope 0) and linear; ELU and sigmoid run as a pass of their own behind a
    conv launched without activation (_post), which takes the whole model to its layer-by-layer form."""
    if "linear" in activation_fn:
        return None
    if "leaky_relu" in activation_fn:
        return torch.nn.LeakyReLU(negative_slope=0.20, inplace=True)
    if "relu" in activation_fn:
        return torch.nn.ReLU()
    if "elu" in activation_fn:
        return torch.nn.ELU()
    if "sigmoid" in activation_fn:
        return torch.nn.Sigmoid()
    raise ValueError("Unsupported activation function: {}".format(activation_fn))


def _slope(act) -> Optional[float]:
    """What the conv kernels fuse: the slope of max(v, slope v), or None for a launch without activation (a linear layer, or one
    whose activation follows as its own pass: _post)."""
    if act is None or _post(act) is not None:
        return None
    if isinstance(act, torch.nn.LeakyReLU):
        return float(act.negative_slope)
    if isinstance(act, torch.nn.ReLU):
        return 0.0
    raise ValueError("Activation not supported by the HIP kernels: {}".format(type(act).__name__))


def _post(act) -> Optional[str]:
    """'elu' / 'sigmoid' for the activations that run behind the conv (ops.activation_), else None."""
    if isinstance(act, torch.nn.ELU):
        if act.alpha != 1.0:
            raise ValueError("ELU: alpha = 1 (torch.nn.ELU(), what the reference's factory builds) is what the HIP kernel computes")
        return "elu"
    if isinstance(act, torch.nn.Sigmoid):
        return "sigmoid"
    return None


def _finish(layer, out, out_absmax):
    """The activation pass of a layer whose activation the kernels do not fuse (ELU, sigmoid); it folds max |out| per frame into the
    tensor's slot -- the conv in front of it was given none -- so that split-operand convs downstream place their fp16 windows on
    the activated values."""
    if layer._post is not None:
        ops.activation_(out, layer._post, out_absmax)
    return out


def _init_weight(weight, weight_initializer):
    if weight_initializer == "kaiming_normal":
        torch.nn.init.kaiming_normal_(weight)
    elif weight_initializer == "xavier_normal":
        torch.nn.init.xavier_normal_(weight)
    elif weight_initializer == "xavier_uniform":
        torch.nn.init.xavier_uniform_(weight)
    elif weight_initializer == "kaiming_uniform":
        pass
    else:
        raise ValueError("Unsupported weight initializer: {}".format(weight_initializer))


class _PackedBlob:
    """Caches the blob a packer (`pack(*weights, out=None, **opts)`, one of ops.pack_*_weight) makes of one or more weights; re-packs
    when a weight is modified in place (version bump), replaced or moved, or when an option changes.  A re-pack goes INTO the
    existing blob (`out=`: same size, same device), so device pointers recorded in a captured HIP graph stay valid
    (GraphedForward re-packs before replaying when it sees a parameter change: KBNetModel.refresh_packed finds every instance
    that is an attribute of a sub-module, see packed_blobs)."""

    def __init__(self, pack):
        self._pack = pack
        self._key = self._blob = self._args = None

    def get(self, *weights, **opts):
        key = ([(w.data_ptr(), w._version, w.device) for w in weights], opts)
        if key != self._key:
            self._blob = self._pack(*weights, out=self._blob, **opts)
            self._key, self._args = key, (weights, opts)
        return self._blob

    def refresh(self):
        """Re-packs if (and only if) this blob has been built before and a weight changed since."""
        if self._blob is not None:
            self.get(*self._args[0], **self._args[1])


def packed_blobs(model):
    """Every _PackedBlob that is an instance attribute of a sub-module of `model` (a KBNetModel / PoseNetModel)."""
    return [v for top in model.modules() for sub in top.modules() for v in vars(sub).values() if isinstance(v, _PackedBlob)]


def data_gradient_blob(layer, weight):
    """`weight` (the conv weight of `layer`: a Conv2d here, a PoseConv2d, a ResNetConv2d) as the data gradient of the layer's
    (kernel size, stride) reads it.  The _PackedBlob is made on the first data gradient -- a model that never trains carries none --
    and packed_blobs() finds it from then on."""
    blob = layer.__dict__.get("_packed_bwd_data")
    if blob is None:
        blob = layer._packed_bwd_data = _PackedBlob(ops.pack_conv2d_data_gradient_weight)
    return blob.get(weight, stride=layer.stride)


# ------------------------------------------------------------------------ layers
def _run_split(layer, weight, srcs, n, h, w, out=None, up2x=False, out_absmax=None, stats=None, pair_out=False, transposed=False):
    """Conv2d.run_split for `layer` = a Conv2d (weight = its OIHW parameter) or, with `transposed` and `up2x`, a TransposeConv2d
    (weight = its in x out x 3 x 3 parameter: the folded up-conv kernels on the layer's own taps)."""
    kinds_ok = all((s.kind == _lib.KBN_SRC_TENSOR or (i == 0 and s.kind == _lib.KBN_SRC_PAIR)) and s.channels % 16 == 0
                   for i, s in enumerate(srcs))
    if (not layer.split or layer.kernel_size != 3 or (up2x and w % 4) or len(srcs) > 2 or (up2x and layer.stride != 1)
            or not kinds_ok or (pair_out and layer._post is not None)):   # (a pair tensor holds what the KERNEL wrote: no ELU / sigmoid behind it)
        return None
    # narrow layers stay on the fp32 kernels (a 64-filter tile would be mostly padding) -- except the folded up-conv,
    # which has 16-filter tiles for them (deconv0's 64 -> 12 at full resolution)
    narrow_up = up2x and layer.split_narrow_up and layer.out_channels <= 16 and layer.in_channels % 32 == 0
    if layer.out_channels < 48 and not narrow_up:
        return None
    dev = weight.device
    srcs = Conv2d._with_slots(srcs, n, dev, stats)
    if pair_out:
        if stats is None or (layer.out_channels % 8 and not narrow_up) or (layer.stride != 1 and up2x):
            return None
        # (the narrow folded up-conv writes 16 channels, zeros past its filters: the decoder tail's input)
        out = ops.PairTensor(n, 16 if narrow_up else layer.out_channels, h, w, dev, stats)
        if layer.stride == 2:
            out.with_sub()   # the even pixels in fp32 too: the next level's 1x1 stride-2 conv_fused reads those
        if out_absmax is not None:
            out.absmax = out_absmax
    elif out is None:
        out = torch.empty((n, layer.out_channels, h, w), device=dev, dtype=torch.float32)
    packed = layer._split_blob(up2x)
    # the latency form (KBNetModel.set_latency_mode): a launch too small for the chip spreads every tile's K loop over several workgroups
    ks = 1
    if getattr(layer, "latency", 0) and not pair_out and all(s.kind == _lib.KBN_SRC_TENSOR for s in srcs):
        ks = ops.ksplit_for(sum(s.channels for s in srcs), layer.out_channels, h, w, layer.stride, up2x=up2x, frames=layer.latency)
    kw = dict(up2x=up2x, negative_slope=layer._slope, stride=layer.stride, folded_up2x=up2x, out_absmax=None if layer._post else out_absmax,
              transposed=transposed)
    res = ops.conv3x3_split(srcs, packed, n, layer.out_channels, h, w, out, ksplit=ks, **kw) if ks > 1 else None
    if res is None:
        res = ops.conv3x3_split(srcs, packed, n, layer.out_channels, h, w, out, **kw)
    return res if res is None else _finish(layer, res, out_absmax)


class Conv2d(torch.nn.Module):
    """Bias-free conv (padding k//2) + activation; kernel sizes 1 and 3, strides 1 and 2."""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1,
                 weight_initializer="kaiming_uniform",
                 activation_func=torch.nn.LeakyReLU(negative_slope=0.10, inplace=True),
                 use_batch_norm=False, use_instance_norm=False):
        super().__init__()
        if use_batch_norm or use_instance_norm:
            raise ValueError("normalisation layers are not part of the KBNet inference path")
        if kernel_size not in (1, 3) or stride not in (1, 2):
            raise ValueError("HIP conv supports kernel_size in {1,3} and stride in {1,2}")
        self.conv = torch.nn.Conv2d(in_channels, out_channels, kernel_size=kernel_size, stride=stride,
                                    padding=kernel_size // 2, bias=False)
        _init_weight(self.conv.weight, weight_initializer)
        self.activation_func = activation_func
        self.kernel_size, self.stride = kernel_size, stride
        self.in_channels, self.out_channels = in_channels, out_channels
        self._slope = _slope(activation_func)
        self._post = _post(activation_func)
        self._packed = _PackedBlob(ops.pack_conv_weight)
        self._packed_split = _PackedBlob(ops.pack_conv3x3_split_weight)      # fp32-grade products on the 16-bit matrix core (ops.conv3x3_split)
        self._packed_split_up = _PackedBlob(ops.pack_conv3x3_split_weight)   # the same for the folded nearest-2x up-conv
        self._packed_split_1x1 = _PackedBlob(ops.pack_conv1x1s2_split_weight)   # conv_fused of the KB block
        # conv_fused on split operands from this width on: KB3 / KB4 (192 / 384 filters: 239 vs 285 and 152 vs 253 us per 32
        # KITTI frames); at KB2's 96 filters the layer is bound by its stride-2 HBM reads either way (365 vs 342 us)
        self.split_fused_min_filters = 192
        self.split = True   # fp32-grade 3x3 convs on the 16-bit matrix core where the shape qualifies
        # the folded up-conv of a layer with at most 16 filters has 16-filter tiles (upconv2x_split16_kernel): deconv0's
        # 64 -> 12 up-conv.  Level with the fp32 9-product kernel on random operands (650 vs 640 us per 32 KITTI frames),
        # 8-11 % faster inside the forward (660-690 vs 745 us, tools/layer_profile.py)
        self.split_narrow_up = True

    @staticmethod
    def _with_slots(srcs, n, dev, stats):
        """Every tensor source of a split-operand launch carries its per-frame max |a| slot (ops.ActStats): the kernel
        places its fp16 window on the data of THIS call.  Sources that come without one (a drop-in module called on
        its own, reference code in front of it) are measured here by a pass over the tensor -- no host sync, no state."""
        for s in srcs:
            if s.kind == _lib.KBN_SRC_TENSOR and (not s.absmax or (stats is not None and not stats.usable(s.absmax))):
                if stats is None:
                    stats = ops.ActStats(n, dev, capacity=len(srcs))
                slot = stats.measure(s._keep[0])
                s.absmax = slot.data_ptr()
                s._keep = (s._keep[0], slot)
        return srcs

    def _split_blob(self, up2x):
        """The blob ops.conv3x3_split reads for this layer; `up2x`: as the folded nearest-2x up-conv."""
        if up2x:
            return self._packed_split_up.get(self.conv.weight, folded_up2x=True)
        return self._packed_split.get(self.conv.weight, stride=self.stride)

    def run_split(self, srcs, n, h, w, out=None, up2x=False, out_absmax=None, stats=None, pair_out=False):
        """3x3 stride-1 conv with two-term fp16 splits of both operands (ops.conv3x3_split, fp32-grade results); `h` x `w`
        is the OUTPUT size.  None when the layer or the shape does not qualify.  `pair_out`: the result as an
        ops.PairTensor (for a split-operand consumer; its absmax slot is `out_absmax` when given); source 0 may be one
        (ops.pair_src).  A shape the pair kernels decline returns None like any other: the caller retries in fp32."""
        return _run_split(self, self.conv.weight, srcs, n, h, w, out, up2x, out_absmax, stats, pair_out)

    def split_fused_qualifies(self, ci, cf):
        return (self.split and self.kernel_size == 1 and self.stride == 2 and ci % 16 == 0 and cf % 16 == 0
                and self.out_channels >= self.split_fused_min_filters and self.in_channels == ci + 3 + cf)

    def run_split_fused(self, image, fused, xyz, n, h, w, out, amax_image=None, amax_fused=None, out_absmax=None, stats=None):
        """conv_fused of a KB block -- this 1x1 stride-2 conv over cat[image, xyz, fused] -- with the tensor channels on
        split operands and the three xyz channels (ops.kb_xyz_s2) in fp32 (ops.conv1x1s2_split); `h` x `w` is the OUTPUT
        size.  None when the layer or the shapes do not qualify."""
        ci, cf = image.shape[1], (0 if fused is None else fused.shape[1])
        if not self.split_fused_qualifies(ci, cf):
            return None
        if isinstance(image, ops.PairTensor):   # the previous level's conv_image as a pair tensor: its fp32 even-pixel side output
            if image.sub is None or fused is None:
                return None
            image, amax_image = image.sub, image.absmax
        srcs = [ops.tensor_src(image, "image", amax_image)] + ([] if fused is None else [ops.tensor_src(fused, "fused", amax_fused)])
        srcs = self._with_slots(srcs, n, image.device, stats)
        packed = self._packed_split_1x1.get(self.conv.weight, xyz_offset=ci)   # (the first xyz channel)
        return ops.conv1x1s2_split(srcs, packed, xyz, n, self.out_channels, h, w, out, negative_slope=self._slope,
                                   out_absmax=out_absmax)

    def packed(self):
        return self._packed.get(self.conv.weight, stride=self.stride)

    def run(self, srcs, n, in_h, in_w, out=None, resize=False, out_absmax=None, stats=None):
        """`out_absmax`: slot (ops.ActStats) that receives max |out| per frame; `stats`: where slots for unmeasured
        inputs come from (split-operand launches only)."""
        cin = sum(s.channels for s in srcs)
        if cin != self.in_channels:   # the packed blob carries no size: a wrong count would read past the weight panel
            raise KbnError(f"expected {self.in_channels} input channels in total, got {cin}")
        oh, ow = -(-in_h // self.stride), -(-in_w // self.stride)
        if not resize:
            res = self.run_split(srcs, n, oh, ow, out=out, out_absmax=out_absmax, stats=stats)   # (_run_split finishes the layer)
            if res is not None:
                return res
        if out is None:
            out = torch.empty((n, self.out_channels, oh, ow), device=self.conv.weight.device, dtype=torch.float32)
        # ELU / sigmoid (_post): the conv without activation and without the slot, then the activation in place (_finish fills the slot)
        res = ops.conv2d(srcs, self.packed(), n, self.out_channels, self.kernel_size, self.stride, in_h, in_w, out,
                         resize=resize, negative_slope=self._slope, out_absmax=None if self._post else out_absmax)
        return _finish(self, res, out_absmax)

    def forward(self, x):
        if x.shape[1] != self.in_channels:
            raise KbnError(f"expected {self.in_channels} input channels, got {x.shape[1]}")
        x = x if _dense(x) else x.contiguous()
        return self.run([ops.tensor_src(x, "x")], x.shape[0], x.shape[2], x.shape[3])


class _SideBranch:
    """Launches issued inside the `with` block go to a side stream that forks from the current stream at the point where
    the object was CREATED and joins it when the block ends -- independent kernels of one level (the KB block's conv_depth
    and conv_fused beside its conv_image) then share the GPU instead of queueing.  Works eagerly and under HIP-graph
    capture (the fork / join become graph edges).  Tensors that outlive the block must be allocated outside it (on the
    current stream); what is allocated inside must also die inside.  KBN_NO_OVERLAP=1 keeps everything on one stream."""

    _streams = {}
    enabled = None        # None: follow KBN_NO_OVERLAP as the library read it (ops.knob; ops.reload_env() refreshes); True / False force
    only_from = None      # raw handle of the one stream that may fork (set while a multi-branch graph is captured), or None

    def __init__(self, device):
        # under capture only: eagerly the extra events cost more host time than the overlap returns (batch 1: 1.59 -> 1.68 ms)
        self.on = bool(device.type == "cuda" and torch.cuda.is_current_stream_capturing()
                       and (_SideBranch.enabled if _SideBranch.enabled is not None else ops.knob("KBN_NO_OVERLAP") == 0))
        if self.on:
            self.cur = torch.cuda.current_stream(device)
            if _SideBranch.only_from is not None and self.cur.cuda_stream != _SideBranch.only_from:
                self.on = False
                return
            key = (device.index, self.cur.cuda_stream)
            self.side = _SideBranch._streams.get(key)
            if self.side is None:
                self.side = _SideBranch._streams[key] = torch.cuda.Stream(device=device)
            self.fork = self.cur.record_event()

    def __enter__(self):
        if self.on:
            self.side.wait_event(self.fork)
            self._ctx = torch.cuda.stream(self.side)
            self._ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if self.on:
            self._ctx.__exit__(*exc)
            self.cur.wait_stream(self.side)
        return False


class _KnobSwitch:
    """A boolean A/B switch of the host mirror that is ON unless its KBN_NO_* variable is set -- as the LIBRARY read the
    environment (ops.knob: at load time and on ops.reload_env(), like the C side's own switches) -- or unless the attribute
    was assigned on the instance (tests, tools)."""

    def __init__(self, *names, enable=None):
        self.names = names
        self.enable = enable      # an opt-IN variable: the switch is ON only when it is set (and no KBN_NO_* name is)

    def __set_name__(self, owner, name):
        self.attr = "_force_" + name

    def __get__(self, obj, objtype=None):
        if obj is None:
            return self
        forced = obj.__dict__.get(self.attr)
        if forced is not None:
            return forced
        return all(ops.knob(n) == 0 for n in self.names) and (self.enable is None or ops.knob(self.enable) != 0)

    def __set__(self, obj, value):
        obj.__dict__[self.attr] = None if value is None else bool(value)


def _dense(t):
    return t.stride(3) == 1 and t.stride(2) == t.shape[3] and t.stride(1) == t.shape[2] * t.shape[3]


class UpConv2d(torch.nn.Module):
    """interpolate(nearest, size=shape) -> conv3x3, with the resize folded into the conv's
    tile staging (no upsampled tensor is materialised)."""

    def __init__(self, in_channels, out_channels, kernel_size=3, weight_initializer="kaiming_uniform",
                 activation_func=torch.nn.LeakyReLU(negative_slope=0.10, inplace=True),
                 use_batch_norm=False, use_instance_norm=False):
        super().__init__()
        self.conv = Conv2d(in_channels, out_channels, kernel_size=kernel_size, stride=1,
                           weight_initializer=weight_initializer, activation_func=activation_func,
                           use_batch_norm=use_batch_norm, use_instance_norm=use_instance_norm)
        self._packed_up2x = _PackedBlob(ops.pack_upconv2x_weight)
        self.split_up = True    # folded 16-product form on split operands (ops.conv3x3_split(folded_up2x=True))

    out_channels = property(lambda self: self.conv.out_channels)

    def forward(self, x, shape, amax=None, out_absmax=None, stats=None, pair_out=False):
        """`amax` / `out_absmax` / `stats` (extensions): the per-frame max |a| slot of `x`, the slot to fill for the result,
        the slot pool of the forward (ops.ActStats).  `x` may be an ops.PairTensor (the previous concat conv's output in
        the producer-written split format): the folded split kernels stage it by DMA.  `pair_out`: the result as an
        ops.PairTensor.  Either way None if the pair kernels decline the layer or the shape."""
        if x.shape[1] != self.conv.in_channels:
            raise KbnError(f"expected {self.conv.in_channels} input channels, got {x.shape[1]}")
        if isinstance(x, ops.PairTensor) or pair_out:
            pair_in = isinstance(x, ops.PairTensor)
            if not pair_in:
                x = x if _dense(x) else x.contiguous()
            n, _, h, w = x.shape
            oh, ow = int(shape[0]), int(shape[1])
            if (oh, ow) != (2 * h, 2 * w) or self.conv.kernel_size != 3 or not self.split_up:
                return None
            src = ops.pair_src(x, "x") if pair_in else ops.tensor_src(x, "x", amax)
            return self.conv.run_split([src], n, oh, ow, up2x=True, out_absmax=out_absmax, stats=stats, pair_out=pair_out)
        x = x if _dense(x) else x.contiguous()
        n, _, h, w = x.shape
        oh, ow = int(shape[0]), int(shape[1])
        if (oh, ow) == (2 * h, 2 * w) and self.conv.kernel_size == 3:
            if self.split_up:
                res = self.conv.run_split([ops.tensor_src(x, "x", amax)], n, oh, ow, up2x=True, out_absmax=out_absmax, stats=stats)
                if res is not None:
                    return res
            # exact 2x: four 2x2 phase convs on the low-res input (4/9 of the MACs)
            out = torch.empty((n, self.conv.out_channels, oh, ow), device=x.device, dtype=torch.float32)
            res = ops.upconv2x(x, self._packed_up2x.get(self.conv.conv.weight), self.conv.out_channels, out,
                               self.conv._slope, out_absmax=None if self.conv._post else out_absmax)
            return _finish(self.conv, res, out_absmax)
        return self.conv.run([ops.tensor_src(x, "x", amax)], n, oh, ow, resize=True, out_absmax=out_absmax, stats=stats)


class TransposeConv2d(torch.nn.Module):
    """ConvTranspose2d(kernel 3, stride 2, padding 1, output_padding 1, no bias) + activation: the decoder blocks' up-sampling layer
    with deconv_type='transpose' (reference src/net_utils.py:350-440; parameter `deconv.weight`, in x out x 3 x 3).  The output is
    exactly twice the input; by output parity the layer is four small convs on its input, i.e. the folded up-conv's kernels with the
    layer's nine taps in nine of their sixteen phase weights (csrc/conv_split.hip uf_fold, csrc/conv_up2x.hip pack_up2x_kernel)."""

    def __init__(self, in_channels, out_channels, kernel_size=3, weight_initializer="kaiming_uniform",
                 activation_func=torch.nn.LeakyReLU(negative_slope=0.10, inplace=True),
                 use_batch_norm=False, use_instance_norm=False):
        super().__init__()
        if use_batch_norm or use_instance_norm:
            raise ValueError("normalisation layers are not part of the KBNet inference path")
        if kernel_size != 3:
            raise ValueError("the HIP transposed conv is the decoder's: kernel_size 3")
        self.deconv = torch.nn.ConvTranspose2d(in_channels, out_channels, kernel_size=kernel_size, stride=2,
                                               padding=kernel_size // 2, output_padding=1, bias=False)
        _init_weight(self.deconv.weight, weight_initializer)
        self.activation_func = activation_func
        self.kernel_size, self.stride = kernel_size, 1    # as _run_split sees the layer: an up-conv
        self.in_channels, self.out_channels = in_channels, out_channels
        self._slope = _slope(activation_func)
        self._post = _post(activation_func)
        self._packed_split_up = _PackedBlob(ops.pack_conv3x3_split_weight)   # the folded up-conv kernels on the layer's own taps
        self._packed_up2x = _PackedBlob(ops.pack_upconv2x_weight)            # the fp32 four-phase kernels
        self.split = True
        self.split_narrow_up = True

    def _split_blob(self, up2x=True):
        return self._packed_split_up.get(self.deconv.weight, folded_up2x=True, transposed=True)

    def forward(self, x, shape=None, amax=None, out_absmax=None, stats=None, pair_out=False):
        """`shape` is accepted and ignored, as in the reference's DecoderBlock (:1468-1469: the transposed conv fixes the size).
        Extensions as UpConv2d.forward; None when `x` is an ops.PairTensor or `pair_out` is asked for and the split kernels
        decline the layer or the shape."""
        if x.shape[1] != self.in_channels:
            raise KbnError(f"expected {self.in_channels} input channels, got {x.shape[1]}")
        pair_in = isinstance(x, ops.PairTensor)
        if not pair_in:
            x = x if _dense(x) else x.contiguous()
        n, _, h, w = x.shape
        oh, ow = 2 * h, 2 * w
        w_t = self.deconv.weight
        src = ops.pair_src(x, "x") if pair_in else ops.tensor_src(x, "x", amax)
        res = _run_split(self, w_t, [src], n, oh, ow, up2x=True, out_absmax=out_absmax, stats=stats, pair_out=pair_out, transposed=True)
        if res is not None or pair_in or pair_out:
            return res
        out = torch.empty((n, self.out_channels, oh, ow), device=x.device, dtype=torch.float32)
        res = ops.upconv2x(x, self._packed_up2x.get(w_t, transposed=True), self.out_channels, out, self._slope,
                           out_absmax=None if self._post else out_absmax, transposed=True)
        return _finish(self, res, out_absmax)


class VGGNetBlock(torch.nn.Module):
    def __init__(self, in_channels, out_channels, n_convolution=1, stride=1,
                 weight_initializer="kaiming_uniform",
                 activation_func=torch.nn.LeakyReLU(negative_slope=0.10, inplace=True),
                 use_batch_norm=False, use_instance_norm=False, use_depthwise_separable=False):
        super().__init__()
        if use_depthwise_separable:
            raise ValueError("depthwise separable convolutions are not part of the KBNet path")
        layers = []
        for _ in range(n_convolution - 1):
            layers.append(Conv2d(in_channels, out_channels, 3, 1, weight_initializer, activation_func,
                                 use_batch_norm, use_instance_norm))
            in_channels = out_channels
        layers.append(Conv2d(in_channels, out_channels, 3, stride, weight_initializer, activation_func,
                             use_batch_norm, use_instance_norm))
        self.conv_block = torch.nn.Sequential(*layers)

    def run(self, srcs, n, h, w, out=None, out_absmax=None, stats=None):
        """Every conv of the block in turn (reference src/net_utils.py:945-958): the stride-1 convs in front write fresh
        tensors, the last one (the block's stride) writes `out` and fills `out_absmax`.  `srcs`: the sources of the FIRST conv
        (a concatenation is just several of them); `h` x `w` is the input size."""
        convs = list(self.conv_block)
        x = None
        for i, conv in enumerate(convs):
            last = i == len(convs) - 1
            x = conv.run(srcs if i == 0 else [ops.tensor_src(x, "x")], n, h, w, out=out if last else None,
                         out_absmax=out_absmax if last else None, stats=stats)
        return x

    def forward(self, x):
        return self.conv_block(x)


class CalibratedBackprojectionBlock(torch.nn.Module):
    """KB layer.  forward(image, depth, coordinates, fused=None) as in the reference;
    `coordinates` may also be the N x 3 x 3 inverse intrinsics of this level, in which case
    K^-1 [x y 1]^T is generated inside the kernels instead of being read from HBM."""

    def __init__(self, in_channels_image, in_channels_depth, in_channels_fused, n_filter_image=48,
                 n_filter_depth=16, n_filter_fused=48, n_convolution_image=1, n_convolution_depth=1,
                 n_convolution_fused=1, weight_initializer="kaiming_uniform",
                 activation_func=torch.nn.LeakyReLU(negative_slope=0.10, inplace=True)):
        super().__init__()
        # n_convolution_image / n_convolution_depth > 1 (reference src/net_utils.py:1311-1325): stride-1 convs stacked in front of
        # a branch's stride-2 conv; such a block runs conv by conv (_run_stacked), the fused launches are KBNet's one-conv form.
        # n_convolution_fused is accepted and unused, as in the reference (conv_fused is ONE 1x1 conv, :1335-1341)
        self.stacked = n_convolution_image != 1 or n_convolution_depth != 1
        self.conv_image = VGGNetBlock(in_channels_image, n_filter_image, n_convolution_image, 2,
                                      weight_initializer, activation_func)
        self.conv_depth = VGGNetBlock(in_channels_depth + 3, n_filter_depth, n_convolution_depth, 2,
                                      weight_initializer, activation_func)
        self.proj_depth = Conv2d(in_channels_depth, 1, kernel_size=1, stride=1,
                                 weight_initializer=weight_initializer, activation_func=activation_func)
        self.conv_fused = Conv2d(in_channels_fused + 3, n_filter_fused, kernel_size=1, stride=2,
                                 weight_initializer=weight_initializer, activation_func=activation_func)
        self.n_filter_image, self.n_filter_depth, self.n_filter_fused = n_filter_image, n_filter_depth, n_filter_fused
        self.split_image = n_filter_image >= 96   # conv_image on the split-operand kernel (KB1's 48 filters: the fused kernel wins)
        self.split_fused = True   # ... and with it conv_fused (1x1 stride 2) on split operands, xyz in fp32
        self._slope = _slope(activation_func)
        # the fused launches are written around max(v, slope v): a block without activation, or with ELU / sigmoid (reference
        # src/net_utils.py:23-45), runs conv by conv like a stacked one, z = act(proj_depth . depth) as a tensor of its own
        self.layerwise = self._slope is None

    def run(self, image, depth, coordinates, fused, out_image=None, out_depth=None, out_fused=None,
            amax_image=None, amax_fused=None, out_amax_image=None, out_amax_skip=None, stats=None, need_image=True,
            pair_image_out=False, fused_done=False):
        """amax_image / amax_fused: per-frame max |a| slots of `image` / `fused` (ops.ActStats; measured here when a
        split-operand conv needs one that is missing); out_amax_image: slot to fill for conv_image's output;
        out_amax_skip: ONE slot for conv_fused's and conv_depth's outputs (the encoder keeps them in one skip tensor)."""
        # `fused_done`: `out_fused` already holds this block's conv_fused (the previous level's launch computed it: ops.kb1_front's
        # `next_fused`); the paths that can honour it leave the layer out, the others recompute it (same values within single-op noise)
        # `image` may be an ops.PairTensor (with its fp32 even-pixel side output) and `pair_image_out` asks for conv_image's result
        # as one: the encoder's chain of stride-2 split convs (KBNetEncoder.encode); None when the pair kernels decline
        pair_in = isinstance(image, ops.PairTensor)
        if (pair_in or pair_image_out) and not (self.conv_image.conv_block[0].split and self.split_image and self.split_fused
                                                and coordinates.dim() == 3 and stats is not None
                                                and not self.stacked and not self.layerwise):
            return None
        n, ci, h, w = image.shape
        cd, cf = depth.shape[1], (0 if fused is None else fused.shape[1])
        want = (self.conv_image.conv_block[0].in_channels, self.conv_depth.conv_block[0].in_channels - 3,
                self.conv_fused.in_channels - 3 - self.conv_image.conv_block[0].in_channels)
        if (ci, cd, cf) != want:   # the kernels trust these counts when they walk the packed weight panels
            raise KbnError(f"KB block built for (image, depth, fused) channels {want}, got {(ci, cd, cf)}")
        if self.stacked or self.layerwise:
            return self._run_stacked(image, depth, coordinates, fused, out_image, out_depth, out_fused, out_amax_image,
                                     out_amax_skip, stats, need_image)
        oh, ow = (h + 1) // 2, (w + 1) // 2
        dev = image.device
        mk = lambda c: torch.empty((n, c, oh, ow), device=dev, dtype=torch.float32)
        out_image = mk(self.n_filter_image) if (out_image is None and not pair_image_out) else out_image
        out_depth = mk(self.n_filter_depth) if out_depth is None else out_depth
        out_fused = mk(self.n_filter_fused) if out_fused is None else out_fused
        kinv = coords = None
        if coordinates.dim() == 3:
            kinv = coordinates.contiguous()
        else:
            coords = coordinates.contiguous()
        ci_conv = self.conv_image.conv_block[0]
        if ci_conv.split and self.split_image and kinv is not None:
            # conv_image (most of the block's FLOPs) on the 16-bit matrix core (fp32-grade split operands); conv_depth and
            # conv_fused -- their inputs are synthesized in-kernel (K^-1 [x y 1]^T, backprojection) -- on the fp32 kernels
            if pair_in:
                amax_image = image.absmax
            elif amax_image is None or (stats is not None and not stats.usable(amax_image.data_ptr())):
                stats = stats if stats is not None else ops.ActStats(n, dev, capacity=3)
                amax_image = stats.measure(image)   # conv_image and conv_fused both read `image`: measured once
            branch = _SideBranch(dev)   # forks HERE: conv_depth and conv_fused read nothing that conv_image writes
            # need_image=False (KBNetEncoder.skip_unused_image): the caller never reads conv_image's output -- the reference's
            # last KB level, whose image branch feeds nothing (src/networks.py:475-523: conv5_image takes conv4_fused)
            isrc = ops.pair_src(image, "image") if pair_in else ops.tensor_src(image, "image", amax_image)
            res = True if not need_image else ci_conv.run_split([isrc], n, oh, ow, out=out_image, out_absmax=out_amax_image, stats=stats,
                                                                pair_out=pair_image_out)
            if res is None and (pair_in or pair_image_out):
                return None
            if pair_image_out and need_image:
                out_image = res
            if res is not None:
                with branch:
                    self._depth_and_fused(image, depth, fused, kinv, n, h, w, oh, ow, out_depth, out_fused, ci, cf,
                                          amax_image, amax_fused, out_amax_skip, stats, skip_fused=fused_done)
                return out_image, out_depth, out_fused
        return ops.kb_block(image, depth, coords, kinv, fused,
                            self.conv_image.conv_block[0].packed(), self.conv_depth.conv_block[0].packed(),
                            self.proj_depth.conv.weight, self.conv_fused.packed(),
                            self.n_filter_image, self.n_filter_depth, self.n_filter_fused,
                            out_image, out_depth, out_fused, self._slope, absmax_image=out_amax_image,
                            absmax_depth=out_amax_skip, absmax_fused=out_amax_skip)

    def _run_stacked(self, image, depth, coordinates, fused, out_image, out_depth, out_fused, out_amax_image, out_amax_skip, stats,
                     need_image=True):
        """A block with n_convolution_image / n_convolution_depth > 1, conv by conv: image -> (stride-1 convs) -> stride-2 conv;
        cat[depth, coordinates] -> (stride-1 convs) -> stride-2 conv; conv_fused over cat[image, xyz, fused] reads the block's
        INPUTS (reference src/net_utils.py:1343-1371).  Coordinates / backprojection channels are synthesized in the kernels
        (K^-1 given) or read from the dense tensor, never concatenated."""
        n, _, h, w = image.shape
        oh, ow = (h + 1) // 2, (w + 1) // 2
        dev = image.device
        mk = lambda c: torch.empty((n, c, oh, ow), device=dev, dtype=torch.float32)
        out_image = mk(self.n_filter_image) if out_image is None else out_image
        out_depth = mk(self.n_filter_depth) if out_depth is None else out_depth
        out_fused = mk(self.n_filter_fused) if out_fused is None else out_fused
        dense = coordinates.dim() == 4
        coordinates = coordinates.contiguous()
        if dense and tuple(coordinates.shape) != (n, 3, h, w):
            raise KbnError(f"coordinates must be N x 3 x H x W = {(n, 3, h, w)} or the N x 3 x 3 inverse intrinsics, got {tuple(coordinates.shape)}")
        if need_image:
            self.conv_image.run([ops.tensor_src(image, "image")], n, h, w, out=out_image, out_absmax=out_amax_image, stats=stats)
        csrc = ops.tensor_src(coordinates, "coordinates") if dense else ops.coords_src(coordinates)
        self.conv_depth.run([ops.tensor_src(depth, "depth"), csrc], n, h, w, out=out_depth, out_absmax=out_amax_skip, stats=stats)
        if self.proj_depth._post is not None:
            # ELU / sigmoid: z = act(proj_depth . depth) and xyz = coordinates * z as tensors (reference src/net_utils.py:1352-1359);
            # the conv kernels synthesize the backprojection only around max(v, slope v)
            z = self.proj_depth.run([ops.tensor_src(depth, "depth")], n, h, w)
            xyz = ops.tensor_src(ops.scale_planes(coordinates if dense else ops.camera_coordinates(coordinates, h, w), z), "xyz")
        else:
            xyz = (ops.xyz_src(depth, self.proj_depth.conv.weight, None, coordinates=coordinates) if dense
                   else ops.xyz_src(depth, self.proj_depth.conv.weight, coordinates))
        srcs = [ops.tensor_src(image, "image"), xyz] + ([] if fused is None else [ops.tensor_src(fused, "fused")])
        self.conv_fused.run(srcs, n, h, w, out=out_fused, out_absmax=out_amax_skip, stats=stats)
        return out_image, out_depth, out_fused

    def _depth_and_fused(self, image, depth, fused, kinv, n, h, w, oh, ow, out_depth, out_fused, ci, cf, amax_image, amax_fused,
                         out_amax_skip, stats, skip_fused=False):
        """conv_depth and conv_fused of the split path (their inputs are synthesized in-kernel: K^-1 [x y 1]^T, backprojection)."""
        self.conv_depth.conv_block[0].run([ops.tensor_src(depth, "depth"), ops.coords_src(kinv)], n, h, w, out=out_depth,
                                          out_absmax=out_amax_skip)
        if skip_fused:
            return
        if (self.split_fused and (fused is None or _dense(fused)) and self.proj_depth._slope is not None
                and self.conv_fused.split_fused_qualifies(ci, cf)):
            # conv_fused's tensor channels on the matrix core too; its backprojection channels, computed once at the
            # pixels a stride-2 1x1 conv reads, enter in fp32
            xyz = ops.kb_xyz_s2(depth, self.proj_depth.conv.weight, kinv, self.proj_depth._slope)
            if self.conv_fused.run_split_fused(image, fused, xyz, n, oh, ow, out_fused, amax_image, amax_fused,
                                               out_absmax=out_amax_skip, stats=stats) is not None:
                return
        if isinstance(image, ops.PairTensor):
            image = image.float()   # the split conv_fused declined a pair tensor's side output: decode it (rare, not fast)
        srcs = [ops.tensor_src(image, "image"), ops.xyz_src(depth, self.proj_depth.conv.weight, kinv)]
        if fused is not None:
            srcs.append(ops.tensor_src(fused, "fused"))
        self.conv_fused.run(srcs, n, h, w, out=out_fused, out_absmax=out_amax_skip)

    def forward(self, image, depth, coordinates, fused=None):
        image = image if _dense(image) else image.contiguous()
        depth = depth if _dense(depth) else depth.contiguous()
        if fused is not None and not _dense(fused):
            fused = fused.contiguous()
        return self.run(image, depth, coordinates, fused)


class DecoderBlock(torch.nn.Module):
    pair_mid = _KnobSwitch("KBN_NO_PAIR_MID")   # A/B switch: the up-conv -> concat-conv tensor as a PairTensor

    def __init__(self, in_channels, skip_channels, out_channels, weight_initializer="kaiming_uniform",
                 activation_func=torch.nn.LeakyReLU(negative_slope=0.10, inplace=True),
                 use_batch_norm=False, use_instance_norm=False, deconv_type="up",
                 use_depthwise_separable=False):
        super().__init__()
        if use_depthwise_separable:
            raise ValueError("depthwise separable convolutions are not part of the KBNet path")
        if deconv_type not in ("up", "transpose"):   # (the reference builds such a block and fails in forward: `deconv` unbound)
            raise ValueError("Unsupported deconv_type: {}".format(deconv_type))
        self.skip_channels = skip_channels
        self.deconv_type = deconv_type
        # reference src/net_utils.py:1413-1434: TransposeConv2d / UpConv2d, kernel 3, the block's activation
        deconv = TransposeConv2d if deconv_type == "transpose" else UpConv2d
        self.deconv = deconv(in_channels, out_channels, 3, weight_initializer, activation_func, use_batch_norm, use_instance_norm)
        self.conv = Conv2d(skip_channels + out_channels, out_channels, 3, 1, weight_initializer,
                           activation_func, use_batch_norm, use_instance_norm)

    def latency_splitk(self, h, w):
        """In the latency form (KBNetModel.set_latency_mode): would this block's up-conv (input h x w) or its concat conv launch
        split-K?  Such a block runs on fp32 tensors."""
        frames = getattr(self.conv, "latency", 0)
        if not frames:
            return False
        up = self.deconv.conv if isinstance(self.deconv, UpConv2d) else self.deconv
        return (ops.ksplit_for(up.in_channels, up.out_channels, 2 * h, 2 * w, 1, up2x=True, frames=frames) > 1
                or ops.ksplit_for(self.conv.in_channels, self.conv.out_channels, 2 * h, 2 * w, 1, frames=frames) > 1)

    def forward(self, x, skip=None, shape=None, amax_x=None, amax_skip=None, out_absmax=None, stats=None, pair_out=False):
        """amax_x / amax_skip / out_absmax / stats (extensions): per-frame max |a| slots of the inputs, the slot to fill
        for the result and the slot pool of the forward (ops.ActStats); missing input slots are measured.  `x` may be an
        ops.PairTensor and `pair_out` asks for one (the decoder's chain of split-operand kernels, MultiScaleDecoder);
        None when the pair kernels decline a shape (the caller repeats the block in fp32)."""
        if pair_out and (not self.conv.split or self.conv.out_channels < 48
                         or self.conv.out_channels % 8 or self.conv.kernel_size != 3 or self.conv._post is not None):
            return None   # declined before anything is launched
        if self.deconv_type == "transpose":
            # the transposed conv fixes the size (reference :1468-1469: `shape` and the skip's size are not consulted); a skip of
            # another size fails in the reference's torch.cat -- here before anything is launched
            shape = (2 * x.shape[2], 2 * x.shape[3])
            if skip is not None and self.skip_channels > 0 and tuple(skip.shape[2:4]) != shape:
                raise RuntimeError(f"Sizes of tensors must match except in dimension 1. Expected size {shape} but got size "
                                   f"{tuple(skip.shape[2:4])} for the skip connection (deconv_type='transpose' doubles the size)")
        elif skip is not None:
            shape = skip.shape[2:4]
        elif shape is None:
            shape = (2 * x.shape[2], 2 * x.shape[3])
        if stats is None:
            stats = ops.ActStats(x.shape[0], x.data.device if isinstance(x, ops.PairTensor) else x.device, capacity=4)
        amax_deconv = stats.new()
        # inside the pair chain the up-conv's output goes to the concat conv as a PairTensor too (that kernel wants at least
        # two 16-channel chunks from each of its two sources)
        deconv = None
        if (pair_out and self.pair_mid and skip is not None and self.skip_channels >= 32 and self.deconv.out_channels >= 32):
            deconv = self.deconv(x, shape=shape, amax=amax_x, out_absmax=amax_deconv, stats=stats, pair_out=True)
        if deconv is None:
            deconv = self.deconv(x, shape=shape, amax=amax_x, out_absmax=amax_deconv, stats=stats)
        if deconv is None:
            return None
        srcs = [ops.pair_src(deconv, "deconv") if isinstance(deconv, ops.PairTensor) else ops.tensor_src(deconv, "deconv", amax_deconv)]
        if self.skip_channels > 0:
            skip = skip if _dense(skip) else skip.contiguous()
            srcs.append(ops.tensor_src(skip, "skip", amax_skip))  # torch.cat([deconv, skip]) fused into the K loop
        if pair_out:
            return self.conv.run_split(srcs, x.shape[0], int(shape[0]), int(shape[1]), out_absmax=out_absmax, stats=stats, pair_out=True)
        return self.conv.run(srcs, x.shape[0], int(shape[0]), int(shape[1]), out_absmax=out_absmax, stats=stats)


# --------------------------------------------------------------------------- S2D
class SparseToDensePool(torch.nn.Module):
    def __init__(self, input_channels, min_pool_sizes=[3, 5, 7, 9], max_pool_sizes=[3, 5, 7, 9],
                 n_filter=8, n_convolution=3, weight_initializer="kaiming_uniform",
                 activation_func="leaky_relu"):
        super().__init__()
        act = activation_func if not isinstance(activation_func, str) else globals()["activation_func"](activation_func)
        self.min_pool_sizes = [s for s in min_pool_sizes if s > 1]
        self.max_pool_sizes = [s for s in max_pool_sizes if s > 1]
        self.len_pool_sizes = len(self.min_pool_sizes) + len(self.max_pool_sizes)
        in_channels = self.len_pool_sizes
        convs = []
        for _ in range(n_convolution):
            convs.append(Conv2d(in_channels, n_filter, kernel_size=1, stride=1,
                                weight_initializer=weight_initializer, activation_func=act))
            in_channels = n_filter
        self.pool_convs = torch.nn.Sequential(*convs)
        self.conv = Conv2d(n_filter + input_channels, n_filter, kernel_size=3, stride=1,
                           weight_initializer=weight_initializer, activation_func=act)
        self._slope = _slope(act)
        # the layers one by one where the fused kernel does not go: no activation / ELU / sigmoid (it is written around max(v, slope v)),
        # more than 8 filters, more than 4 1x1 convs, more than 2 input channels (kbn_s2d_forward's limits, include/kbnet_hip.h)
        # or more than 8 pools
        self.layerwise = self._slope is None or n_filter > 8 or n_convolution > 4 or input_channels > 2 or self.len_pool_sizes > 8

    def forward(self, x):
        if self.layerwise:
            # reference src/networks.py:2168-2196: pyramid -> 1x1 convs -> cat[., x] (two sources of one launch) -> 3x3 conv
            x = x if _dense(x) else x.contiguous()
            n, _, h, w = x.shape
            if self.len_pool_sizes <= 8:
                y = ops.s2d_pyramid(x, self.min_pool_sizes, self.max_pool_sizes)
            else:   # the pyramid kernel holds eight pools: the min pools, then the max pools, eight at a time (channel order as :2170-2189)
                mins, maxs = self.min_pool_sizes, self.max_pool_sizes
                parts = [ops.s2d_pyramid(x, mins[i:i + 8], []) for i in range(0, len(mins), 8)]
                parts += [ops.s2d_pyramid(x, [], maxs[i:i + 8]) for i in range(0, len(maxs), 8)]
                y = torch.cat(parts, dim=1)
            for conv in self.pool_convs:
                y = conv.run([ops.tensor_src(y, "pool")], n, h, w)
            return self.conv.run([ops.tensor_src(y, "pool"), ops.tensor_src(x, "x")], n, h, w)
        return ops.s2d_forward(x, [c.conv.weight for c in self.pool_convs], self.conv.conv.weight,
                               self.min_pool_sizes, self.max_pool_sizes, self._slope)


# ----------------------------------------------------------------------- encoder
class KBNetEncoder(torch.nn.Module):
    """KBNet encoder: KB at level 0, KB or plain VGG blocks at levels 1-3, level 4 plain (the shipped presets) or
    a KB level with the reference's quirk Q3 (block 4 called twice).  Skip tensors are written in place: each KB
    block's conv_fused / conv_depth land in the two channel slices of one buffer, which
    is both the skip connection and the next block's `fused` / `depth` inputs."""

    # conv_image of KB levels 1 and 2 as ops.PairTensor for the next level's split convs (KBN_NO_PAIR=1 / KBN_NO_PAIR_ENC=1: fp32 tensors)
    pair_chain = _KnobSwitch("KBN_NO_PAIR", "KBN_NO_PAIR_ENC")
    # S2D -> conv0_depth -> level-0 conv_depth (+ xyz) as ONE launch (ops.s2d_depth_front, csrc/s2d_stage.h).  OPT-IN
    # (KBN_DEPTH_FRONT_FUSION=1 or `encoder.fuse_s2d = True`): measured inside the forward it is level with the two launches it
    # replaces -- it removes their 0.9 GB HBM round trip of the S2D tensor, not time
    fuse_s2d = _KnobSwitch("KBN_NO_DEPTH_FRONT_FUSION", enable="KBN_DEPTH_FRONT_FUSION")
    # level 1's conv_fused (1x1 stride 2 over cat[conv_image, xyz, conv_fused] of level 0) inside level 0's image launch: the layer
    # reads only the even pixels of the two tensors that launch's lanes hold (ops.kb1_front next_fused; KBN_NO_FRONT_NEXT=1: own launch)
    front_next = _KnobSwitch("KBN_NO_FRONT_NEXT")

    def __init__(self, input_channels_image=3, input_channels_depth=1,
                 n_filters_image=[48, 96, 192, 384, 384], n_filters_depth=[16, 32, 64, 128, 128],
                 n_filters_fused=[48, 96, 192, 384, 384], n_convolutions_image=[1, 1, 1, 1, 1],
                 n_convolutions_depth=[1, 1, 1, 1, 1], n_convolutions_fused=[1, 1, 1, 1, 1],
                 resolutions_backprojection=[0, 1, 2], weight_initializer="kaiming_uniform",
                 activation_func="leaky_relu"):
        super().__init__()
        for lst in (n_convolutions_image, n_convolutions_depth, n_convolutions_fused, n_filters_image,
                    n_filters_depth, n_filters_fused):
            assert len(lst) == 5
        if 0 not in resolutions_backprojection:
            raise ValueError("resolution 0 must use calibrated backprojection (undefined in the reference otherwise)")
        self.resolutions_backprojection = list(resolutions_backprojection)
        act = globals()["activation_func"](activation_func)
        fi, fd, ff = n_filters_image, n_filters_depth, n_filters_fused
        self.conv0_image = Conv2d(input_channels_image, fi[0], 3, 1, weight_initializer, act)
        self.conv0_depth = Conv2d(input_channels_depth, fd[0], 3, 1, weight_initializer, act)
        self.calibrated_backprojection1 = CalibratedBackprojectionBlock(
            fi[0], fd[0], fi[0], fi[0], fd[0], ff[0], n_convolutions_image[0], n_convolutions_depth[0],
            n_convolutions_fused[0], weight_initializer, act)
        for n in (1, 2, 3):
            if n in resolutions_backprojection:
                cf = fi[n - 1] + ff[n - 1] if (n - 1) in resolutions_backprojection else fi[n - 1]
                setattr(self, f"calibrated_backprojection{n + 1}", CalibratedBackprojectionBlock(
                    fi[n - 1], fd[n - 1], cf, fi[n], fd[n], ff[n], n_convolutions_image[n],
                    n_convolutions_depth[n], n_convolutions_fused[n], weight_initializer, act))
            else:
                setattr(self, f"conv{n + 1}_image", VGGNetBlock(fi[n - 1], fi[n], n_convolutions_image[n], 2,
                                                               weight_initializer, act))
                setattr(self, f"conv{n + 1}_depth", VGGNetBlock(fd[n - 1], fd[n], n_convolutions_depth[n], 2,
                                                               weight_initializer, act))
        if 4 in resolutions_backprojection:
            # The reference BUILDS this block (src/networks.py:266-283) and never calls it: its level-4 branch re-uses
            # calibrated_backprojection4 (:512, quirk Q3).  It exists here for the same state_dict; encode() reproduces the quirk.
            cf = fi[3] + ff[3] if 3 in resolutions_backprojection else fi[3]
            self.calibrated_backprojection5 = CalibratedBackprojectionBlock(
                fi[3], fd[3], cf, fi[4], fd[4], ff[4], n_convolutions_image[4], n_convolutions_depth[4],
                n_convolutions_fused[4], weight_initializer, act)
        else:
            self.conv5_image = VGGNetBlock(fi[3], fi[4], n_convolutions_image[4], 2, weight_initializer, act)
            self.conv5_depth = VGGNetBlock(fd[3], fd[4], n_convolutions_depth[4], 2, weight_initializer, act)
        self._f = (list(fi), list(fd), list(ff))
        # conv0_image + the level-0 KB block's conv_image / conv_fused as ONE launch, conv0's output kept on the CU
        # (ops.kb1_front, csrc/kb1_front.hip): KBNet's level 0 (48 / 48 filters) in all presets; other widths keep the
        # separate kernels
        self.front = True
        # OFF by default (the reference computes it): do not launch conv_image of KB level 3, whose output nothing reads
        self.skip_unused_image = False
        self._packed_front = _PackedBlob(ops.pack_kb1_front_weight)
        self._packed_front_next = _PackedBlob(ops.pack_kb1_front_next_weight)
        self._packed_depth_front = _PackedBlob(ops.pack_kb1_depth_front_weight)
        # the blob of the on-chip S2D stage (`fuse_s2d`): KBNetModel.forward hands encode() the S2D module and its input instead of the
        # S2D tensor, and _front decides where the layer runs
        self._packed_s2d_front = _PackedBlob(lambda *ws, out=None: ops.pack_s2d_depth_front_weight(ws[:-1], ws[-1], out=out))

    def _front(self, image, depth, kinv, stats, s2d=None, kinv_next=None):
        """Level 0 with conv0_image / conv0_depth fused in (their outputs stay on the CU): (skip, conv_image, conv_depth,
        conv_fused, amax_image, amax_skip), or None when the shapes are outside ops.kb1_front's (the caller runs the conv0s
        and the block on their own; nothing has been launched then).  `depth`: the S2D output, or None with `s2d` =
        (SparseToDensePool module, its N x 2 x H x W input): the S2D layer then runs inside the depth branch's launch
        (ops.s2d_depth_front) or, where that declines, on its own in front of it.  `kinv_next`: callable giving the level-1 inverse
        intrinsics; when the next level is a KB level of KBNet's widths its conv_fused rides along in the image launch and the tuple
        ends with (its skip tensor, that tensor's absmax slot) instead of None."""
        blk = self.calibrated_backprojection1
        ci, cf, cd = blk.conv_image.conv_block[0], blk.conv_fused, blk.conv_depth.conv_block[0]
        c0 = self.conv0_image
        if (not self.front or not c0.split or not ci.split or c0._slope is None or blk.proj_depth._slope is None
                or cf.in_channels != c0.out_channels + 3 or not _dense(image) or blk.stacked):
            return None
        n, _, h, w = image.shape
        # decided BEFORE anything is launched: a late decline (KBN_NO_SPLIT=1, a slope outside [0, 1], an oversized map) would
        # leave the depth branch's launches below to be repeated by the caller's three-launch path
        if not ops.kb1_front_supported(image.shape[1], c0.out_channels, ci.out_channels, h, w, c0._slope):
            return None
        packed = self._packed_front.get(c0.conv.weight, ci.conv.weight, cf.conv.weight)
        if packed is None:
            return None
        fi, fd, ff = self._f
        oh, ow = (h + 1) // 2, (w + 1) // 2
        dev = image.device
        skip = torch.empty((n, ff[0] + fd[0], oh, ow), device=dev, dtype=torch.float32)
        out_fused, out_depth = skip[:, :ff[0]], skip[:, ff[0]:]
        out_image = torch.empty((n, fi[0], oh, ow), device=dev, dtype=torch.float32)
        a_img, a_skip = stats.new(), stats.new()
        # depth branch: conv0_depth -> conv_depth (+ xyz) in one launch too, or the separate kernels
        c0d = self.conv0_depth
        xyz = None
        depth_front_ok = (c0d.split and cd.split and c0d._slope is not None and (depth is None or _dense(depth))
                          and ops.kb1_front_supported(c0d.in_channels, c0d.out_channels, cd.out_channels, h, w, c0d._slope, depth_branch=True))
        packed_d = self._packed_depth_front.get(c0d.conv.weight, cd.conv.weight, blk.proj_depth.conv.weight) if depth_front_ok else None
        if depth is None:
            s2d_mod, s2d_x = s2d
            if (self.fuse_s2d and packed_d is not None and not s2d_mod.layerwise and s2d_mod._slope is not None
                    and s2d_x.shape[1] == 2 and _dense(s2d_x) and len(s2d_mod.pool_convs) == 3
                    and ops.s2d_depth_front_supported(s2d_x.shape[1], s2d_mod.min_pool_sizes, s2d_mod.max_pool_sizes, len(s2d_mod.pool_convs),
                                                      s2d_mod.conv.out_channels, c0d.out_channels, cd.out_channels, h, w, s2d_mod._slope, c0d._slope)):
                packed_s = self._packed_s2d_front.get(*[c.conv.weight for c in s2d_mod.pool_convs], s2d_mod.conv.conv.weight)
                if packed_s is not None:
                    res = ops.s2d_depth_front(s2d_x, kinv, packed_s, packed_d, s2d_mod.min_pool_sizes, s2d_mod.max_pool_sizes, c0d.out_channels,
                                              cd.out_channels, out_depth, s2d_mod._slope, c0d._slope, blk._slope, blk.proj_depth._slope,
                                              out_depth_absmax=a_skip)
                    if res is None:
                        raise KbnError("s2d_depth_front declined a problem kbn_s2d_depth_front_query accepted")
                    xyz = res[1]
            if xyz is None:
                depth = s2d_mod(s2d_x)   # the S2D tensor after all: its own launch
        if xyz is None and packed_d is not None:
            res = ops.kb1_depth_front(depth, kinv, packed_d, c0d.out_channels, cd.out_channels, out_depth, c0d._slope, blk._slope,
                                      blk.proj_depth._slope, out_depth_absmax=a_skip)
            xyz = res[1] if res is not None else None
        if xyz is None:
            conv_depth0 = c0d(depth)
            xyz = ops.kb_xyz_s2(conv_depth0, blk.proj_depth.conv.weight, kinv, blk.proj_depth._slope)
            cd.run([ops.tensor_src(conv_depth0, "depth"), ops.coords_src(kinv)], n, h, w, out=out_depth, out_absmax=a_skip)
        nxt, nxt_info = None, None
        blk2 = getattr(self, "calibrated_backprojection2", None) if 1 in self.resolutions_backprojection else None
        if (self.front_next and blk2 is not None and kinv_next is not None and not blk2.stacked and blk2.split_image
                and blk2.conv_image.conv_block[0].split
                and blk2.conv_fused.in_channels == ci.out_channels + 3 + cf.out_channels and blk2.proj_depth._slope is not None
                and ops.kb1_front_next_supported(image.shape[1], c0.out_channels, ci.out_channels, blk2.n_filter_fused, h, w, c0._slope)):
            packed_n = self._packed_front_next.get(blk2.conv_fused.conv.weight, image_channels=fi[0])
            if packed_n is not None:
                h2, w2 = (oh + 1) // 2, (ow + 1) // 2
                skip2 = torch.empty((n, ff[1] + fd[1], h2, w2), device=dev, dtype=torch.float32)
                a_skip2 = stats.new()
                xyz2 = ops.kb_xyz_s2(out_depth, blk2.proj_depth.conv.weight, kinv_next(), blk2.proj_depth._slope)
                slope2 = blk2.conv_fused._slope
                nxt = (packed_n, xyz2, skip2[:, :ff[1]], 1.0 if slope2 is None else slope2, a_skip2)
                nxt_info = (skip2, a_skip2)
        if ops.kb1_front(image, packed, xyz, c0.out_channels, ci.out_channels, out_image, out_fused,
                         c0._slope, blk._slope, a_img, a_skip, next_fused=nxt) is None:
            raise KbnError("kb1_front declined a problem kbn_kb1_front_query accepted")
        return skip, out_image, out_depth, out_fused, a_img, a_skip, nxt_info

    def _image_splitk(self, level, h, w):
        """In the latency form: would KB level `level`'s stride-2 image conv (input h x w) launch split-K?"""
        blk = getattr(self, f"calibrated_backprojection{level + 1}", None)
        if blk is None:
            return False
        ci = blk.conv_image.conv_block[0]
        frames = getattr(ci, "latency", 0)
        return bool(frames) and ops.ksplit_for(ci.in_channels, ci.out_channels, (h + 1) // 2, (w + 1) // 2, 2, frames=frames) > 1

    def forward(self, image, depth, intrinsics):
        latent, skips, _, _ = self.encode(image, depth, intrinsics)
        return latent, skips

    def encode(self, image, depth, intrinsics, stats=None, s2d=None):
        """forward() plus the per-frame max |a| slots of what it returns: (latent, skips, amax_latent, amax_skips).  Every
        conv of the encoder folds max |out| into the slot of its output tensor (ops.ActStats); the split-operand convs
        downstream -- here and in the decoder -- place their fp16 windows on them.  `depth` may be None with `s2d` =
        (SparseToDensePool module, its input): the S2D layer is then evaluated here, inside level 0's depth launch where it fits."""
        fi, fd, ff = self._f
        n, _, h0, w0 = image.shape
        if stats is None:
            stats = ops.ActStats(n, image.device)
        dev = image.device
        image = image if _dense(image) else image.contiguous()
        if depth is not None:
            depth = depth if _dense(depth) else depth.contiguous()
        intrinsics = intrinsics.contiguous()

        kinv = ops.intrinsics_inverse(intrinsics, 1.0, 1.0)
        h, w = h0, w0
        h1, w1 = (h0 + 1) // 2, (w0 + 1) // 2
        # Q1: every deeper KB level scales K by the level-1 ratio (reference src/networks.py:342-343)
        sx, sy = w1 / w0, h1 / h0
        kinv1_box = []   # the level-1 inverse serves every deeper level (Q1): computed once, by whoever needs it first

        def kinv1_get():
            if not kinv1_box:
                kinv1_box.append(ops.intrinsics_inverse(intrinsics, sx, sy))
            return kinv1_box[0]

        front = self._front(image, depth, kinv, stats, s2d, kinv_next=kinv1_get) if 0 in self.resolutions_backprojection else None
        if front is None:
            if depth is None:
                depth = s2d[0](s2d[1])
            conv_image = self.conv0_image(image)
            conv_depth = self.conv0_depth(depth)
        conv_fused = None
        skips, amax_skips = [], []
        amax_image = amax_skip = None   # slots of the current conv_image tensor / of the previous level's skip tensor
        next_done = None                # (skip tensor, slot) of level 1 when level 0's launch already wrote its conv_fused
        for level in range(4):
            oh, ow = (h + 1) // 2, (w + 1) // 2
            a_img, a_skip = stats.new(), stats.new()
            if level == 0 and front is not None:
                skip, conv_image, conv_depth, conv_fused, amax_image, a_skip, next_done = front
            elif level in self.resolutions_backprojection:
                blk = getattr(self, f"calibrated_backprojection{level + 1}")
                if level > 0:
                    kinv = kinv1_get()
                fused_done = level == 1 and next_done is not None
                if fused_done:
                    skip, a_skip = next_done
                else:
                    skip = torch.empty((n, ff[level] + fd[level], oh, ow), device=dev, dtype=torch.float32)
                out_fused, out_depth = skip[:, :ff[level]], skip[:, ff[level]:]
                # the image branch of the last KB level in front of a plain level 4 feeds nothing (reference
                # src/networks.py:475-523: conv5_image reads conv4_fused, conv4_image only lends its shape)
                unused = self.skip_unused_image and level == 3 and 4 not in self.resolutions_backprojection
                # conv_image of a KB level is read by the next KB level only -- its stride-2 split conv_image and, at the even
                # pixels, its conv_fused: it travels as an ops.PairTensor (+ the fp32 even-pixel side output) from level 1 on
                want_pair = self.pair_chain and 1 <= level < 3 and (level + 1) in self.resolutions_backprojection
                if want_pair and self._image_splitk(level + 1, oh, ow):
                    want_pair = False   # the latency form: the next level's image conv runs split-K, on an fp32 source
                res = None
                if want_pair or isinstance(conv_image, ops.PairTensor):
                    res = blk.run(conv_image, conv_depth, kinv, conv_fused, None, out_depth, out_fused,
                                  amax_image=amax_image, amax_fused=amax_skip if conv_fused is not None else None,
                                  out_amax_image=a_img, out_amax_skip=a_skip, stats=stats, need_image=not unused,
                                  pair_image_out=want_pair, fused_done=fused_done)
                if res is None:
                    if isinstance(conv_image, ops.PairTensor):   # a pair tensor the next level declined: decode it (rare, not fast)
                        conv_image, amax_image = conv_image.float(), None
                    res = blk.run(
                        conv_image, conv_depth, kinv, conv_fused, None, out_depth, out_fused,
                        amax_image=amax_image if level > 0 else None, amax_fused=amax_skip if conv_fused is not None else None,
                        out_amax_image=a_img, out_amax_skip=a_skip, stats=stats, need_image=not unused, fused_done=fused_done)
                conv_image, conv_depth, conv_fused = res
                amax_image = a_img
            else:
                # plain level: conv_image lives in the skip tensor, whose slot (a superset: a safe bound) serves it too
                src, a_src = (conv_fused, amax_skip) if conv_fused is not None else (conv_image, amax_image if level > 0 else None)
                skip = torch.empty((n, fi[level] + fd[level], oh, ow), device=dev, dtype=torch.float32)
                ci_blk = getattr(self, f"conv{level + 1}_image")
                cd_blk = getattr(self, f"conv{level + 1}_depth")
                branch = _SideBranch(dev)
                conv_image = ci_blk.run([ops.tensor_src(src, "image", a_src)], n, h, w, out=skip[:, :fi[level]], out_absmax=a_skip,
                                        stats=stats)
                with branch:
                    conv_depth = cd_blk.run([ops.tensor_src(conv_depth, "depth", amax_skip)], n, h, w, out=skip[:, fi[level]:],
                                            out_absmax=a_skip, stats=stats)
                conv_fused = None
                amax_image = a_skip
            amax_skip = a_skip
            skips.append(skip)
            amax_skips.append(a_skip)
            h, w = oh, ow
        oh, ow = (h + 1) // 2, (w + 1) // 2
        amax_latent = stats.new()
        if 4 in self.resolutions_backprojection:
            # Quirk Q3 (reference src/networks.py:499-517): the level-4 branch calls calibrated_backprojection4 -- level 3's block --
            # a second time, on level 3's outputs, with the level-1-ratio intrinsics of every deeper level (Q1); the block built as
            # calibrated_backprojection5 stays unused.  Like the reference this needs a KB layer at level 3 and levels 2 and 3 of
            # equal width (the block's channel check raises otherwise, where the reference raises a shape error); latent =
            # cat[conv5_fused, conv5_depth] then carries block 4's filter counts.
            if 3 not in self.resolutions_backprojection:
                raise AttributeError("'KBNetEncoder' object has no attribute 'calibrated_backprojection4'")   # as in the reference
            blk = self.calibrated_backprojection4
            if isinstance(conv_image, ops.PairTensor):
                conv_image, amax_image = conv_image.float(), None
            latent = torch.empty((n, blk.n_filter_fused + blk.n_filter_depth, oh, ow), device=dev, dtype=torch.float32)
            blk.run(conv_image, conv_depth, kinv1_get(), conv_fused, None, latent[:, blk.n_filter_fused:], latent[:, :blk.n_filter_fused],
                    amax_image=amax_image, amax_fused=amax_skip if conv_fused is not None else None, out_amax_image=stats.new(),
                    out_amax_skip=amax_latent, stats=stats, need_image=not self.skip_unused_image)
            return latent, skips, amax_latent, amax_skips
        latent = torch.empty((n, fi[4] + fd[4], oh, ow), device=dev, dtype=torch.float32)
        src, a_src = (conv_fused, amax_skip) if conv_fused is not None else (conv_image, amax_image)
        branch = _SideBranch(dev)   # the two convs of level 4 are independent
        self.conv5_image.run([ops.tensor_src(src, "image", a_src)], n, h, w, out=latent[:, :fi[4]],
                             out_absmax=amax_latent, stats=stats)
        with branch:
            self.conv5_depth.run([ops.tensor_src(conv_depth, "depth", amax_skip)], n, h, w, out=latent[:, fi[4]:],
                                 out_absmax=amax_latent, stats=stats)
        return latent, skips, amax_latent, amax_skips


# ----------------------------------------------------------------------- decoder
class MultiScaleDecoder(torch.nn.Module):
    """The decoder as KBNet builds it: five 'up' DecoderBlocks, n_resolution=1, linear
    output0.  `forward` returns `[logits]` like the reference (the caller takes [-1])."""

    # deconv4 .. deconv1 hand their concat-conv outputs to the next up-conv as ops.PairTensor (KBN_NO_PAIR=1: fp32 tensors)
    pair_chain = _KnobSwitch("KBN_NO_PAIR")
    pair_tail = _KnobSwitch("KBN_NO_PAIR_TAIL")   # A/B: deconv0's up-conv -> tail tensor as a PairTensor

    def __init__(self, input_channels=256, output_channels=1, n_resolution=1,
                 n_filters=[256, 128, 64, 32, 16], n_skips=[256, 128, 64, 32, 0],
                 weight_initializer="kaiming_uniform", activation_func="leaky_relu",
                 output_func="linear", use_batch_norm=False, use_instance_norm=False, deconv_type="up"):
        super().__init__()
        if n_resolution != 1 or output_func != "linear" or len(n_filters) != 5 or output_channels != 1:
            raise ValueError("implemented for KBNet's decoder: 5 levels, n_resolution=1, linear 1-channel output")
        if use_batch_norm or use_instance_norm:
            raise ValueError("normalisation layers are not part of the KBNet inference path")
        self.n_resolution = n_resolution
        self.output_func = output_func
        act = globals()["activation_func"](activation_func)
        cin = input_channels
        for i, name in enumerate(("deconv4", "deconv3", "deconv2", "deconv1", "deconv0")):
            setattr(self, name, DecoderBlock(cin, n_skips[i], n_filters[i], weight_initializer, act,
                                             deconv_type=deconv_type))
            cin = n_filters[i]
        self.output0 = Conv2d(n_filters[4], output_channels, 3, 1, weight_initializer, None)
        self._packed_tail = _PackedBlob(ops.pack_conv_tail_weight)

    def features(self, x, skips, shape):
        """Everything up to (not including) output0."""
        stats = ops.ActStats(x.shape[0], x.device)
        x, amax = self.features_level1(x, skips, stats=stats)
        return self.deconv0(x, None, shape=tuple(shape)[-2:], amax_x=amax, stats=stats)

    def features_level1(self, x, skips, amax_x=None, amax_skips=None, stats=None, allow_pair=False):
        """deconv4 .. deconv1: the half-resolution features deconv0 starts from, and their per-frame max |a| slot.
        amax_x / amax_skips: the slots of the latent / the skip tensors (KBNetEncoder.encode); missing ones are measured.
        `allow_pair`: the result may be an ops.PairTensor (depth() hands it to deconv0's up-conv)."""
        if stats is None:
            stats = ops.ActStats(x.shape[0], x.device)
        amax_skips = amax_skips if amax_skips is not None else [None] * 4
        amax = amax_x
        for blk, i in ((self.deconv4, 3), (self.deconv3, 2), (self.deconv2, 1), (self.deconv1, 0)):
            a_out = stats.new()
            # the concat conv's output is read by the next block's up-conv only: as a PairTensor when that kernel takes one
            y = None
            # the latency form: a block whose up-conv or concat conv would run split-K takes and returns fp32 tensors (the split-K
            # kernels read fp32 sources); the pair chain starts behind the last such block
            if not isinstance(x, ops.PairTensor) and blk.latency_splitk(x.shape[2], x.shape[3]):
                y = blk(x, skips[i], amax_x=amax, amax_skip=amax_skips[i], out_absmax=a_out, stats=stats)
            # (not with KBN_NO_SPLIT=1: every split-operand launch would decline, after the block's up-conv had already run in fp32)
            if y is None and self.pair_chain and (allow_pair or i > 0) and ops.split_enabled():
                y = blk(x, skips[i], amax_x=amax, amax_skip=amax_skips[i], out_absmax=a_out, stats=stats, pair_out=True)
            if y is None and isinstance(x, ops.PairTensor):
                # a pair tensor in, an fp32 tensor out (the block's up-conv stages the pair source by DMA, mode "pair in /
                # fp32 out"): the last block of features() / forward(), where the caller wants fp32
                y = blk(x, skips[i], amax_x=amax, amax_skip=amax_skips[i], out_absmax=a_out, stats=stats)
                if y is None:
                    x = x.float()   # a shape the pair kernels declined after one of them produced x: rare, not fast
                    amax = None
            if y is None:
                y = blk(x, skips[i], amax_x=amax, amax_skip=amax_skips[i], out_absmax=a_out, stats=stats)
            x = y
            amax = a_out
        return x, amax

    def depth(self, x, skips, shape, min_predict_depth, max_predict_depth, return_logits=False, out=None,
              amax_x=None, amax_skips=None, stats=None):
        """The whole decoder + KBNetModel.forward's depth mapping (reference src/kbnet_model.py:179-184).  deconv0's
        second conv, output0 and the sigmoid mapping run as ONE kernel when deconv0 has no skip and its width is a
        multiple of 4 channels (KBNet: 12); otherwise conv, then the fused output0 + mapping head."""
        if stats is None:
            stats = ops.ActStats(x.shape[0], x.device)
        d0 = self.deconv0
        x, amax = self.features_level1(x, skips, amax_x, amax_skips, stats, allow_pair=d0.skip_channels == 0)
        if d0.skip_channels == 0:
            packed = self._packed_tail.get(d0.conv.conv.weight) if (d0.conv.split and d0.conv._post is None) else None
            up = None
            if packed is not None and self.pair_tail and self.pair_chain and d0.conv.out_channels <= 12:
                # deconv0's up-conv hands the tail a PairTensor too (16 channels for KBNet's 12)
                up = d0.deconv(x, shape=tuple(shape)[-2:], amax=amax, stats=stats, pair_out=True)
                if up is not None:
                    res = ops.conv_tail(up, packed, self.output0.conv.weight, min_predict_depth, max_predict_depth, d0.conv._slope,
                                        return_logits=return_logits, out=out)
                    if res is not None:
                        return res
                    up = up.float()[:, :d0.conv.out_channels].contiguous()   # the tail declined it: decode (rare, not fast)
            if up is None:
                up = d0.deconv(x, shape=tuple(shape)[-2:], amax=amax, stats=stats)
            if up is None:   # deconv0's up-conv declined the pair tensor
                up = d0.deconv(x.float(), shape=tuple(shape)[-2:], amax=None, stats=stats)
            if packed is not None:   # the 12 -> 12 conv of the tail on split fp16 operands (csrc/tail.hip)
                res = ops.conv_tail(up, packed, self.output0.conv.weight, min_predict_depth,
                                    max_predict_depth, d0.conv._slope, return_logits=return_logits, out=out)
                if res is not None:
                    return res
            if d0.conv._post is None:   # (an ELU / sigmoid conv runs on its own, then the output0 + mapping head)
                res = ops.conv_head(up, d0.conv.conv.weight, self.output0.conv.weight, min_predict_depth,
                                    max_predict_depth, d0.conv._slope, return_logits=return_logits, out=out)
                if res is not None:
                    return res
            feats = d0.conv.run([ops.tensor_src(up, "deconv")], up.shape[0], up.shape[2], up.shape[3])
        else:
            feats = d0(x, None, shape=tuple(shape)[-2:], amax_x=amax, stats=stats)
        return ops.depth_head(feats, self.output0.conv.weight, min_predict_depth, max_predict_depth,
                              return_logits=return_logits, out=out)

    def forward(self, x, skips, shape=None):
        return [self.output0(self.features(x, skips, shape))]


# ------------------------------------------------------------------------- model
def paired_planes(first, second):
    """The N x 2 x H x W tensor whose channel 0 is `first` and channel 1 is `second` when the two N x 1 x H x W fp32 tensors
    ARE the two planes of one such buffer (`second`'s planes directly behind `first`'s, frame by frame) -- what
    `new_depth_input_pair` hands out; None otherwise.  KBNetModel.forward uses it to skip the reference's
    torch.cat([sparse_depth, validity_map_depth]) (a copy of both planes per call)."""
    if (first.dim() != 4 or first.shape != second.shape or first.shape[1] != 1 or first.dtype != torch.float32
            or second.dtype != torch.float32 or first.device != second.device):
        return None
    n, _, h, w = first.shape
    hw = h * w
    if (first.stride()[2:] != (w, 1) or second.stride()[2:] != (w, 1) or second.data_ptr() != first.data_ptr() + 4 * hw
            or (n > 1 and (first.stride(0) != 2 * hw or second.stride(0) != 2 * hw))
            or first.untyped_storage().data_ptr() != second.untyped_storage().data_ptr()):
        return None
    return torch.as_strided(first, (n, 2, h, w), (2 * hw, hw, w, 1))


def new_depth_input_pair(n, height, width, device):
    """(sparse_depth, validity_map_depth): N x 1 x H x W views of ONE N x 2 x H x W buffer, the layout S2D reads directly.
    An input pipeline that writes its sparse depth and validity map here saves the concatenation of every forward."""
    pair = torch.empty((n, 2, height, width), device=device, dtype=torch.float32)
    return pair[:, 0:1], pair[:, 1:2]


# Stream capture in THREAD-LOCAL error mode: under the default ("global") mode a HIP call that is illegal during capture fails the capture
# when ANY thread makes it -- and ProcessGroupNCCL's watchdog thread polls the events of recent collectives (hipEventQuery) all the time.
# A capture() after the first all-gather of a process (bench.py's side legs, the mixed-shape stream, a second batch shape) then died one
# run in four with "operation not permitted when stream is capturing" thrown on the WATCHDOG thread, which terminates the process
# (round 6, profiles/r06/v99_rccl_child_failure.err).  Nothing on the capturing thread needs the global check.
_CAPTURE_MODE = "thread_local"


class GraphedForward:
    """HIP-graph replay of `KBNetModel.forward` for a fixed batch shape (torch.cuda.CUDAGraph is
    the plumbing: capture, private memory pool, replay; every node is one of our kernels or a
    torch copy).

    `branches` > 1 captures the batch as that many equal sub-batches on concurrent branches of the graph
    (frames are independent): while one branch's kernel drains its last, partly filled round of
    workgroups, the other branch's kernel already runs -- +4 % at 2 x 4 KITTI frames, bit-identical
    output.  Default: 2 branches for even batches of at least 4 frames, otherwise 1.

    `outputs` = 2 captures the graph TWICE, each copy writing its own output tensor (one memory pool: the activations are
    shared, only the N x 1 x H x W result exists twice), and calls alternate between them (`rotating_outputs`): the tensor a
    call returns stays untouched until the next-but-one call, so an asynchronous consumer -- the all-gather of
    dist.ShardedRunner.step_pipelined, in flight under the next step's forward -- reads it in place instead of from a copy.

    `split_graphs` (with branches > 1): ONE GRAPH PER SUB-BATCH instead of one graph that forks -- a replay launches them on
    concurrent streams and joins.  A fork inside a forked capture crashes hipStreamEndCapture on ROCm 7.2, which keeps the
    per-level side branches (conv_depth / conv_fused of a KB level beside its conv_image: _SideBranch) off inside a forking graph;
    a graph of its own per sub-batch forks only once, so both kinds of concurrency run together.  Same bits either way."""

    def __init__(self, model, image, sparse_depth, validity_map_depth, intrinsics, branches=None, tune=True, outputs=1,
                 split_graphs=False):
        # the static sparse depth / validity inputs are the two planes of one buffer (paired_planes: no torch.cat in the graph)
        sd, vm = new_depth_input_pair(sparse_depth.shape[0], sparse_depth.shape[2], sparse_depth.shape[3], sparse_depth.device)
        sd.copy_(sparse_depth)
        vm.copy_(validity_map_depth)
        self.static_in = [image.clone(), sd, vm, intrinsics.clone()]
        n = self.static_in[0].shape[0]
        if branches is None:
            branches = 2 if (n >= 4 and n % 2 == 0) else 1
        if branches < 1 or n % branches != 0:
            raise KbnError(f"cannot split a batch of {n} frames into {branches} equal branches")
        if outputs not in (1, 2):
            raise KbnError(f"outputs must be 1 or 2, got {outputs}")
        per = n // branches
        parts = [[t[i * per:(i + 1) * per] for t in self.static_in] for i in range(branches)]
        self.model = model
        self.rotating_outputs = outputs if outputs > 1 else 0
        self.split_graphs = bool(split_graphs) and branches > 1
        self._turn = 0
        dev = self.static_in[0].device
        with torch.cuda.device(dev):
            self._capture(model, parts, branches, per, n, tune, outputs)

    def _capture(self, model, parts, branches, per, n, tune, outputs=1):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        # warm-up on a side stream: packs weights, sets kernel attributes and -- the one place the host mirror
        # opts in to it -- tunes launch geometry for this batch shape (ops.autotune; ABI calls never tune on their own)
        with torch.cuda.stream(side), ops.autotune(bool(tune)):
            for _ in range(2):
                model.forward(*parts[0])
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self._weights = model.weight_state()
        self.branches = branches
        self._streams = [torch.cuda.Stream() for _ in range(branches - 1)]
        # The output tensors live OUTSIDE the graphs' memory pool (allocated here, before any capture): a second capture that
        # shares the first one's pool may hand out memory the first capture's tensors occupy -- its activations on purpose, but an
        # output tensor allocated under capture went the same way on ROCm 7.2 (both copies returned one address).
        h, w = self.static_in[1].shape[-2:]
        self.graphs = []
        self.static_outs = [torch.empty((n, 1, h, w), device=self.static_in[0].device, dtype=torch.float32) for _ in range(outputs)]
        for k in range(outputs):
            if self.split_graphs:
                # one graph per sub-batch (each with its own pool: they replay concurrently; copy k shares copy 0's pool of the same branch)
                row = []
                for i in range(branches):
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, pool=self.graphs[0][i].pool() if self.graphs else None, capture_error_mode=_CAPTURE_MODE):
                        model.forward(*parts[i], out=self.static_outs[k][i * per:(i + 1) * per])
                    row.append(g)
                self.graphs.append(row)
                continue
            graph = torch.cuda.CUDAGraph()
            # one memory pool for all copies: they replay one after the other on one stream, never concurrently
            with torch.cuda.graph(graph, pool=self.graphs[0].pool() if self.graphs else None, capture_error_mode=_CAPTURE_MODE):
                self._record(model, parts, branches, per, self.static_outs[k])
            self.graphs.append(graph)
        self.graph, self.static_out = self.graphs[0], self.static_outs[0]

    def _record(self, model, parts, branches, per, static_out):
        """The launches of one forward into `static_out`, issued under capture."""
        if branches == 1:
            model.forward(*self.static_in, out=static_out)
            return static_out
        cur = torch.cuda.current_stream()
        # a fork inside a forked branch (and any wait between two forked streams) crashes hipStreamEndCapture on
        # ROCm 7.2 (tools/probe/fork_capture_bisect.py), and forking only the capturing stream's sub-batch measured no
        # gain (2795-2812 vs 2816-2845 frames/s): the per-level side branches stay off under sub-batch branches
        _SideBranch.only_from = 0
        try:
            for s in self._streams:
                s.wait_stream(cur)
            for i, s in enumerate(self._streams):   # every branch writes its frames of the one output tensor
                with torch.cuda.stream(s):
                    model.forward(*parts[i + 1], out=static_out[(i + 1) * per:(i + 2) * per])
            model.forward(*parts[0], out=static_out[0:per])
            for s in self._streams:
                cur.wait_stream(s)
        finally:
            _SideBranch.only_from = None
        return static_out

    def next_output(self):
        """The tensor the NEXT call will write (and return): with two rotating outputs, what an asynchronous reader of an earlier
        result has to be done with before that call (dist.ShardedRunner.step_pipelined asks)."""
        return self.static_outs[self._turn]

    def __call__(self, image, sparse_depth, validity_map_depth, intrinsics):
        with torch.cuda.device(self.static_out.device):
            return self._replay(image, sparse_depth, validity_map_depth, intrinsics)

    def _replay(self, image, sparse_depth, validity_map_depth, intrinsics):
        state = self.model.weight_state()
        if state != self._weights:
            # The graph holds raw device pointers: to the parameters (S2D, proj_depth and the head read them
            # directly) and to the packed blobs.  In-place updates (load_state_dict, restore_model, copy_) keep
            # the parameter storage; the blobs are re-packed in place here, ahead of the replay on this stream.
            if [p for p, _ in state] != [p for p, _ in self._weights]:
                raise KbnError("a parameter's storage moved after capture() (e.g. .to() or a re-assignment): "
                               "call capture() again")
            self.model.refresh_packed()
            self._weights = state
        for dst, src in zip(self.static_in, (image, sparse_depth, validity_map_depth, intrinsics)):
            if dst.data_ptr() != src.data_ptr():
                dst.copy_(src)
        k = self._turn
        self._turn = (k + 1) % len(self.graphs)
        if self.split_graphs:
            cur = torch.cuda.current_stream()
            for st in self._streams:
                st.wait_stream(cur)
            for i, st in enumerate(self._streams):
                with torch.cuda.stream(st):
                    self.graphs[k][i + 1].replay()
            self.graphs[k][0].replay()
            for st in self._streams:
                cur.wait_stream(st)
        else:
            self.graphs[k].replay()
        return self.static_outs[k]


class KBNetModel(object):
    """Inference counterpart of reference `KBNetModel` (src/kbnet_model.py:24-186): same
    constructor arguments and `forward(image, sparse_depth, validity_map_depth, intrinsics)`.
    One process drives one GPU; multi-GPU runs shard frames across processes (dist.py)
    instead of wrapping modules in DataParallel."""

    def __init__(self, input_channels_image, input_channels_depth, min_pool_sizes_sparse_to_dense_pool,
                 max_pool_sizes_sparse_to_dense_pool, n_convolution_sparse_to_dense_pool,
                 n_filter_sparse_to_dense_pool, n_filters_encoder_image, n_filters_encoder_depth,
                 resolutions_backprojection, n_filters_decoder, deconv_type="up",
                 weight_initializer="xavier_normal", activation_func="leaky_relu",
                 min_predict_depth=1.5, max_predict_depth=100.0, device=torch.device("cuda"), trainable: bool = False):
        # `trainable` (extension): the model gets its backward pass -- with grad mode on and a parameter that requires grad, forward
        # runs layer by layer and records autograd (kbnet_train.py); what that path does not differentiate is refused here
        self._has_backward = bool(trainable)
        if trainable:
            kbnet_train.check(deconv_type, activation_func)
        self.min_predict_depth = min_predict_depth
        self.max_predict_depth = max_predict_depth
        self.device = device
        self.sparse_to_dense_pool = SparseToDensePool(
            input_channels=input_channels_depth, min_pool_sizes=min_pool_sizes_sparse_to_dense_pool,
            max_pool_sizes=max_pool_sizes_sparse_to_dense_pool, n_convolution=n_convolution_sparse_to_dense_pool,
            n_filter=n_filter_sparse_to_dense_pool, weight_initializer=weight_initializer,
            activation_func=activation_func)
        n_filters_encoder = [i + z for i, z in zip(n_filters_encoder_image, n_filters_encoder_depth)]
        n_skips = n_filters_encoder[:-1][::-1] + [0]
        self.encoder = KBNetEncoder(
            input_channels_image=input_channels_image, input_channels_depth=n_filter_sparse_to_dense_pool,
            n_filters_image=list(n_filters_encoder_image), n_filters_depth=list(n_filters_encoder_depth),
            n_filters_fused=list(n_filters_encoder_image), resolutions_backprojection=list(resolutions_backprojection),
            weight_initializer=weight_initializer, activation_func=activation_func)
        self.decoder = MultiScaleDecoder(
            input_channels=n_filters_encoder[-1], output_channels=1, n_resolution=1,
            n_filters=list(n_filters_decoder), n_skips=n_skips, weight_initializer=weight_initializer,
            activation_func=activation_func, output_func="linear", use_batch_norm=False, deconv_type=deconv_type)
        self.to(device)
        self.eval()

    @classmethod
    def from_config(cls, cfg: KBNetConfig, device=torch.device("cuda"), trainable: bool = False):
        return cls(cfg.input_channels_image, cfg.input_channels_depth,
                   list(cfg.min_pool_sizes_sparse_to_dense_pool), list(cfg.max_pool_sizes_sparse_to_dense_pool),
                   cfg.n_convolution_sparse_to_dense_pool, cfg.n_filter_sparse_to_dense_pool,
                   list(cfg.n_filters_encoder_image), list(cfg.n_filters_encoder_depth),
                   list(cfg.resolutions_backprojection), list(cfg.n_filters_decoder), cfg.deconv_type,
                   cfg.weight_initializer, cfg.activation_func, cfg.min_predict_depth, cfg.max_predict_depth,
                   device, trainable)

    # -- forward ---------------------------------------------------------------
    def forward(self, image, sparse_depth, validity_map_depth, intrinsics, return_logits=False, out=None, return_inner=False):
        """`out` (extension): write the N x 1 x H x W depth map into this tensor instead of a new one.

        Built with trainable=True, with grad mode on and a parameter that requires grad the depth carries a grad_fn: the network
        runs layer by layer and records autograd (kbnet_train.forward_recorded); `out` and `return_logits` are refused there and
        `return_inner` adds the dict name -> activation of every layer.  Otherwise this is the fused forward, nothing recorded."""
        if self._has_backward and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            if out is not None or return_logits:
                raise KbnError("KBNetModel.forward: out= and return_logits exist on the fused forward only; this call is recorded for "
                               "autograd (run it under torch.no_grad(), or requires_grad_(False))")
            return kbnet_train.forward_recorded(self, image, sparse_depth, validity_map_depth, intrinsics, return_inner=return_inner)
        if return_inner:
            raise KbnError("KBNetModel.forward: return_inner exists on the recorded path only (trainable=True, grad mode on, a parameter "
                           "that requires grad): the fused forward never materialises most activations")
        return self._forward_fused(image, sparse_depth, validity_map_depth, intrinsics, return_logits, out)

    @torch.no_grad()
    def _forward_fused(self, image, sparse_depth, validity_map_depth, intrinsics, return_logits=False, out=None):
        if out is not None and return_logits:
            raise KbnError("out= and return_logits are mutually exclusive")
        input_depth = paired_planes(sparse_depth, validity_map_depth)   # the two planes of one N x 2 x H x W buffer: no copy
        if input_depth is None:
            input_depth = torch.cat([sparse_depth, validity_map_depth], dim=1)   # reference src/kbnet_model.py:161
        shape = input_depth.shape[-2:]
        # per-frame max |a| of every activation tensor, kept on the device: the split-operand convs place their fp16
        # windows on the data of THIS call (no calibration state, no host round trip; ops.ActStats)
        stats = ops.ActStats(image.shape[0], image.device)
        # the S2D layer (reference src/kbnet_model.py:163) runs inside the encoder's first depth launch where the shapes fit
        # (KBNetEncoder._front: S2D -> conv0_depth -> level-0 conv_depth in one kernel), otherwise as its own launch in front of it
        latent, skips, amax_latent, amax_skips = self.encoder.encode(image, None, intrinsics, stats,
                                                                     s2d=(self.sparse_to_dense_pool, input_depth.contiguous()))
        # decoder; its tail (deconv0's second conv + output0 + sigmoid + d_min / (s + d_min/d_max)) is one kernel
        return self.decoder.depth(latent, skips, shape, self.min_predict_depth, self.max_predict_depth,
                                  return_logits=return_logits, out=out, amax_x=amax_latent, amax_skips=amax_skips, stats=stats)

    def set_latency_mode(self, enabled: bool = True, frames: int = 1):
        """The LATENCY form of the forward, for launches of a few frames (the reference's own run loop is batch 1: src/kbnet.py:764-772,
        887).  One KITTI frame gives the low-resolution layers 6-30 workgroups for 256 CUs -- deconv4's conv runs 24 workgroups of 48
        K-chunks each -- so every split-operand 3x3 conv whose launch of `frames` frames cannot fill half the chip spreads each tile's K
        loop over up to 16 workgroups and a second kernel adds the partial sums (kbn_conv3x3_split_forward_ksplit, ops.ksplit_for).  The
        split-K kernels read and write fp32 tensors, so the decoder blocks / KB levels that use them leave the pair-tensor chains; the
        chains start behind the last of them.  `frames`: the frames ONE LAUNCH carries -- 1 for the run loop (and for batch 2), 4 for a
        batch-8 graph (two branches of four frames) -- a property of the mode, not read off the tensors, so that inside a mode a frame's
        bits do not depend on how it is run (eager = graph replay = alone or in a batch).  Same 1e-4 parity as the default form, ANOTHER
        summation order.  Off by default; from 16 frames per launch on no layer qualifies any more."""
        frames = int(frames) if enabled else 0
        if enabled and frames < 1:
            raise KbnError("set_latency_mode: frames must be at least 1")
        for top in self.modules():
            for m in top.modules():
                if isinstance(m, (Conv2d, TransposeConv2d)):
                    m.latency = frames
        self.latency_mode = frames
        return self

    def capture(self, image, sparse_depth, validity_map_depth, intrinsics, branches=None, tune=True, outputs=1, split_graphs=False):
        """Captures one forward of this batch shape into a HIP graph and returns a callable
        `replay(image, sparse_depth, validity_map_depth, intrinsics) -> depth` (inputs are copied
        into the graph's static buffers unless they ARE those buffers; the output tensor is
        re-used between replays).  Removes the ~35 per-launch host round trips of a forward.
        `tune`: time candidate launch geometries during the warm-up (results are bit-identical either way).
        `outputs` = 2: two alternating output tensors (GraphedForward: what dist.ShardedRunner.step_pipelined gathers in place)."""
        return GraphedForward(self, image, sparse_depth, validity_map_depth, intrinsics, branches, tune, outputs, split_graphs)

    def weight_state(self):
        """(storage pointer, version) of every parameter: what a captured graph depends on."""
        return [(p.data_ptr(), p._version) for p in self.parameters()]

    def refresh_packed(self):
        """Re-packs (in place) the MFMA-ordered blobs of weights that changed since they were packed."""
        for blob in packed_blobs(self):
            blob.refresh()

    # -- nn.Module-like plumbing the reference driver uses ------------------------
    def modules(self):
        return (self.sparse_to_dense_pool, self.encoder, self.decoder)

    def parameters(self):
        return [p for m in self.modules() for p in m.parameters()]

    def requires_grad_(self, flag: bool = True):
        """Sets requires_grad on every parameter; True needs a model built with trainable=True."""
        if flag and not self._has_backward:
            raise KbnError("KBNetModel.requires_grad_: this model was built without a backward pass (trainable=True builds one)")
        for p in self.parameters():
            p.requires_grad_(bool(flag))
        return self

    def train(self):
        raise KbnError("the HIP path is inference only")

    def eval(self):
        for m in self.modules():
            m.eval()

    def to(self, device):
        for m in self.modules():
            m.to(device)
        self.device = device

    def data_parallel(self):
        """Reference src/kbnet_model.py:408-415 wraps its three sub-networks in torch.nn.DataParallel (one process, replicas fed by
        threads, weights re-broadcast every forward).  Here the batch splits across GPUs as ONE PROCESS PER GPU (dist.ShardedRunner:
        frames sharded, weights resident, one RCCL all-gather of the outputs), so this call -- the reference's constructor makes it --
        has nothing to wrap and changes nothing; checkpoints still carry the `module.` prefix its wrappers produce (save_model)."""
        return self

    def compute_loss(self, image0=None, image1=None, image2=None, output_depth0=None, sparse_depth0=None, validity_map_depth0=None,
                     intrinsics=None, pose01=None, pose02=None, w_color=0.15, w_structure=0.95, w_sparse_depth=0.60, w_smoothness=0.04):
        """The reference's objective (src/kbnet_model.py:188-304): warp image1 / image2 into image0's view with the predicted depth
        and the relative poses, then colour L1 + SSIM + sparse-depth L1 + edge-aware smoothness -- a quality score that needs no
        ground truth, and a loss to train against.  Returns (loss, loss_info) with the reference's keys (0-dim fp32 tensors and the
        two warped images), plus loss_info['per_frame']: N x 4 fp64, the (colour, structure, sparse depth, smoothness) of each frame.
        One kernel launch (ops.photometric_loss) and a few scalar torch ops on its N x 8 sums; nothing synchronises with the host.
        A frame without a valid sparse point makes the sparse-depth term (and the loss) NaN, as in the reference.

        Differentiable with respect to output_depth0, pose01 and pose02, what the reference trains through: `loss.backward()` is one
        more launch (ops.photometric_loss_backward) and nothing image-sized is kept for it beyond the inputs themselves.  The
        gradient reaches whatever torch graph produced the depth and the poses (ops.pose_matrix included).  The images, the sparse
        depth, the validity map and the intrinsics are data: one that requires grad raises KbnError.  The warped images in loss_info
        are for logging and carry no gradient (the reference's do; nothing trains through them).  No double backward."""
        given = {"image0": image0, "image1": image1, "image2": image2, "output_depth0": output_depth0, "sparse_depth0": sparse_depth0,
                 "validity_map_depth0": validity_map_depth0, "intrinsics": intrinsics, "pose01": pose01, "pose02": pose02}
        missing = [k for k, v in given.items() if v is None]
        if missing:
            raise KbnError("compute_loss: missing " + ", ".join(missing) + " (reference src/kbnet_model.py:188-201)")
        sums, image01, image02 = ops.photometric_loss(image0, image1, image2, output_depth0, sparse_depth0, validity_map_depth0,
                                                      intrinsics, pose01, pose02, return_images=True)
        per_frame = ops.loss_terms(sums, image0.shape[2], image0.shape[3])
        color, structure, sparse, smooth = per_frame.mean(dim=0).float().unbind(0)
        loss = w_color * color + w_structure * structure + w_sparse_depth * sparse + w_smoothness * smooth
        return loss, {"loss_color": color, "loss_structure": structure, "loss_sparse_depth": sparse, "loss_smoothness": smooth,
                      "loss": loss, "image01": image01, "image02": image02, "per_frame": per_frame}

    def log_summary(self, summary_writer, tag, step, image0=None, image01=None, image02=None, output_depth0=None, sparse_depth0=None,
                    validity_map0=None, ground_truth0=None, pose01=None, pose02=None, scalars={}, n_display=4):
        """The reference's log_summary (src/kbnet_model.py:417-650), same signature and defaults: the same add_histogram, add_scalar
        and add_image calls on `summary_writer` (any object with those three methods; TensorBoard itself stays outside the package),
        with the same tag strings, in the same order.  The two image panels -- inputs beside their colourised errors, a column a
        frame -- are written by one kernel launch each (ops.summary_image_panel, ops.summary_depth_panel) and handed over as
        3 x Hg x Wg device tensors; the reference builds them on the host through matplotlib and torchvision.  See summary.py."""
        summary.log_summary(self.max_predict_depth, summary_writer, tag, step, image0=image0, image01=image01, image02=image02,
                            output_depth0=output_depth0, sparse_depth0=sparse_depth0, validity_map0=validity_map0,
                            ground_truth0=ground_truth0, pose01=pose01, pose02=pose02, scalars=scalars, n_display=n_display)

    def load_state_dicts(self, sd_s2d, sd_encoder, sd_decoder):
        """Accepts keys with or without the DataParallel `module.` prefix."""
        for m, sd in zip(self.modules(), (sd_s2d, sd_encoder, sd_decoder)):
            sd = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}
            m.load_state_dict(sd, strict=True)

    def restore_model(self, checkpoint_path, optimizer=None):
        """Loads a reference checkpoint (reference src/kbnet_model.py:378-406).  With an `optimizer` (kb.optim.Adam or
        torch.optim.Adam over this model's parameters, and the pose model's if the checkpoint was written with both groups) the
        checkpoint's `optimizer_state_dict` is loaded into it: Adam's moments and step counts resume where they were saved.  An empty
        dict -- what save_model(..., optimizer=None) writes -- leaves the optimizer as it is.  A dict that does not fit the optimizer
        raises what load_state_dict raises (the reference swallows that error, src/kbnet_model.py:400-403, and resumes from zero
        moments without a word)."""
        ckpt = torch.load(checkpoint_path, map_location=self.device)
        self.load_state_dicts(ckpt["sparse_to_dense_pool_state_dict"], ckpt["encoder_state_dict"],
                              ckpt["decoder_state_dict"])
        optim.load_checkpoint_state(optimizer, ckpt)
        return ckpt.get("train_step", 0), optimizer

    def save_model(self, checkpoint_path, step=0, optimizer=None):
        """Writes the reference's checkpoint layout (src/kbnet_model.py:353-376), keys
        prefixed with `module.` like its DataParallel-wrapped modules produce."""
        pref = lambda sd: {"module." + k: v for k, v in sd.items()}
        torch.save({"train_step": step,
                    "optimizer_state_dict": optimizer.state_dict() if optimizer is not None else {},
                    "sparse_to_dense_pool_state_dict": pref(self.sparse_to_dense_pool.state_dict()),
                    "encoder_state_dict": pref(self.encoder.state_dict()),
                    "decoder_state_dict": pref(self.decoder.state_dict())}, checkpoint_path)


from . import kbnet_train  # noqa: E402  (kbnet_train.py: the recorded forward of KBNetModel(trainable=True))
from . import summary  # noqa: E402  (summary.py: KBNetModel.log_summary)
from .posenet import PoseDecoder, PoseEncoder, PoseNetModel  # noqa: E402,F401  (posenet.py: the pose network beside KBNetModel)
from .posenet_resnet import (ResNetBlock, ResNetEncoder, ResNetPoseDecoder, ResNetPoseNetModel,  # noqa: E402,F401  (posenet_resnet.py:
                             load_pose_model)                                                      # the ResNet-18 / 34 pose networks)
