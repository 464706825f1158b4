"""Tensor-level wrappers over the C ABI.  PyTorch is plumbing here: it owns the
device memory and the stream; every computation below is a HIP kernel launch
through libkbnet_hip.so.  CPU tensors are rejected (no fallback).
"""

from __future__ import annotations

import contextlib
import ctypes as C
import functools
import struct
from typing import List, Optional, Sequence

import torch

from . import _lib
from ._lib import ConvSrc, KbnError, check


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _on_tensor_device(fn):
    """The C side launches on the calling thread's CURRENT device and on the stream it is handed, so every
    wrapper below runs with the tensors' device current (reference modules accept any device:
    `KBNetModel(..., device=cuda:1)` while cuda:0 is current, DataParallel replicas on per-device
    threads) and takes torch's current stream of THAT device.  Tensors on different devices are an error."""
    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        idx = None
        for a in list(args) + list(kwargs.values()):
            if isinstance(a, torch.Tensor) and a.is_cuda:
                if idx is None:
                    idx = a.device.index
                elif a.device.index != idx:
                    raise KbnError(f"{fn.__name__}: tensors live on different devices (cuda:{idx} and {a.device})")
        if idx is None or idx == torch.cuda.current_device():
            return fn(*args, **kwargs)
        with torch.cuda.device(idx):
            return fn(*args, **kwargs)
    return wrapper


def reload_env():
    """Re-reads the KBN_* switches from the environment (the library reads them once at load time).  The host mirror's
    own A/B switches (KBN_NO_PAIR*, KBN_NO_OVERLAP, ...) are answered by the library too (`knob`), so they follow."""
    _lib.load().kbn_reload_env()


def knob(name: str) -> int:
    """Value of a KBN_* switch as the library read it (kbn_knob): 0 when unset."""
    return int(_lib.load().kbn_knob(name.encode()))


def split_enabled() -> bool:
    """False under KBN_NO_SPLIT=1: every split-operand entry point declines (A/B against the all-fp32-MFMA path)."""
    return knob("KBN_NO_SPLIT") == 0


@contextlib.contextmanager
def autotune(enabled: bool = True):
    """First-use tuning of launch geometry is OFF by default (ABI calls only enqueue work).  Inside this
    context the first launch of every problem shape times its candidate geometries on the stream and
    waits for its own events (kbn_set_autotune); the choices stay cached for the process."""
    lib = _lib.load()
    old = lib.kbn_set_autotune(1 if enabled else 0)
    try:
        yield
    finally:
        lib.kbn_set_autotune(old)


# Optional per-launch timing (bench.py): when PROFILE is a list, every ABI call is
# bracketed by HIP events recorded on the launch stream and
# (name, work, executed, pipe, nbytes, start, end) is appended.  `work` is the launch's ALGORITHMIC FLOPs
# (the reference's direct formulation: convs, and the conv part of S2D / the head; 0 for pure byte movers); `executed` the FLOPs the launch really
# issues on the matrix cores (Winograd / phase-decomposed up-convs execute fewer; tile and channel padding
# execute more), None for byte-bound launches; `pipe` names the pipe those MFMAs run on -- "fp32"
# (v_mfma_f32_*_f32: the vector datapath's 157.3 TFLOP/s), "fp16" (split-operand kernels: three fp16 MFMAs per fp32
# product on the 2.5 PFLOP/s matrix core) -- so that whoever prices `executed`
# uses the right peak; `nbytes` the launch's ALGORITHMIC HBM bytes (every input read once + every output written once).
PROFILE = None
PIPE_PEAK_TFLOPS = {"fp32": 157.3, "fp16": 2500.0}    # MI355X_MICROARCH.md, dense
PIPE_PRODUCTS = {"fp32": 1.0, "fp16": 3.0}    # MFMA products issued per product of the reference


def _launch(name: str, work: float, fn, executed=None, pipe: Optional[str] = None, nbytes: Optional[float] = None):
    if PROFILE is None:
        return fn()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    status = fn()
    end.record()
    PROFILE.append((name, work, executed() if callable(executed) else executed, pipe, nbytes, start, end))
    return status


def _launched(what: str, name: str, work: float, fn, **record) -> bool:
    """_launch for an entry point that may decline the problem: False on KBN_ERR_UNSUPPORTED, with the profile record dropped (the
    wrapper returns None and whatever the caller launches instead records itself); any other status goes through `check`."""
    status = _launch(name, work, fn, **record)
    if status == _lib.KBN_ERR_UNSUPPORTED:
        if PROFILE is not None:
            PROFILE.pop()
        return False
    check(status, what)
    return True


def _act_args(negative_slope: Optional[float]):
    """(has_activation, negative_slope) as the entry points take max(v, slope v); None: no activation."""
    return (0, 0.0) if negative_slope is None else (1, float(negative_slope))


def _src_bytes(srcs, n: int) -> float:
    """fp32-equivalent bytes the tensor / pair sources of a conv hold (4 B per value in both formats)."""
    total = 0
    for s in srcs:
        if s.kind in (_lib.KBN_SRC_TENSOR, _lib.KBN_SRC_PAIR):
            total += s.channels * s.src_height * s.src_width
    return 4.0 * n * total


def conv_executed_flops(n, out_channels, in_channels, kernel_size, stride, in_height, in_width, resize=False):
    """FLOPs kbn_conv2d_forward issues on the matrix cores for this problem, padding included, from the
    launch plan (kbn_conv2d_query): Winograd F(2x2,3x3) regions of 64 tiles x 16 frequencies x 64-channel
    output tiles; direct kernels 4*MW m-blocks of 16 pixels x NB n-blocks of 16 channels x padded K."""
    pl = conv_plan(n, out_channels, in_channels, kernel_size, stride, in_height, in_width, resize)
    if pl["kernel"] == "wino":
        return 2.0 * pl["workgroups"] * 64 * 16 * in_channels * 64
    cpad = -(-in_channels // pl["CK"]) * pl["CK"]
    return 2.0 * pl["workgroups"] * (4 * pl["MW"] * 16) * (pl["NB"] * 16) * cpad * kernel_size * kernel_size


def upconv2x_executed_flops(n, in_channels, out_channels, src_height, src_width, plain=False):
    """`plain`: the four-phase form whatever the shape (the transposed conv: kbn_deconv2x_forward)."""
    info = (C.c_int * 4)()
    check(_lib.load().kbn_upconv2x_query(n, in_channels, out_channels, src_height, src_width, info), "kbn_upconv2x_query")
    if plain and info[0] == 9:   # the 9-product form has its own filter tiling: the four-phase one pads to make_up2x_plan's tiles
        nblk = -(-out_channels // 16)
        best, bestpad = 1, 1 << 30
        for nb in range(1, 5):
            pad = -(-nblk // nb) * nb
            if pad < bestpad or (pad == bestpad and nb > best):
                best, bestpad = nb, pad
        info[1] = bestpad * 16
    return 2.0 * n * src_height * src_width * (16 if plain else info[0]) * info[1] * info[2]


_PLAN_CACHE = {}


def conv_plan(n: int, out_channels: int, in_channels: int, kernel_size: int, stride: int, in_height: int,
              in_width: int, resize: bool = False):
    """Kernel variant the library picks (kbn_conv2d_query): dict with CK, NB, MW, TWB, TH,
    workgroups, maxpos, pipelined (3 = conv_wino_kernel, where MW x TWB is the region's tile
    rows x columns; 2 = conv_dma_kernel; 1/0 = conv_igemm_kernel) and `kernel` (its name)."""
    key = (n, out_channels, in_channels, kernel_size, stride, in_height, in_width, int(resize))
    if key not in _PLAN_CACHE:
        info = (C.c_int * 8)()
        check(_lib.load().kbn_conv2d_query(*key, info), "kbn_conv2d_query")
        d = dict(zip(("CK", "NB", "MW", "TWB", "TH", "workgroups", "maxpos", "pipelined"), info))
        d["kernel"] = {3: "wino", 2: "dma"}.get(d["pipelined"], "igemm")
        _PLAN_CACHE[key] = d
    return _PLAN_CACHE[key]


ROUTE_FAMILIES = ("none", "wino", "dma", "dma_syn", "igemm_pipe", "igemm", "up2x9", "up2x_dma", "up2x")
_ROUTE_FIELDS = ("family", "KS", "STRIDE", "CK", "NB", "MW", "TWB", "RT", "CT", "epi_lds", "form", "granule", "half")


def last_conv_route() -> dict:
    """What the calling thread's LAST conv2d / conv2d_kbnet / upconv2x / deconv2x call really launched (kbn_conv_last_route;
    conv_plan and PROFILE's names are predictions from the shape).  `family` is one of ROUTE_FAMILIES ("none": the call
    failed or found no kernel); KS, STRIDE, CK, NB, MW, TWB are the template arguments of the kernel that ran, RT x CT the
    Winograd region, `epi_lds` the LDS epilogue in effect, `form` / `granule` / `half` the up-conv's algebraic form
    (9 / 3 / 4), DMA granule in bytes (16 / 4 / 0) and half-size tile."""
    info = (C.c_int * 16)()
    check(_lib.load().kbn_conv_last_route(info), "kbn_conv_last_route")
    d = dict(zip(_ROUTE_FIELDS, info))
    d["family"] = ROUTE_FAMILIES[d["family"]]
    return d


def _require(t: torch.Tensor, name: str, ndim: Optional[int] = None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise KbnError(f"{name}: expected a CUDA/HIP tensor (the HIP path has no CPU fallback)")
    if t.dtype != torch.float32:
        raise KbnError(f"{name}: expected float32, got {t.dtype}")
    if ndim is not None and t.dim() != ndim:
        raise KbnError(f"{name}: expected {ndim} dims, got {tuple(t.shape)}")


def _weight(t: torch.Tensor, name: str = "weight") -> torch.Tensor:
    """A 4-d fp32 parameter as the dense device tensor the C side reads."""
    w = t.detach().contiguous()
    _require(w, name, 4)
    return w


def _out_tensor(out: Optional[torch.Tensor], shape, device, name: str = "out", planes: bool = False) -> torch.Tensor:
    """A new fp32 tensor of `shape`, or the given `out` once it is known to be an fp32 device tensor of that shape, contiguous
    (`planes`: dense frames suffice, e.g. a channel slice; the caller takes its pointer with _planes)."""
    if out is None:
        return torch.empty(shape, device=device, dtype=torch.float32)
    _require(out, name, len(shape))
    if tuple(out.shape) != tuple(shape) or not (planes or out.is_contiguous()):
        raise KbnError(f"{name} has shape {tuple(out.shape)}, expected {'' if planes else 'a contiguous '}{tuple(shape)}")
    return out


def _planes(t: torch.Tensor, name: str):
    """(ptr, batch_stride) of an N x C x H x W tensor whose frames are dense C x H x W blocks
    (a contiguous tensor or a channel slice of one)."""
    _require(t, name, 4)
    n, c, h, w = t.shape
    if t.stride(3) != 1 or t.stride(2) != w or t.stride(1) != h * w:
        raise KbnError(f"{name}: planes must be dense (got strides {t.stride()})")
    return t.data_ptr(), (t.stride(0) if n > 1 else c * h * w)


def _int_array(values: Sequence[int]):
    arr = (C.c_int * max(len(values), 1))(*values)
    return arr


# ------------------------------------------------------------- activation statistics
class ActStats:
    """Per-frame max |a| slots of the tensors of one forward (include/kbnet_hip.h, "activation statistics"): one zeroed
    int32 buffer [capacity][n]; `new()` hands out a row.  A conv launch folds max |out| of every frame into the slot
    it is given (`out_absmax=`); `tensor_src(t, absmax=slot)` hands it to the consumer, whose split-operand kernel
    derives its fp16 window from it on the device, frame by frame.  Allocated inside the forward (also under graph
    capture: the zero fill is a node of the graph), so nothing outlives the call."""

    def __init__(self, n: int, device, capacity: int = 40):
        self.buf = torch.zeros((capacity, n), device=device, dtype=torch.int32)
        self.n, self.used = n, 0
        self.unfilled = set()   # data_ptr of slots handed to a launch that does not fill them (a layer-by-layer activation pass in between)

    def skip(self, slot: Optional[torch.Tensor]):
        """A producer that writes (part of) the slot's tensor without folding its maxima: consumers measure the tensor."""
        if slot is not None:
            self.unfilled.add(slot.data_ptr())

    def usable(self, slot_ptr) -> bool:
        return bool(slot_ptr) and slot_ptr not in self.unfilled

    def new(self) -> torch.Tensor:
        if self.used == self.buf.shape[0]:   # more tensors than foreseen: chain another buffer (one more fill launch)
            self.buf = torch.zeros_like(self.buf)
            self.used = 0
        slot = self.buf[self.used]
        self.used += 1
        return slot

    def measure(self, t: torch.Tensor) -> torch.Tensor:
        """A slot filled by a pass over `t` (kbn_absmax_frames): tensors that come from outside the forward."""
        return absmax_frames(t, self.new())


def _slot_ptr(slot: Optional[torch.Tensor], n: int):
    if slot is None:
        return None
    if slot.dtype != torch.int32 or slot.dim() != 1 or slot.shape[0] != n or not slot.is_contiguous() or not slot.is_cuda:
        raise KbnError(f"absmax slot: expected a contiguous int32 device tensor of {n} elements")
    return slot.data_ptr()


@_on_tensor_device
def absmax_frames(t: torch.Tensor, slot: torch.Tensor) -> torch.Tensor:
    """Folds max |t[i]| of every frame i into slot[i] (bit patterns; kbn_absmax_frames).  No synchronisation."""
    ptr, bs = _planes(t, "t")
    n, c, h, w = t.shape
    check(_launch("absmax", 4.0 * n * c * h * w,
                  lambda: _lib.load().kbn_absmax_frames(ptr, bs, n, c * h * w, _slot_ptr(slot, n), _stream()),
                  nbytes=4.0 * n * c * h * w), "kbn_absmax_frames")
    return slot


def slot_values(slot: torch.Tensor) -> torch.Tensor:
    """The per-frame maxima a slot holds, as floats (diagnostics, tests; synchronises when read)."""
    return slot.view(torch.float32)


# ----------------------------------------------------------------------------- S2D
@_on_tensor_device
def s2d_forward(x, w_pool_convs: List[torch.Tensor], w_conv, min_pool_sizes, max_pool_sizes,
                negative_slope: float = 0.2, out: Optional[torch.Tensor] = None):
    lib = _lib.load()
    _require(x, "x", 4)
    x = x.contiguous()
    n, cin, h, w = x.shape
    ws = [_weight(wt, f"pool_convs.{i}.weight") for i, wt in enumerate(w_pool_convs)]
    wc = _weight(w_conv, "conv.weight")
    nf = wc.shape[0]
    mins = [int(s) for s in min_pool_sizes if s > 1]
    maxs = [int(s) for s in max_pool_sizes if s > 1]
    if ws[0].shape[1] != len(mins) + len(maxs) or wc.shape[1] != nf + cin:
        raise KbnError("S2D weight shapes do not match the pool lists / input channels")
    out = _out_tensor(out, (n, nf, h, w), x.device, "s2d_forward: out")
    wptrs = (C.c_void_p * len(ws))(*[wt.data_ptr() for wt in ws])
    amin, amax = _int_array(mins), _int_array(maxs)
    # (work = the layer's multiply-adds x 2: nothing is skipped or padded, so executed = algorithmic; its bytes travel as `nbytes`)
    check(_launch("s2d", 2.0 * n * h * w * (ws[0].shape[1] * nf + (len(ws) - 1) * nf * nf + 9 * (nf + cin) * nf),
                  lambda: lib.kbn_s2d_forward(x.data_ptr(), wptrs, wc.data_ptr(), out.data_ptr(), n, h, w, cin,
                                              amin, len(mins), amax, len(maxs), len(ws), nf,
                                              float(negative_slope), _stream()),
                  # both convs on v_mfma_f32_4x4x1 (the fp32 datapath): 2 x (pools x nf + (convs - 1) x nf^2 + 9 (nf + cin) nf) per pixel
                  executed=2.0 * n * h * w * (ws[0].shape[1] * nf + (len(ws) - 1) * nf * nf + 9 * (nf + cin) * nf),
                  pipe="fp32", nbytes=4.0 * n * h * w * (cin + nf)), "kbn_s2d_forward")
    return out


@_on_tensor_device
def s2d_pyramid(x, min_pool_sizes, max_pool_sizes):
    lib = _lib.load()
    _require(x, "x", 4)
    x = x.contiguous()
    n, cin, h, w = x.shape
    mins = [int(s) for s in min_pool_sizes if s > 1]
    maxs = [int(s) for s in max_pool_sizes if s > 1]
    out = torch.empty((n, len(mins) + len(maxs), h, w), device=x.device, dtype=torch.float32)
    check(lib.kbn_s2d_pyramid(x.data_ptr(), cin * h * w, out.data_ptr(), n, h, w, _int_array(mins),
                              len(mins), _int_array(maxs), len(maxs), _stream()), "kbn_s2d_pyramid")
    return out


# ---------------------------------------------------------------------- intrinsics
@_on_tensor_device
def intrinsics_inverse(intrinsics, scale_x: float = 1.0, scale_y: float = 1.0):
    lib = _lib.load()
    _require(intrinsics, "intrinsics", 3)
    k = intrinsics.contiguous()
    if k.shape[1:] != (3, 3):
        raise KbnError("intrinsics must be N x 3 x 3")
    out = torch.empty_like(k)
    check(lib.kbn_intrinsics_inverse(k.data_ptr(), out.data_ptr(), k.shape[0], float(scale_x),
                                     float(scale_y), _stream()), "kbn_intrinsics_inverse")
    return out


@_on_tensor_device
def camera_coordinates(kinv, height: int, width: int):
    lib = _lib.load()
    _require(kinv, "kinv", 3)
    kinv = kinv.contiguous()
    out = torch.empty((kinv.shape[0], 3, height, width), device=kinv.device, dtype=torch.float32)
    check(lib.kbn_camera_coordinates(kinv.data_ptr(), out.data_ptr(), kinv.shape[0], height, width,
                                     _stream()), "kbn_camera_coordinates")
    return out


# --------------------------------------------------------------------------- conv2d
def _pack_into(out: Optional[torch.Tensor], nbytes: int, like: torch.Tensor, pack, what: str) -> torch.Tensor:
    """The blob of `nbytes` that `pack(ptr)` -- a C packer, returning its status -- fills: `out` when that is a blob of this size on
    `like`'s device (a re-pack in place: the device pointer a captured graph holds stays valid), otherwise a new one."""
    n = nbytes // 4
    if out is None or out.numel() != n or out.device != like.device or out.dtype != torch.float32 or not out.is_contiguous():
        out = torch.empty(n, device=like.device, dtype=torch.float32)
    check(pack(out.data_ptr()), what)
    return out


@_on_tensor_device
def pack_conv_weight(weight: torch.Tensor, stride: int = 1, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """OIHW -> MFMA fragment order for a conv of this stride (done once per weight; see
    _PackedBlob in modules.py).  `out`: an existing blob of the right size to re-pack into (keeps
    the device pointer a captured graph holds valid)."""
    lib = _lib.load()
    w = _weight(weight)
    oc, cin, kh, kw = w.shape
    if kh != kw:
        raise KbnError("square kernels only")
    nbytes = lib.kbn_conv2d_packed_weight_bytes(oc, cin, kh, stride)
    if nbytes == 0:
        raise KbnError(f"unsupported conv weight shape {tuple(w.shape)}")
    return _pack_into(out, nbytes, w, lambda p: lib.kbn_conv2d_pack_weight(w.data_ptr(), p, oc, cin, kh, stride, _stream()),
                      "kbn_conv2d_pack_weight")


def tensor_src(t: torch.Tensor, name="src", absmax: Optional[torch.Tensor] = None) -> ConvSrc:
    """`absmax`: the tensor's per-frame max |a| slot (ActStats), when its producer filled one."""
    ptr, bs = _planes(t, name)
    s = ConvSrc()
    s.kind = _lib.KBN_SRC_TENSOR
    s.channels = t.shape[1]
    s.data = ptr
    s.batch_stride = bs
    s.src_height, s.src_width = t.shape[2], t.shape[3]
    s.absmax = _slot_ptr(absmax, t.shape[0])
    s._keep = (t, absmax)   # the struct holds raw pointers
    return s


class PairTensor:
    """An activation tensor in the producer-written split format (include/kbnet_hip.h, "PAIR tensors"): per frame
    [channels / 8][h1 | h2][H * W + 1 pixels][8 channels] fp16 with a 2^k = h1 + 2^-11 h2, the per-frame 2^k in `scale`
    (written by the producing kernel) and the true max |a| per frame in the `absmax` slot.  Only tensors that split-operand
    kernels alone read are kept this way: the decoder's concat-conv outputs (conv3x3_split(out=PairTensor), read by the
    next up-conv through pair_src).  Same bytes as fp32; the consumers stage it by LDS-DMA instead of splitting it."""

    LOG = None   # diagnostics (tests/analysis): when a list hangs here, every PairTensor of a forward is appended

    def __init__(self, n: int, channels: int, height: int, width: int, device, stats: "ActStats"):
        if channels % 8:
            raise KbnError("PairTensor: channels must be a multiple of 8")
        if PairTensor.LOG is not None:
            PairTensor.LOG.append(self)
        self.shape = (n, channels, height, width)
        self.data = torch.empty((n, channels // 8, 2, height * width + 1, 8), device=device, dtype=torch.float16)
        self.scale = torch.empty(n, device=device, dtype=torch.float32)
        self.absmax = stats.new()
        # stride-2 producers (conv3x3_split(stride=2, out=PairTensor)) can also write the pixels (2y, 2x) in fp32, as a dense
        # N x C x ceil(H/2) x ceil(W/2) tensor: what the next KB level's 1x1 stride-2 conv_fused reads of this tensor
        self.sub: Optional[torch.Tensor] = None

    @property
    def device(self):
        return self.data.device

    def with_sub(self) -> "PairTensor":
        n, c, h, w = self.shape
        self.sub = torch.empty((n, c, (h + 1) // 2, (w + 1) // 2), device=self.data.device, dtype=torch.float32)
        return self

    def window_slack_log2(self) -> torch.Tensor:
        """Per frame: binades between the top of the fp16 window the producer chose from its BOUND (2^15 / scale) and the true
        max |a| it then measured (the absmax slot).  The two terms keep 22 bits down to 2^-29 of the window, so a slack
        below ~16 costs nothing (tests/test_split_math_cpu.py); diagnostics only (synchronises)."""
        amax = slot_values(self.absmax).double().clamp_min(1e-300)
        return 15.0 - torch.log2(amax * self.scale.double())

    def float(self) -> torch.Tensor:
        """The tensor as N x C x H x W fp32 (tests, diagnostics)."""
        n, c, h, w = self.shape
        v = self.data[:, :, 0, :h * w].double() + self.data[:, :, 1, :h * w].double() / 2048.0   # n, c/8, hw, 8
        v = v / self.scale.double().view(n, 1, 1, 1)
        return v.permute(0, 1, 3, 2).reshape(n, c, h, w).float()


def pair_src(t: PairTensor, name="src") -> ConvSrc:
    n, c, h, w = t.shape
    s = ConvSrc()
    s.kind = _lib.KBN_SRC_PAIR
    s.channels = c
    s.data = t.data.data_ptr()
    s.batch_stride = t.data.stride(0)
    s.src_height, s.src_width = h, w
    s.absmax = _slot_ptr(t.absmax, n)
    s.scale = t.scale.data_ptr()
    s._keep = (t,)
    return s


def _kinv(kinv: torch.Tensor) -> torch.Tensor:
    """The N x 3 x 3 inverse intrinsics as the dense row-major block the kernels read through a raw pointer (torch.linalg.inv
    hands back column-major matrices: read in place they would be their transposes)."""
    _require(kinv, "kinv", 3)
    if tuple(kinv.shape[1:]) != (3, 3):
        raise KbnError(f"kinv must be N x 3 x 3, got {tuple(kinv.shape)}")
    return kinv.contiguous()


def coords_src(kinv: torch.Tensor) -> ConvSrc:
    kinv = _kinv(kinv)
    s = ConvSrc()
    s.kind = _lib.KBN_SRC_COORDS
    s.channels = 3
    s.kinv = kinv.data_ptr()
    s._keep = (kinv,)   # the struct holds raw pointers: the tensors live as long as it does
    return s


def xyz_src(depth: torch.Tensor, proj_weight: torch.Tensor, kinv: Optional[torch.Tensor], coordinates: Optional[torch.Tensor] = None) -> ConvSrc:
    """The KB layer's backprojection channels coords * act(proj . depth), computed in-kernel; coords = K^-1 [x y 1]^T from `kinv`
    (N x 3 x 3) or read from the dense `coordinates` tensor (N x 3 x H x W, the reference's own argument)."""
    ptr, bs = _planes(depth, "depth")
    s = ConvSrc()
    s.kind = _lib.KBN_SRC_XYZ
    s.channels = 3
    s.data = ptr
    s.batch_stride = bs
    s.aux_channels = depth.shape[1]
    s.proj_weight = proj_weight.data_ptr()
    if coordinates is not None:
        _require(coordinates, "coordinates", 4)
        if not coordinates.is_contiguous() or tuple(coordinates.shape) != (depth.shape[0], 3, depth.shape[2], depth.shape[3]):
            raise KbnError("coordinates must be a contiguous N x 3 x H x W tensor of the depth features' size")
        s.coordinates = coordinates.data_ptr()
        s.coordinates_batch_stride = coordinates.stride(0)
    else:
        kinv = _kinv(kinv)
        s.kinv = kinv.data_ptr()
    s._keep = (depth, proj_weight, kinv, coordinates)
    return s


@_on_tensor_device
def conv2d(srcs: List[ConvSrc], packed_weight: torch.Tensor, n: int, out_channels: int,
           kernel_size: int, stride: int, in_height: int, in_width: int, out: torch.Tensor,
           resize: bool = False, negative_slope: Optional[float] = 0.2, out_absmax: Optional[torch.Tensor] = None):
    """`out` is an N x out_channels x ceil(H/s) x ceil(W/s) tensor or channel slice; `out_absmax`: slot that receives
    max |out| per frame."""
    lib = _lib.load()
    arr = (ConvSrc * len(srcs))(*srcs)
    optr, obs = _planes(out, "out")
    oh, ow = -(-in_height // stride), -(-in_width // stride)
    if tuple(out.shape) != (n, out_channels, oh, ow):
        raise KbnError(f"out has shape {tuple(out.shape)}, expected {(n, out_channels, oh, ow)}")
    cin = sum(s.channels for s in srcs)
    name = "conv_igemm"
    if PROFILE is not None:
        pl = conv_plan(n, out_channels, cin, kernel_size, stride, in_height, in_width, resize)
        if pl["kernel"] == "wino":
            name = "conv_wino"
        else:
            name = ("conv_dma" if pl["pipelined"] == 2 else "conv_igemm") + \
                f"<{kernel_size},{stride},{pl['CK']},{pl['NB']},{pl['MW']}>"
    check(_launch(name,
                  2.0 * n * oh * ow * cin * kernel_size * kernel_size * out_channels,
                  lambda: lib.kbn_conv2d_forward(arr, len(srcs), packed_weight.data_ptr(), optr, obs, n,
                                                 out_channels, kernel_size, stride, in_height, in_width,
                                                 _lib.KBN_RESIZE_NEAREST if resize else _lib.KBN_RESIZE_NONE,
                                                 *_act_args(negative_slope), _slot_ptr(out_absmax, n), _stream()),
                  executed=lambda: conv_executed_flops(n, out_channels, cin, kernel_size, stride, in_height, in_width,
                                                       resize),
                  pipe="fp32",
                  nbytes=_src_bytes(srcs, n) + 4.0 * n * (oh * ow * out_channels + sum(
                      s.aux_channels * in_height * in_width for s in srcs if s.kind == _lib.KBN_SRC_XYZ))), "kbn_conv2d_forward")
    return out


# ------------------------------------------------- layer-by-layer form: activation in place, backprojection
ACT_KINDS = {"elu": _lib.KBN_ACT_ELU, "sigmoid": _lib.KBN_ACT_SIGMOID}


@_on_tensor_device
def activation_(t: torch.Tensor, kind: str, out_absmax: Optional[torch.Tensor] = None) -> torch.Tensor:
    """t <- ELU(t) / sigmoid(t) in place (kbn_activation_forward): the activation of a conv that was launched without one, for
    the activations the fused kernels do not carry (reference src/net_utils.py:38-43).  `t`: a dense N x C x H x W tensor or a
    channel slice of one.  `out_absmax`: the tensor's per-frame max |a| slot (ActStats), filled with the maxima of the activated values."""
    lib = _lib.load()
    tptr, tbs = _planes(t, "t")
    n = t.shape[0]
    per = t.shape[1] * t.shape[2] * t.shape[3]
    check(_launch("activation", 0.0, lambda: lib.kbn_activation_forward(tptr, tbs, n, per, ACT_KINDS[kind], _slot_ptr(out_absmax, n), _stream()),
                  nbytes=8.0 * n * per), "kbn_activation_forward")
    return t


@_on_tensor_device
def scale_planes(x: torch.Tensor, z: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[n, c] = x[n, c] * z[n, 0] (kbn_scale_planes_forward): the KB block's xyz = coordinates * z (reference
    src/net_utils.py:1357-1359) when z is a tensor of its own."""
    lib = _lib.load()
    xptr, xbs = _planes(x, "x")
    zptr, zbs = _planes(z, "z")
    n, c, h, w = x.shape
    if tuple(z.shape) != (n, 1, h, w):
        raise KbnError(f"scale_planes: z has shape {tuple(z.shape)}, expected {(n, 1, h, w)}")
    out = _out_tensor(out, (n, c, h, w), x.device, "scale_planes: out", planes=True)
    optr, obs = _planes(out, "out")
    check(_launch("scale_planes", 1.0 * n * c * h * w,
                  lambda: lib.kbn_scale_planes_forward(xptr, xbs, zptr, zbs, optr, obs, n, c, h, w, _stream()),
                  nbytes=4.0 * n * h * w * (2 * c + 1)), "kbn_scale_planes_forward")
    return out


# ---------------------------------------------------------------------- up-conv 2x
def _deconv_weight(weight: torch.Tensor) -> torch.Tensor:
    """ConvTranspose2d's in x out x 3 x 3 parameter with out_channels leading: the layout the packers read."""
    return weight.detach().permute(1, 0, 2, 3).contiguous()


@_on_tensor_device
def pack_upconv2x_weight(weight: torch.Tensor, out: Optional[torch.Tensor] = None, transposed: bool = False) -> torch.Tensor:
    """OIHW 3x3 weight -> phase-summed MFMA blob for `upconv2x` (once per weight).  `transposed`: `weight` is a
    ConvTranspose2d(kernel 3, stride 2, padding 1, output_padding 1) parameter, in x out x 3 x 3, and the blob is
    for `upconv2x(transposed=True)` (kbn_deconv2x_pack_weight)."""
    lib = _lib.load()
    w = _weight(_deconv_weight(weight) if transposed else weight)
    oc, cin, kh, kw = w.shape
    if (kh, kw) != (3, 3):
        raise KbnError("upconv2x needs a 3x3 weight")
    pack = lib.kbn_deconv2x_pack_weight if transposed else lib.kbn_upconv2x_pack_weight
    nbytes = lib.kbn_upconv2x_packed_weight_bytes(oc, cin)
    if nbytes == 0:      # a refusal, not "an empty blob"
        raise KbnError(f"unsupported up-conv weight shape {tuple(w.shape)}")
    return _pack_into(out, nbytes, w, lambda p: pack(w.data_ptr(), p, oc, cin, _stream()),
                      "kbn_deconv2x_pack_weight" if transposed else "kbn_upconv2x_pack_weight")


@_on_tensor_device
def upconv2x(x: torch.Tensor, packed_weight: torch.Tensor, out_channels: int, out: torch.Tensor,
             negative_slope: Optional[float] = 0.2, out_absmax: Optional[torch.Tensor] = None, transposed: bool = False):
    """nearest 2x upsample + conv3x3 (+ LeakyReLU): x N x C x h x w -> out N x out_channels x 2h x 2w.
    `transposed`: ConvTranspose2d(kernel 3, stride 2, padding 1, output_padding 1) (+ LeakyReLU) instead, same sizes
    (kbn_deconv2x_forward; blob from pack_upconv2x_weight(transposed=True))."""
    lib = _lib.load()
    xptr, xbs = _planes(x, "x")
    n, cin, h, w = x.shape
    optr, obs = _planes(out, "out")
    if tuple(out.shape) != (n, out_channels, 2 * h, 2 * w):
        raise KbnError(f"out has shape {tuple(out.shape)}, expected {(n, out_channels, 2 * h, 2 * w)}")
    fwd = lib.kbn_deconv2x_forward if transposed else lib.kbn_upconv2x_forward
    name = "kbn_deconv2x_forward" if transposed else "kbn_upconv2x_forward"
    # algorithmic work of the reference formulation (9 taps at the upsampled resolution; transposed: 9 taps per SOURCE pixel)
    work = 2.0 * n * h * w * cin * 9 * out_channels * (1 if transposed else 4)
    if transposed:   # always the four-phase form: 16 channel products per source pixel over the padded channel counts
        executed = lambda: upconv2x_executed_flops(n, cin, out_channels, h, w, plain=True)
    else:
        executed = lambda: upconv2x_executed_flops(n, cin, out_channels, h, w)
    check(_launch("conv_up2x", work,
                  lambda: fwd(xptr, xbs, packed_weight.data_ptr(), optr, obs, n, cin,
                              out_channels, h, w, *_act_args(negative_slope), _slot_ptr(out_absmax, n), _stream()),
                  executed=executed, pipe="fp32",
                  nbytes=4.0 * n * h * w * (cin + 4 * out_channels)), name)
    return out


# ------------------------------------------------------------------------ KB block
@_on_tensor_device
def kb_block(image, depth, coordinates, kinv, fused, packed_w_image, packed_w_depth, proj_weight,
             packed_w_fused, filters_image: int, filters_depth: int, filters_fused: int,
             out_image, out_depth, out_fused, negative_slope: float = 0.2, absmax_image=None, absmax_depth=None,
             absmax_fused=None):
    """Inputs/outputs may be channel slices; exactly one of coordinates / kinv may be None.  absmax_*: slots that
    receive max |out| per frame of the three outputs (two may be the same slot)."""
    lib = _lib.load()
    n, ci, h, w = image.shape
    iptr, ibs = _planes(image, "image")
    dptr, dbs = _planes(depth, "depth")
    cd = depth.shape[1]
    if fused is not None:
        fptr, fbs = _planes(fused, "fused")
        cf = fused.shape[1]
    else:
        fptr, fbs, cf = None, 0, 0
    cptr = None
    if coordinates is not None:
        _require(coordinates, "coordinates", 4)
        if not coordinates.is_contiguous() or tuple(coordinates.shape) != (n, 3, h, w):
            raise KbnError("coordinates must be a contiguous N x 3 x H x W tensor")
        cptr = coordinates.data_ptr()
    kptr = None
    if kinv is not None:
        _require(kinv, "kinv", 3)
        kptr = kinv.data_ptr()
    pw = proj_weight.detach().contiguous()
    _require(pw, "proj_weight")
    oh, ow = (h + 1) // 2, (w + 1) // 2
    for t, f, nm in ((out_image, filters_image, "out_image"), (out_depth, filters_depth, "out_depth"),
                     (out_fused, filters_fused, "out_fused")):
        if tuple(t.shape) != (n, f, oh, ow):
            raise KbnError(f"{nm} has shape {tuple(t.shape)}, expected {(n, f, oh, ow)}")
    oi, oibs = _planes(out_image, "out_image")
    od, odbs = _planes(out_depth, "out_depth")
    of, ofbs = _planes(out_fused, "out_fused")
    flops = 2.0 * n * oh * ow * (9 * ci * filters_image + 9 * (cd + 3) * filters_depth +
                                  (ci + 3 + cf) * filters_fused)
    check(_launch("kb_block", flops,
                  lambda: lib.kbn_kb_block_forward(iptr, ibs, dptr, dbs, cptr, kptr, fptr, fbs,
                                                   packed_w_image.data_ptr(), packed_w_depth.data_ptr(),
                                                   pw.data_ptr(), packed_w_fused.data_ptr(), oi, oibs, od, odbs,
                                                   of, ofbs, n, h, w, ci, cd, cf, filters_image, filters_depth,
                                                   filters_fused, float(negative_slope), _slot_ptr(absmax_image, n),
                                                   _slot_ptr(absmax_depth, n), _slot_ptr(absmax_fused, n), _stream()),
                  executed=flops,   # direct convs: executed = algorithmic (tile padding not counted)
                  pipe="fp32", nbytes=4.0 * n * (h * w * (ci + cd + cf) + oh * ow * (filters_image + filters_depth + filters_fused))),
          "kbn_kb_block_forward")
    return out_image, out_depth, out_fused


# ---------------------------------------------------------------------- depth head
HEAD_MAX_CHANNELS = 16   # csrc/head.hip HD_MAXC


@_on_tensor_device
def depth_head(x, weight, min_predict_depth: float, max_predict_depth: float, return_logits=False, out=None):
    """`out`: optional contiguous N x 1 x H x W destination (e.g. a batch slice of a larger output buffer)."""
    lib = _lib.load()
    _require(x, "x", 4)
    x = x.contiguous()
    w = _weight(weight)
    n, c, h, wd = x.shape
    if tuple(w.shape) != (1, c, 3, 3):
        raise KbnError(f"depth head weight must be 1 x {c} x 3 x 3")
    if c > HEAD_MAX_CHANNELS:
        # run_kbnet.py --n_filters_decoder with a last width past the head kernel's 16 channels: output0 as a conv of its own, then the
        # mapping as the head kernel over that one plane with an identity tap (1.0 * logit + eight exact zeros: the logits as they are)
        plane = conv2d([tensor_src(x, "x")], pack_conv_weight(w, 1), n, 1, 3, 1, h, wd,
                       torch.empty((n, 1, h, wd), device=x.device, dtype=torch.float32), negative_slope=None)
        # (device ops only -- a fill and a pad: this runs under HIP-graph capture too)
        ident = torch.nn.functional.pad(torch.ones((1, 1, 1, 1), device=x.device, dtype=torch.float32), (1, 1, 1, 1))
        return depth_head(plane, ident, min_predict_depth, max_predict_depth, return_logits=return_logits, out=out)
    depth = _out_tensor(out, (n, 1, h, wd), x.device)
    logits = torch.empty_like(depth) if return_logits else None
    check(_launch("depth_head", 4.0 * n * h * wd * (c + 1),
                  lambda: lib.kbn_depth_head_forward(x.data_ptr(), w.data_ptr(), depth.data_ptr(),
                                                     logits.data_ptr() if return_logits else None, n, c, h, wd,
                                                     float(min_predict_depth), float(max_predict_depth),
                                                     _stream()), nbytes=4.0 * n * h * wd * (c + 1)), "kbn_depth_head_forward")
    return (depth, logits) if return_logits else depth


@_on_tensor_device
def conv_head(x, w_conv, w_out, min_predict_depth: float, max_predict_depth: float,
              negative_slope: Optional[float] = 0.2, return_logits=False, out=None):
    """deconv0's second conv + output0 + depth mapping in one launch (kbn_conv_head_forward).  Returns None when
    the shape does not qualify (channels % 4, width % 4, alignment): the caller runs the two-launch path."""
    lib = _lib.load()
    xptr, xbs = _planes(x, "x")
    n, c, h, wd = x.shape
    wc, wo = _weight(w_conv, "w_conv"), _weight(w_out, "w_out")
    if tuple(wc.shape) != (c, c, 3, 3) or tuple(wo.shape) != (1, c, 3, 3):
        raise KbnError(f"conv_head weights must be {c} x {c} x 3 x 3 and 1 x {c} x 3 x 3")
    depth = _out_tensor(out, (n, 1, h, wd), x.device)
    logits = torch.empty_like(depth) if return_logits else None
    flops = 2.0 * n * h * wd * c * 9 * c
    if not _launched("kbn_conv_head_forward", "conv_head", flops,
                     lambda: lib.kbn_conv_head_forward(xptr, xbs, wc.data_ptr(), wo.data_ptr(), depth.data_ptr(),
                                                       logits.data_ptr() if return_logits else None, n, c, h, wd,
                                                       *_act_args(negative_slope),
                                                       float(min_predict_depth), float(max_predict_depth), _stream()),
                     # 75 m-blocks of 16 positions per 64 x 16 tile, 16 filter columns, K = 9 c
                     executed=2.0 * n * (-(-h // 16)) * (-(-wd // 64)) * 75 * 16 * 16 * 9 * c, pipe="fp32",
                     nbytes=4.0 * n * h * wd * (c + 1)):
        return None
    return (depth, logits) if return_logits else depth


@_on_tensor_device
def pack_conv_tail_weight(w_conv: torch.Tensor, out: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """Blob of `conv_tail` from the raw C x C x 3 x 3 weight of deconv0's second conv (kbn_conv_tail_pack_weight); None when
    C is outside the kernel's range."""
    lib = _lib.load()
    w = _weight(w_conv, "w_conv")
    c = w.shape[0]
    nbytes = lib.kbn_conv_tail_packed_weight_bytes(c) if tuple(w.shape) == (c, c, 3, 3) else 0
    if nbytes == 0:
        return None
    return _pack_into(out, nbytes, w, lambda p: lib.kbn_conv_tail_pack_weight(w.data_ptr(), p, c, _stream()), "kbn_conv_tail_pack_weight")


@_on_tensor_device
def conv_tail(x, packed_w_conv, w_out, min_predict_depth: float, max_predict_depth: float,
              negative_slope: Optional[float] = 0.2, return_logits=False, out=None):
    """deconv0's second conv (on split fp16 operands) + output0 + depth mapping in one launch (kbn_conv_tail_forward).
    `x`: N x C x H x W fp32, or the up-conv's PairTensor of 16 channels (kbn_conv_tail_forward_pair; C = w_out's channels).
    Returns None when the shape does not qualify: the caller runs conv_head / the two-launch path."""
    lib = _lib.load()
    wo = _weight(w_out, "w_out")
    pair = isinstance(x, PairTensor)
    if pair:
        n, cp, h, wd = x.shape
        c = wo.shape[1]
        if cp != 16 or c > 16:
            return None
    else:
        xptr, xbs = _planes(x, "x")
        n, c, h, wd = x.shape
    if tuple(wo.shape) != (1, c, 3, 3):
        raise KbnError(f"conv_tail: w_out must be 1 x {c} x 3 x 3")
    depth = _out_tensor(out, (n, 1, h, wd), x.device)
    logits = torch.empty_like(depth) if return_logits else None
    flops = 2.0 * n * h * wd * c * 9 * c
    tiles = n * (-(-h // 16)) * (-(-wd // 32))
    tail_args = (packed_w_conv.data_ptr(), wo.data_ptr(), depth.data_ptr(), logits.data_ptr() if return_logits else None, n, c, h, wd,
                 *_act_args(negative_slope), float(min_predict_depth), float(max_predict_depth))
    if not _launched("kbn_conv_tail_forward", "conv_tail", flops,
                     (lambda: lib.kbn_conv_tail_forward_pair(x.data.data_ptr(), x.data.stride(0), x.scale.data_ptr(), *tail_args, _stream()))
                     if pair else (lambda: lib.kbn_conv_tail_forward(xptr, xbs, *tail_args, _stream())),
                     executed=tiles * 39 * 15 * 2.0 * 16 * 16 * 32,   # 39 pixel blocks x 15 MFMAs of 16 x 16 x 32 per tile
                     pipe="fp16", nbytes=4.0 * n * h * wd * ((16 if pair else c) + 1)):
        return None
    return (depth, logits) if return_logits else depth


# ----------------------------------------------------- fp32-grade convs on the 16-bit matrix core (split operands)
@_on_tensor_device
def pack_conv3x3_split_weight(weight: torch.Tensor, out: Optional[torch.Tensor] = None, stride: int = 1,
                              folded_up2x: bool = False, transposed: bool = False) -> torch.Tensor:
    """OIHW fp32 3x3 weight -> per-filter scaled two-term fp16 split in MFMA order for `conv3x3_split` with the same
    `stride` / `folded_up2x` (in_channels % 16 == 0).  `folded_up2x`: the sixteen 2x2 parity weights of the nearest-2x
    up-conv (sums of the 3x3 taps that read the same source pixel) instead of the nine taps.  `transposed`: `weight` is a
    ConvTranspose2d(kernel 3, stride 2, padding 1, output_padding 1) parameter (in x out x 3 x 3) and the blob is the one
    `conv3x3_split(up2x=True, folded_up2x=True, transposed=True)` reads (mode 4: the folded kernels, the layer's own taps)."""
    mode = 4 if transposed else (3 if folded_up2x else (2 if stride == 2 else 0))
    lib = _lib.load()
    w = _weight(_deconv_weight(weight) if transposed else weight)
    oc, cin, kh, kw = w.shape
    nbytes = lib.kbn_conv3x3_split_packed_weight_bytes(oc, cin, mode) if (kh, kw) == (3, 3) else 0
    if nbytes == 0:
        raise KbnError(f"conv3x3_split needs a 3x3 weight with in_channels % 16 == 0, got {tuple(w.shape)}")
    return _pack_into(out, nbytes, w, lambda p: lib.kbn_conv3x3_split_pack_weight(w.data_ptr(), p, oc, cin, mode, _stream()),
                      "kbn_conv3x3_split_pack_weight")


def act_exponent_for(amax: float) -> int:
    """The exponent the split kernels derive on the device from a frame's max |a| (sp_act_scale, csrc/conv_split.hip):
    k = 14 - floor(log2(max |a|)) puts the maximum in [2^14, 2^15) of the fp16 window (overflow at 65504); zero or
    denormal maxima take 100, Inf / NaN -100.  Host-side restatement for tests and for callers of the static
    `act_exponent` argument."""
    import struct
    b = struct.unpack("<I", struct.pack("<f", abs(amax)))[0] if amax == amax else 0x7fc00000
    return max(-100, min(100, 14 + 127 - (b >> 23)))


def conv3x3_split_executed_flops(n, cin, out_channels, height, width, stride=1, folded_up2x=False):
    """fp16 MFMA FLOPs the split kernels ISSUE (what SQ_INSTS_MFMA x 32768 counts, profiles/*/traffic.json): three
    products per fp32 product over M = 32 output pixels of a row x N = 32 filters (16 for the narrow folded up-conv)
    x K = 16 channels per instruction.  Padding that is issued: the columns of the last 32-pixel segment of a row and
    the filters of the last 32-filter block.  Padding that is NOT issued since the kernels skip it (wave-uniform tests,
    csrc/conv_split.hip): output rows below the map and 32-filter blocks that lie entirely past the last filter of a
    64- / 128-wide tile.  Folded up-conv: 16 products per low-resolution pixel instead of 36 per output pixel quad."""
    if folded_up2x:
        nblk = 16 if (out_channels <= 16 and cin % 32 == 0) else 32   # narrow layers: v_mfma_f32_16x16x32_f16, 16-pixel segments
        seg = 16 if nblk == 16 else 32
        sh, sw = height // 2, width // 2
        wide = out_channels >= 64 and (-(-out_channels // 32)) % 2 == 0     # the 64-filter tiles (csrc/conv_split.hip, uf_wide)
        if nblk == 32 and wide and sw >= 32 and 1 <= sw % 32 <= 16:
            px = sh * 32 * (sw // 32) + -(-sh // 2) * 32                     # the narrow last column on transposed tiles: blocks of two rows
        else:
            px = sh * (-(-sw // seg) * seg)
        return 3 * 2.0 * n * px * cin * 16 * (-(-out_channels // nblk) * nblk)
    if stride == 1 and width >= 32 and 1 <= width % 32 <= 16:
        # the narrow last column runs on transposed tiles (32 rows x 16 columns; csrc/conv_split.hip, TP): blocks of two rows
        px = height * 32 * (width // 32) + -(-height // 2) * 32
    else:
        px = height * (-(-width // 32) * 32)
    return 3 * 2.0 * n * px * cin * 9 * (-(-out_channels // 32) * 32)


@_on_tensor_device
def conv3x3_split(srcs: List[ConvSrc], packed_weight: torch.Tensor, n: int, out_channels: int, height: int, width: int,
                  out: torch.Tensor, up2x: bool = False, negative_slope: Optional[float] = 0.2, stride: int = 1,
                  act_exponent: int = -6, folded_up2x: bool = False, out_absmax: Optional[torch.Tensor] = None,
                  transposed: bool = False, ksplit: int = 1):
    """3x3 conv (+ LeakyReLU) of up to two concatenated tensor sources (`up2x`: of ONE source upsampled 2x, nearest;
    `stride` 2: sources are the 2x larger input planes), fp32 in / fp32 out, every product taken as three fp16 MFMAs
    over two-term splits of both operands (kbn_conv3x3_split_forward): fp32-grade accuracy at 3/16 of the fp32 MFMA's
    time.  `height` x `width` is the OUTPUT size.  The fp16 window follows the data when every source carries its absmax
    slot (tensor_src(absmax=)): per frame, on the device; only sources without slots fall back to the static
    `act_exponent` k (|a| 2^k < 65504).  `out_absmax`: slot that receives max |out| per frame.
    `folded_up2x` (with `up2x`): the folded 16-product form, weights from
    pack_conv3x3_split_weight(folded_up2x=True).  `transposed` (with both): the layer is a ConvTranspose2d(kernel 3, stride 2,
    padding 1, output_padding 1) instead -- same kernels, blob from pack_conv3x3_split_weight(transposed=True).
    `ksplit` > 1: the latency form of the plain, the stride-2 and the wide folded up-conv (kbn_conv3x3_split_forward_ksplit): every
    tile's K loop spread over `ksplit` workgroups, their partial sums added in split order by a second kernel -- for launches too small
    to fill the chip (ksplit_for); fp32 sources and an fp32 output only.  Returns None when the shape does not qualify (the caller
    stays on the fp32-MFMA kernels)."""
    if transposed and not (up2x and folded_up2x):
        raise KbnError("conv3x3_split: transposed goes with up2x and folded_up2x")
    if up2x and stride != 1:
        raise KbnError("conv3x3_split: up2x and stride 2 are mutually exclusive")
    lib = _lib.load()
    arr = (ConvSrc * len(srcs))(*srcs)
    pair = isinstance(out, PairTensor)   # the output in the producer-written split format (its slot doubles as out_absmax)
    if pair:
        optr, obs = (None, 0) if (out.sub is None or stride != 2) else _planes(out.sub, "out.sub")
        if out_absmax is None:
            out_absmax = out.absmax
    else:
        optr, obs = _planes(out, "out")
    want = (n, 16 if (pair and up2x and folded_up2x and out_channels <= 16) else out_channels, height, width)   # the narrow up-conv writes 16
    if tuple(out.shape) != want:
        raise KbnError(f"out has shape {tuple(out.shape)}, expected {want}")
    cin = sum(s.channels for s in srcs)
    flops = 2.0 * n * height * width * cin * 9 * out_channels / (4 if transposed else 1)   # transposed: nine taps per SOURCE pixel
    mode = (4 if transposed else (3 if folded_up2x else 1)) if up2x else (2 if stride == 2 else 0)
    if ksplit > 1:
        if pair or mode == 1:
            raise KbnError("conv3x3_split: ksplit goes with the plain / stride-2 / folded up-conv forms and an fp32 output")
        ws = torch.empty((ksplit, n, out_channels, height, width), device=out.device, dtype=torch.float32)
        done = _launched("kbn_conv3x3_split_forward_ksplit", ("conv_split", "", "conv_split_s2", "conv_split_upfold", "conv_split_upfold")[mode], flops,
                         lambda: lib.kbn_conv3x3_split_forward_ksplit(arr, len(srcs), packed_weight.data_ptr(), optr, obs, n, out_channels, height, width,
                                                                      mode, max(-60, min(60, int(act_exponent))), *_act_args(negative_slope),
                                                                      _slot_ptr(out_absmax, n), int(ksplit), ws.data_ptr(), _stream()),
                         executed=conv3x3_split_executed_flops(n, cin, out_channels, height, width, stride, up2x and folded_up2x),
                         pipe="fp16", nbytes=_src_bytes(srcs, n) + 4.0 * n * height * width * out_channels * (1 + 2 * ksplit))
        return out if done else None
    if not _launched("kbn_conv3x3_split_forward", ("conv_split", "conv_split_up", "conv_split_s2", "conv_split_upfold", "conv_split_upfold")[mode], flops,
                     lambda: lib.kbn_conv3x3_split_forward(arr, len(srcs), packed_weight.data_ptr(), optr, obs, n,
                                                           out_channels, height, width,
                                                           mode, max(-60, min(60, int(act_exponent))),
                                                           *_act_args(negative_slope), _slot_ptr(out_absmax, n),
                                                           out.data.data_ptr() if pair else None,
                                                           out.data.stride(0) if pair else 0,
                                                           out.scale.data_ptr() if pair else None, _stream()),
                     executed=conv3x3_split_executed_flops(n, cin, out_channels, height, width, stride, up2x and folded_up2x),
                     pipe="fp16", nbytes=_src_bytes(srcs, n) + 4.0 * n * height * width * want[1]
                     + (4.0 * n * out_channels * out.sub.shape[2] * out.sub.shape[3] if (pair and out.sub is not None and stride == 2) else 0.0)):
        return None
    return out


def ksplit_for(cin: int, out_channels: int, height: int, width: int, stride: int = 1, cus: int = 256, up2x: bool = False, frames: int = 1) -> int:
    """How many workgroups share a tile's K loop in the latency form (KBNetModel.set_latency_mode(frames=)): as many as bring a launch
    of `frames` frames to about one workgroup per CU -- every range at least two 16-channel chunks long, at most 16 -- and 1 when
    its tiles already fill half the chip or the output is large (the partial planes cost HBM traffic: 2 x ksplit x the output).  A
    function of the layer and of the MODE's `frames`, never of the batch a call happens to carry: inside a mode a frame's bits do not
    depend on what runs beside it."""
    if up2x:   # the folded up-conv: 8 x 32 low-resolution pixels x 64 filters per workgroup
        tiles = -(-(width // 2) // 32) * (-(-(height // 2) // 8)) * (-(-out_channels // 64))
    else:
        tiles = -(-width // 32) * (-(-height // (8 if stride == 2 else 16))) * (-(-out_channels // (128 if stride == 2 else 64)))
    tiles *= max(1, int(frames))
    chunks = cin // 16
    if tiles * 2 > cus or chunks < 4 or 4 * out_channels * height * width * max(1, int(frames)) > (16 << 20):
        return 1
    ks = min(16, chunks // 2, max(1, cus // tiles))
    while ks > 1 and -(-chunks // ks) * (ks - 1) >= chunks:   # no empty range
        ks -= 1
    return ks


# ----------------------------------------------------- KB block: conv_fused on split operands
@_on_tensor_device
def pack_conv1x1s2_split_weight(weight: torch.Tensor, xyz_offset: int = -1, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """OI11 fp32 weight of a 1x1 conv -> blob of `conv1x1s2_split`: per-filter scaled two-term fp16 split of the tensor
    channels in MFMA order (+ the fp32 weights of the three xyz channels that start at input channel `xyz_offset`,
    -1: the conv has none).  Tensor channels (in_channels, minus 3 with xyz) % 16 == 0."""
    lib = _lib.load()
    w = _weight(weight)
    oc, cin, kh, kw = w.shape
    has_xyz = xyz_offset >= 0
    nbytes = lib.kbn_conv1x1s2_split_packed_weight_bytes(oc, cin - (3 if has_xyz else 0), 1 if has_xyz else 0) if (kh, kw) == (1, 1) else 0
    if nbytes == 0:
        raise KbnError(f"conv1x1s2_split needs a 1x1 weight with tensor channels % 16 == 0, got {tuple(w.shape)}")
    return _pack_into(out, nbytes, w, lambda p: lib.kbn_conv1x1s2_split_pack_weight(w.data_ptr(), p, oc, cin, int(xyz_offset), _stream()),
                      "kbn_conv1x1s2_split_pack_weight")


@_on_tensor_device
def kb_xyz_s2(depth: torch.Tensor, proj_weight: torch.Tensor, kinv: torch.Tensor, negative_slope: Optional[float] = 0.2,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The KB block's backprojection K^-1 [x y 1]^T z, z = act(proj_weight . depth), at the input pixels (2y, 2x) its
    stride-2 1x1 conv reads: N x 3 x ceil(H/2) x ceil(W/2) (kbn_kb_xyz_s2_forward)."""
    lib = _lib.load()
    dptr, dbs = _planes(depth, "depth")
    n, cd, h, w = depth.shape
    oh, ow = (h + 1) // 2, (w + 1) // 2
    pw = proj_weight.detach().contiguous()
    if pw.numel() != cd or tuple(kinv.shape) != (n, 3, 3) or not kinv.is_contiguous():
        raise KbnError("kb_xyz_s2: proj_weight must hold one weight per depth channel, kinv must be a dense N x 3 x 3")
    if out is None:
        out = torch.empty((n, 3, oh, ow), device=depth.device, dtype=torch.float32)
    optr, obs = _planes(out, "xyz")
    check(_launch("kb_xyz", 2.0 * n * oh * ow * cd,
                  lambda: lib.kbn_kb_xyz_s2_forward(dptr, dbs, cd, h, w, pw.data_ptr(), kinv.data_ptr(), *_act_args(negative_slope),
                                                    optr, obs, n, _stream()), nbytes=4.0 * n * oh * ow * (cd + 3)), "kbn_kb_xyz_s2_forward")
    return out


@_on_tensor_device
def conv1x1s2_split(srcs: List[ConvSrc], packed_weight: torch.Tensor, xyz: Optional[torch.Tensor], n: int, out_channels: int,
                    height: int, width: int, out: torch.Tensor, negative_slope: Optional[float] = 0.2, act_exponent: int = -6,
                    out_absmax: Optional[torch.Tensor] = None):
    """1x1 stride-2 conv (+ LeakyReLU) of one or two tensor sources (+ the three fp32 xyz channels of `xyz`, from
    kb_xyz_s2) on split operands (kbn_conv1x1s2_split_forward); `height` x `width` is the OUTPUT size.  None when the
    shape does not qualify."""
    lib = _lib.load()
    arr = (ConvSrc * len(srcs))(*srcs)
    optr, obs = _planes(out, "out")
    if tuple(out.shape) != (n, out_channels, height, width):
        raise KbnError(f"out has shape {tuple(out.shape)}, expected {(n, out_channels, height, width)}")
    xptr, xbs = (None, 0)
    if xyz is not None:
        if tuple(xyz.shape) != (n, 3, height, width):
            raise KbnError(f"xyz has shape {tuple(xyz.shape)}, expected {(n, 3, height, width)}")
        xptr, xbs = _planes(xyz, "xyz")
    cin = sum(s.channels for s in srcs)
    flops = 2.0 * n * height * width * (cin + (3 if xyz is not None else 0)) * out_channels
    executed = 3 * 2.0 * n * (-(-height // 8) * 8) * (-(-width // 32) * 32) * cin * (-(-out_channels // 128) * 128)   # this kernel skips nothing
    if not _launched("kbn_conv1x1s2_split_forward", "conv_split_1x1s2", flops,
                     lambda: lib.kbn_conv1x1s2_split_forward(arr, len(srcs), packed_weight.data_ptr(), xptr, xbs, optr, obs, n,
                                                             out_channels, height, width, max(-60, min(60, int(act_exponent))),
                                                             *_act_args(negative_slope), _slot_ptr(out_absmax, n), _stream()),
                     executed=executed, pipe="fp16",
                     # a 1x1 stride-2 conv needs the even pixels of its sources only
                     nbytes=4.0 * n * height * width * (cin + (3 if xyz is not None else 0) + out_channels)):
        return None
    return out


# ----------------------------------------------------- encoder front: conv0_image + KB1's conv_image / conv_fused in one launch
@_on_tensor_device
def pack_kb1_front_weight(w_conv0: torch.Tensor, w_conv_image: torch.Tensor, w_conv_fused: torch.Tensor,
                          out: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """Blob of `kb1_front` (kbn_kb1_front_pack_weight) from conv0_image's weight (F0 x C x 3 x 3), the level-0 KB block's
    conv_image weight (FI x F0 x 3 x 3) and conv_fused weight (FI x (F0 + 3) x 1 x 1).  None when the shapes are outside
    the kernel's (F0 = FI = 48, C <= 4)."""
    lib = _lib.load()
    w0, wi, wf = _weight(w_conv0, "w_conv0"), _weight(w_conv_image, "w_conv_image"), _weight(w_conv_fused, "w_conv_fused")
    f0, c = w0.shape[0], w0.shape[1]
    fi = wi.shape[0]
    if tuple(w0.shape[2:]) != (3, 3) or tuple(wi.shape) != (fi, f0, 3, 3) or tuple(wf.shape) != (fi, f0 + 3, 1, 1):
        return None
    nbytes = lib.kbn_kb1_front_packed_weight_bytes(c, f0, fi)
    if nbytes == 0:
        return None
    return _pack_into(out, nbytes, w0, lambda p: lib.kbn_kb1_front_pack_weight(w0.data_ptr(), wi.data_ptr(), wf.data_ptr(), p, c, f0, fi, _stream()),
                      "kbn_kb1_front_pack_weight")


def kb1_front_supported(image_channels: int, conv0_filters: int, kb_filters: int, height: int, width: int,
                        conv0_negative_slope: float, depth_branch: bool = False) -> bool:
    """Would kb1_front (depth_branch: kb1_depth_front) take this problem?  (kbn_kb1_front_query / kbn_kb1_depth_front_query)"""
    lib = _lib.load()
    q = lib.kbn_kb1_depth_front_query if depth_branch else lib.kbn_kb1_front_query
    return q(int(image_channels), int(conv0_filters), int(kb_filters), int(height), int(width), float(conv0_negative_slope)) == _lib.KBN_OK


@_on_tensor_device
def pack_kb1_front_next_weight(w_conv_fused: torch.Tensor, image_channels: int, out: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """Blob of kb1_front's `next` stage (kbn_kb1_front_next_pack_weight) from the NEXT KB block's conv_fused weight,
    F x (image_channels + 3 + fused_channels) x 1 x 1.  None when the widths are outside the kernel's (48 + 3 + 48 -> 96)."""
    lib = _lib.load()
    wf = _weight(w_conv_fused, "w_conv_fused")
    fo, cin = wf.shape[0], wf.shape[1]
    cf = cin - 3 - image_channels
    if tuple(wf.shape[2:]) != (1, 1) or cf < 0:
        return None
    nbytes = lib.kbn_kb1_front_next_packed_weight_bytes(int(image_channels), int(cf), int(fo))
    if nbytes == 0:
        return None
    return _pack_into(out, nbytes, wf, lambda p: lib.kbn_kb1_front_next_pack_weight(wf.data_ptr(), p, int(image_channels), int(cf), int(fo), _stream()),
                      "kbn_kb1_front_next_pack_weight")


def kb1_front_next_supported(image_channels: int, conv0_filters: int, kb_filters: int, next_filters: int, height: int, width: int,
                             conv0_negative_slope: float) -> bool:
    """Would kb1_front take the next level's conv_fused along?  (kbn_kb1_front_next_query; KBN_NO_FRONT_NEXT=1 says no)"""
    return _lib.load().kbn_kb1_front_next_query(int(image_channels), int(conv0_filters), int(kb_filters), int(next_filters), int(height),
                                                int(width), float(conv0_negative_slope)) == _lib.KBN_OK


@_on_tensor_device
def kb1_front(image: torch.Tensor, packed_weight: torch.Tensor, xyz: Optional[torch.Tensor],
              conv0_filters: int, kb_filters: int, out_image: torch.Tensor, out_fused: torch.Tensor,
              conv0_negative_slope: float = 0.2, kb_negative_slope: float = 0.2, out_image_absmax=None, out_fused_absmax=None,
              next_fused=None):
    """conv0_image -> (conv_image, conv_fused) of the level-0 KB block in one launch, conv0's output kept on the CU
    (kbn_kb1_front_forward).  `xyz`: the backprojection channels from kb_xyz_s2.  None when the shape does not qualify.
    `next_fused` = (packed_next, xyz_next, out_next_fused, negative_slope, out_next_absmax): the NEXT KB level's conv_fused in the
    same launch (kbn_kb1_front_next_forward) -- its inputs are the even pixels of this launch's two outputs."""
    lib = _lib.load()
    iptr, ibs = _planes(image, "image")
    n, c, h, w = image.shape
    oh, ow = (h + 1) // 2, (w + 1) // 2
    for t, nm in ((out_image, "out_image"), (out_fused, "out_fused")):
        if tuple(t.shape) != (n, kb_filters, oh, ow):
            raise KbnError(f"{nm} has shape {tuple(t.shape)}, expected {(n, kb_filters, oh, ow)}")
    oi, oibs = _planes(out_image, "out_image")
    of, ofbs = _planes(out_fused, "out_fused")
    xptr, xbs = (None, 0)
    if xyz is not None:
        if tuple(xyz.shape) != (n, 3, oh, ow):
            raise KbnError(f"xyz has shape {tuple(xyz.shape)}, expected {(n, 3, oh, ow)}")
        xptr, xbs = _planes(xyz, "xyz")
    flops = 2.0 * n * (h * w * c * 9 * conv0_filters + oh * ow * conv0_filters * 9 * kb_filters + oh * ow * (conv0_filters + 3) * kb_filters)
    # issued fp16 MFMA FLOPs: per 8 x 16 tile and 16-filter chunk 36 x 9 (conv0) + 8 x 6 x 3 x 3 (conv_image, conv_fused) MFMAs of 16 x 16 x 32
    tiles = n * (-(-oh // 8)) * (-(-ow // 16))
    executed = tiles * (conv0_filters // 16) * (36 * 9 + 8 * 6 * (kb_filters // 16) * 3) * 2.0 * 16 * 16 * 32
    nbytes = 4.0 * n * (h * w * c + oh * ow * (2 * kb_filters + (3 if xyz is not None else 0)))
    if next_fused is None:
        call = lambda: lib.kbn_kb1_front_forward(iptr, ibs, packed_weight.data_ptr(), xptr, xbs,
                                                 oi, oibs, of, ofbs, n, c, conv0_filters, kb_filters, h, w,
                                                 float(conv0_negative_slope), float(kb_negative_slope),
                                                 _slot_ptr(out_image_absmax, n), _slot_ptr(out_fused_absmax, n), _stream())
    else:
        packed_next, xyz_next, out_next, slope_next, amax_next = next_fused
        h2, w2 = (oh + 1) // 2, (ow + 1) // 2
        fo = out_next.shape[1]
        if tuple(out_next.shape) != (n, fo, h2, w2) or tuple(xyz_next.shape) != (n, 3, h2, w2):
            raise KbnError(f"next_fused: out {tuple(out_next.shape)} / xyz {tuple(xyz_next.shape)}, expected {(n, fo, h2, w2)} / {(n, 3, h2, w2)}")
        on, onbs = _planes(out_next, "out_next_fused")
        xn, xnbs = _planes(xyz_next, "xyz_next")
        flops += 2.0 * n * h2 * w2 * (2 * kb_filters + 3) * fo
        executed += tiles * 2 * (fo // 16) * (2 * kb_filters // 32) * 3 * 2.0 * 16 * 16 * 32   # 2 pixel blocks x filter blocks x k-steps x 3 products
        nbytes += 4.0 * n * h2 * w2 * (fo + 3)
        call = lambda: lib.kbn_kb1_front_next_forward(iptr, ibs, packed_weight.data_ptr(), xptr, xbs,
                                                      oi, oibs, of, ofbs, n, c, conv0_filters, kb_filters, h, w,
                                                      float(conv0_negative_slope), float(kb_negative_slope),
                                                      _slot_ptr(out_image_absmax, n), _slot_ptr(out_fused_absmax, n),
                                                      packed_next.data_ptr(), xn, xnbs, on, onbs, fo, float(slope_next),
                                                      _slot_ptr(amax_next, n), _stream())
    if not _launched("kbn_kb1_front_forward", "kb1_front", flops, call, executed=executed, pipe="fp16", nbytes=nbytes):
        return None
    return out_image, out_fused


@_on_tensor_device
def pack_kb1_depth_front_weight(w_conv0: torch.Tensor, w_conv_depth: torch.Tensor, w_proj: torch.Tensor,
                                out: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """Blob of `kb1_depth_front` from conv0_depth's weight (16 x C x 3 x 3), the level-0 KB block's conv_depth weight
    (16 x 19 x 3 x 3) and proj_depth weight (1 x 16 x 1 x 1).  None when the shapes are outside the kernel's."""
    lib = _lib.load()
    w0, wc, wp = _weight(w_conv0, "w_conv0"), _weight(w_conv_depth, "w_conv_depth"), _weight(w_proj, "w_proj")
    f0, c = w0.shape[0], w0.shape[1]
    fd = wc.shape[0]
    if tuple(w0.shape[2:]) != (3, 3) or tuple(wc.shape) != (fd, f0 + 3, 3, 3) or wp.numel() != f0:
        return None
    nbytes = lib.kbn_kb1_depth_front_packed_weight_bytes(c, f0, fd)
    if nbytes == 0:
        return None
    return _pack_into(out, nbytes, w0, lambda p: lib.kbn_kb1_depth_front_pack_weight(w0.data_ptr(), wc.data_ptr(), wp.data_ptr(), p, c, f0, fd, _stream()),
                      "kbn_kb1_depth_front_pack_weight")


@_on_tensor_device
def kb1_depth_front(depth: torch.Tensor, kinv: torch.Tensor, packed_weight: torch.Tensor, conv0_filters: int, kb_filters: int,
                    out_depth: torch.Tensor, conv0_negative_slope: float = 0.2, kb_negative_slope: float = 0.2,
                    proj_negative_slope: Optional[float] = 0.2, out_depth_absmax=None, xyz: Optional[torch.Tensor] = None):
    """conv0_depth -> conv_depth of the level-0 KB block (coordinate channels in fp32) and the backprojection channels xyz, in
    one launch (kbn_kb1_depth_front_forward).  Returns (out_depth, xyz) or None when the shape does not qualify."""
    lib = _lib.load()
    dptr, dbs = _planes(depth, "depth")
    n, c, h, w = depth.shape
    oh, ow = (h + 1) // 2, (w + 1) // 2
    if tuple(out_depth.shape) != (n, kb_filters, oh, ow):
        raise KbnError(f"out_depth has shape {tuple(out_depth.shape)}, expected {(n, kb_filters, oh, ow)}")
    if tuple(kinv.shape) != (n, 3, 3) or not kinv.is_contiguous():
        raise KbnError("kinv must be a dense N x 3 x 3")
    _require(kinv, "kinv", 3)
    if xyz is None:
        xyz = torch.empty((n, 3, oh, ow), device=depth.device, dtype=torch.float32)
    optr, obs = _planes(out_depth, "out_depth")
    xptr, xbs = _planes(xyz, "xyz")
    flops = 2.0 * n * (h * w * c * 9 * conv0_filters + oh * ow * ((conv0_filters + 3) * 9 * kb_filters + conv0_filters))
    tiles = n * (-(-oh // 8)) * (-(-ow // 16))
    executed = tiles * (36 * 9 + 8 * 15) * 2.0 * 16 * 16 * 32
    if not _launched("kbn_kb1_depth_front_forward", "kb1_depth_front", flops,
                     lambda: lib.kbn_kb1_depth_front_forward(dptr, dbs, kinv.data_ptr(), packed_weight.data_ptr(), optr, obs, xptr, xbs,
                                                             n, c, conv0_filters, kb_filters, h, w, float(conv0_negative_slope),
                                                             float(kb_negative_slope), *_act_args(proj_negative_slope),
                                                             _slot_ptr(out_depth_absmax, n), _stream()),
                     executed=executed, pipe="fp16", nbytes=4.0 * n * (h * w * c + oh * ow * (kb_filters + 3))):
        return None
    return out_depth, xyz


# ----------------------------------------------------- S2D -> conv0_depth -> KB1's depth branch in one launch
@_on_tensor_device
def pack_s2d_depth_front_weight(w_pool_convs: List[torch.Tensor], w_conv: torch.Tensor, out: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """Blob of the on-chip S2D stage of `s2d_depth_front` (kbn_s2d_depth_front_pack_weight) from SparseToDensePool's weights:
    pool_convs.{0,1,2}.conv.weight and conv.conv.weight.  None when the shapes are outside the kernel's (three 1x1 layers of 8
    filters, a 3x3 conv over 8 + 2 channels)."""
    lib = _lib.load()
    if len(w_pool_convs) != 3:
        return None
    ws = [_weight(w) for w in w_pool_convs]
    wc = _weight(w_conv)
    npool = ws[0].shape[1]
    if (tuple(ws[0].shape) != (8, npool, 1, 1) or tuple(ws[1].shape) != (8, 8, 1, 1) or tuple(ws[2].shape) != (8, 8, 1, 1)
            or tuple(wc.shape) != (8, 10, 3, 3)):
        return None
    nbytes = lib.kbn_s2d_depth_front_packed_weight_bytes(npool)
    if nbytes == 0:
        return None
    return _pack_into(out, nbytes, wc, lambda p: lib.kbn_s2d_depth_front_pack_weight(ws[0].data_ptr(), ws[1].data_ptr(), ws[2].data_ptr(), wc.data_ptr(),
                                                                                     p, npool, _stream()), "kbn_s2d_depth_front_pack_weight")


def s2d_depth_front_supported(input_channels: int, min_pool_sizes, max_pool_sizes, n_convolution: int, n_filter: int, conv0_filters: int,
                              kb_filters: int, height: int, width: int, s2d_negative_slope: float, conv0_negative_slope: float) -> bool:
    """Would `s2d_depth_front` take this problem?  (kbn_s2d_depth_front_query: pool preset, widths, slopes, switches)"""
    mins = [int(k) for k in min_pool_sizes if k > 1]
    maxs = [int(k) for k in max_pool_sizes if k > 1]
    return _lib.load().kbn_s2d_depth_front_query(int(input_channels), _int_array(mins), len(mins), _int_array(maxs), len(maxs), int(n_convolution),
                                                 int(n_filter), int(conv0_filters), int(kb_filters), int(height), int(width),
                                                 float(s2d_negative_slope), float(conv0_negative_slope)) == _lib.KBN_OK


@_on_tensor_device
def s2d_depth_front(x: torch.Tensor, kinv: torch.Tensor, packed_s2d: torch.Tensor, packed_weight: torch.Tensor, min_pool_sizes, max_pool_sizes,
                    conv0_filters: int, kb_filters: int, out_depth: torch.Tensor, s2d_negative_slope: float = 0.2,
                    conv0_negative_slope: float = 0.2, kb_negative_slope: float = 0.2, proj_negative_slope: Optional[float] = 0.2,
                    out_depth_absmax=None, xyz: Optional[torch.Tensor] = None):
    """SparseToDensePool -> conv0_depth -> conv_depth of the level-0 KB block and the backprojection channels xyz in ONE launch
    (kbn_s2d_depth_front_forward): `x` = N x 2 x H x W [sparse depth, validity]; the S2D tensor stays on the CU.  Returns
    (out_depth, xyz) or None when the problem does not qualify (the caller runs s2d_forward + kb1_depth_front)."""
    lib = _lib.load()
    xptr, xbs = _planes(x, "x")
    n, c, h, w = x.shape
    oh, ow = (h + 1) // 2, (w + 1) // 2
    if tuple(out_depth.shape) != (n, kb_filters, oh, ow):
        raise KbnError(f"out_depth has shape {tuple(out_depth.shape)}, expected {(n, kb_filters, oh, ow)}")
    if tuple(kinv.shape) != (n, 3, 3) or not kinv.is_contiguous():
        raise KbnError("kinv must be a dense N x 3 x 3")
    _require(kinv, "kinv", 3)
    if xyz is None:
        xyz = torch.empty((n, 3, oh, ow), device=x.device, dtype=torch.float32)
    optr, obs = _planes(out_depth, "out_depth")
    zptr, zbs = _planes(xyz, "xyz")
    mins = [int(k) for k in min_pool_sizes if k > 1]
    maxs = [int(k) for k in max_pool_sizes if k > 1]
    npool = len(mins) + len(maxs)
    nf = 8
    # the reference's work for the three layers (S2D at full resolution, conv0_depth, conv_depth + proj at half resolution)
    flops = 2.0 * n * (h * w * (npool * nf + 2 * nf * nf + 9 * (nf + c) * nf + nf * 9 * conv0_filters)
                       + oh * ow * ((conv0_filters + 3) * 9 * kb_filters + conv0_filters))
    tiles = n * (-(-oh // 8)) * (-(-ow // 16))
    executed = tiles * (27 * 6 + 22 * 12 + 36 * 9 + 8 * 15) * 2.0 * 16 * 16 * 32   # chain, 3x3 pairs, conv0, conv_depth: MFMAs of 16 x 16 x 32 per tile
    amin, amax = _int_array(mins), _int_array(maxs)
    if not _launched("kbn_s2d_depth_front_forward", "s2d_depth_front", flops,
                     lambda: lib.kbn_s2d_depth_front_forward(xptr, xbs, kinv.data_ptr(), packed_s2d.data_ptr(), packed_weight.data_ptr(), optr, obs,
                                                             zptr, zbs, n, c, amin, len(mins), amax, len(maxs), 3, nf, conv0_filters, kb_filters,
                                                             h, w, float(s2d_negative_slope), float(conv0_negative_slope), float(kb_negative_slope),
                                                             *_act_args(proj_negative_slope), _slot_ptr(out_depth_absmax, n), _stream()),
                     executed=executed, pipe="fp16", nbytes=4.0 * n * (h * w * c + oh * ow * (kb_filters + 3))):
        return None
    return out_depth, xyz


# ------------------------------------------------------- pre-model stage / evaluation
@_on_tensor_device
def preprocess(image, sparse_depth, kernel_size: int = 7, threshold: float = 1.5, normalize_image: bool = True,
               normalized_image_range=(0, 1)):
    """Validity map + outlier removal (+ image normalisation): what reference src/kbnet.py:899-912 does
    before calling the model.  `normalized_image_range` as run_kbnet.py --normalized_image_range (reference
    src/transforms.py:185-214): [0, 1] image / 255, [-1, 1] 2 (image / 255) - 1, [0, 255] the image as it came (the reference returns
    its input for that range), anything else ValueError.  Returns (image, filtered_validity, filtered_sparse); image is None only
    with normalize_image=False (the caller keeps its own tensor) or when none was passed."""
    rng = [float(v) for v in normalized_image_range]
    untouched = rng == [0.0, 255.0]
    if untouched:
        normalize_image = False
    elif rng not in ([0.0, 1.0], [-1.0, 1.0]):
        raise ValueError("Unsupported normalization range: {}".format(list(normalized_image_range)))
    lib = _lib.load()
    _require(sparse_depth, "sparse_depth", 4)
    sd = sparse_depth.contiguous()
    n, _, h, w = sd.shape
    img = out_img = None
    c = 0
    if image is not None and normalize_image:
        _require(image, "image", 4)
        img = image.contiguous()
        c = img.shape[1]
        out_img = torch.empty_like(img)
    validity = torch.empty_like(sd)
    filtered = torch.empty_like(sd)
    ws = torch.empty(1, device=sd.device, dtype=torch.int32)
    check(lib.kbn_preprocess_forward(img.data_ptr() if img is not None else None, sd.data_ptr(),
                                     out_img.data_ptr() if out_img is not None else None, validity.data_ptr(),
                                     filtered.data_ptr(), ws.data_ptr(), 4, n, c, h, w, int(kernel_size),
                                     float(threshold), 1 if rng == [-1.0, 1.0] else 0, _stream()), "kbn_preprocess_forward")
    if untouched and image is not None:
        out_img = image.contiguous()
    return out_img, validity, filtered


@_on_tensor_device
def unpack_frames(image_u8, depth_raw, width: Optional[int] = None, x_offset: int = 0):
    """Decoded PNG pixels on the device -> (image N x 3 x H x W float32 in 0..255, sparse depth
    N x 1 x H x W float32 = raw / 256): the tensors reference src/datasets.py:259-283 returns.
    image_u8: N x H x Wraw x C uint8 (C in 1, 3, 4) or None; `width` / `x_offset` select the columns (the
    middle third of a triplet: width = Wraw // 3, x_offset = width).  depth_raw: N x H x W int16 (bit
    pattern of the 16-bit PNG samples) or uint8, or None."""
    lib = _lib.load()
    if image_u8 is None and depth_raw is None:
        raise KbnError("unpack_frames: nothing to unpack")
    image = depth = None
    n = h = wraw = c = 0
    if image_u8 is not None:
        if not image_u8.is_cuda or image_u8.dtype != torch.uint8 or image_u8.dim() != 4:
            raise KbnError("image_u8: expected a CUDA/HIP uint8 tensor N x H x W x C")
        image_u8 = image_u8.contiguous()
        n, h, wraw, c = image_u8.shape
        if width is None:
            width = wraw
        image = torch.empty((n, 3, h, width), device=image_u8.device, dtype=torch.float32)
    bits = 16
    if depth_raw is not None:
        if not depth_raw.is_cuda or depth_raw.dim() != 3 or depth_raw.dtype not in (torch.int16, torch.uint8):
            raise KbnError("depth_raw: expected a CUDA/HIP int16 (16-bit samples) or uint8 tensor N x H x W")
        depth_raw = depth_raw.contiguous()
        bits = 16 if depth_raw.dtype == torch.int16 else 8
        if image_u8 is not None and (depth_raw.shape[0] != n or depth_raw.shape[1] != h or depth_raw.shape[2] != width):
            raise KbnError(f"depth_raw has shape {tuple(depth_raw.shape)}, expected {(n, h, width)}")
        n, h, width = depth_raw.shape
        depth = torch.empty((n, 1, h, width), device=depth_raw.device, dtype=torch.float32)
    check(lib.kbn_unpack_frames_forward(image_u8.data_ptr() if image_u8 is not None else None,
                                        depth_raw.data_ptr() if depth_raw is not None else None,
                                        image.data_ptr() if image is not None else None,
                                        depth.data_ptr() if depth is not None else None,
                                        n, h, width, wraw if image_u8 is not None else width, int(x_offset),
                                        c if image_u8 is not None else 3, bits, _stream()), "kbn_unpack_frames_forward")
    return image, depth


@_on_tensor_device
def export_pack(image=None, depth_a=None, depth_b=None, scale: float = 255.0, shift: float = 0.0, out=None):
    """The pixels of a batch's output files in ONE launch (kbn_export_pack_forward, csrc/export_pack.hip) -> (rgb, samples_a,
    samples_b), None where the source was None:
      image N x 3 x H x W fp32 -> rgb N x H x W x 3 uint8, interleaved: clamp(trunc(scale * v + shift), 0, 255), NaN -> 0, product and
        sum each rounded to fp32.  (255, 0) on a [0, 1] image is the reference's `(255 * image).astype(np.uint8)` (src/kbnet.py:1015);
        (127.5, 127.5) serves a [-1, 1] image, (1, 0) a [0, 255] one.
      depth_a, depth_b N x 1 x H x W (or N x H x W) fp32 -> N x H x W int16 holding the uint16 bit patterns min(trunc(z * 256), 65535),
        NaN and negatives 0 -- loader.depth_samples' values (view the host copy as np.uint16).
    Inputs are made dense here.  `out`: (rgb, samples_a, samples_b) to write into -- dense device tensors of those shapes and
    dtypes, views of larger buffers welcome, None where the source is None.  CPU tensors raise KbnError (no CPU fallback), so do
    shapes that disagree, naming the offender."""
    fn = "export_pack"
    given = [("image", image), ("depth_a", depth_a), ("depth_b", depth_b)]
    if all(t is None for _, t in given):
        raise KbnError(f"{fn}: nothing to pack")
    dense, shape = [], None
    for name, t in given:
        if t is None:
            dense.append(None)
            continue
        _require(t, f"{fn}: {name}")
        t = t.detach()
        if name == "image":
            if t.dim() != 4 or t.shape[1] != 3:
                raise KbnError(f"{fn}: image has shape {tuple(t.shape)}, expected N x 3 x H x W")
            nhw = (t.shape[0], t.shape[2], t.shape[3])
        else:
            if t.dim() == 4 and t.shape[1] == 1:
                nhw = (t.shape[0], t.shape[2], t.shape[3])
            elif t.dim() == 3:
                nhw = tuple(t.shape)
            else:
                raise KbnError(f"{fn}: {name} has shape {tuple(t.shape)}, expected N x 1 x H x W or N x H x W")
        if shape is None:
            shape, first = nhw, name
        elif nhw != shape:
            raise KbnError(f"{fn}: {name} has shape {tuple(t.shape)}: its N, H, W {nhw} differ from {first}'s {shape}")
        dense.append(t.contiguous())
    n, h, w = (int(v) for v in shape)
    if n < 1 or h < 1 or w < 1:
        raise KbnError(f"{fn}: empty batch or frame ({n} x {h} x {w})")
    device = next(t for t in dense if t is not None).device
    want = [((n, h, w, 3), torch.uint8), ((n, h, w), torch.int16), ((n, h, w), torch.int16)]
    if out is None:
        out = (None, None, None)
    if len(out) != 3:
        raise KbnError(f"{fn}: out is (rgb, samples_a, samples_b), got {len(out)} entries")
    outs = []
    for (name, _), src, o, (oshape, dtype), oname in zip(given, dense, out, want, ("rgb", "samples_a", "samples_b")):
        if src is None:
            if o is not None:
                raise KbnError(f"{fn}: out has {oname} but no {name} was passed")
            outs.append(None)
        elif o is None:
            outs.append(torch.empty(oshape, device=device, dtype=dtype))
        else:
            if not isinstance(o, torch.Tensor) or not o.is_cuda or o.device != device:
                raise KbnError(f"{fn}: out {oname}: expected a tensor on {device} (the HIP path has no CPU fallback)")
            if o.dtype != dtype or tuple(o.shape) != oshape or not o.is_contiguous():
                raise KbnError(f"{fn}: out {oname} is {o.dtype} {tuple(o.shape)}, expected a contiguous {dtype} {oshape}")
            outs.append(o)
    ptr = [t.data_ptr() if t is not None else None for t in dense + outs]
    lib = _lib.load()
    sources = sum(1 for t in dense[1:] if t is not None)
    check(_launch("export_pack", 0.0,
                  lambda: lib.kbn_export_pack_forward(ptr[0], float(scale), float(shift), ptr[1], ptr[2], ptr[3], ptr[4], ptr[5], n, h, w, _stream()),
                  nbytes=float(n * h * w) * ((15 if dense[0] is not None else 0) + 6 * sources)), "kbn_export_pack_forward")
    return tuple(outs)


def pack_frames_stride(height: int, width: int, channels: int, bits: int) -> int:
    """Bytes of one frame's slot in pack_frames' `out` (kbn_pack_frames_stride: the encoder's bound rounded up to 16); raises
    KbnError for sizes the device encoder refuses."""
    stride = int(_lib.load().kbn_pack_frames_stride(int(width), int(height), int(channels), int(bits)))
    if stride == 0:
        raise KbnError(f"pack_frames: {height} x {width} x {channels} samples of {bits} bits cannot be packed on the device (channels 1, 3 "
                       f"or 4, bits 8 or 16, sizes >= 1, width <= {_lib.KBN_PACK_FRAMES_MAX_WIDTH}, an encoding below 4 GiB)")
    return stride


def pack_frames_workspace_bytes(n: int, height: int, width: int, channels: int, bits: int) -> int:
    """Device bytes pack_frames needs as `workspace` for n such frames (kbn_pack_frames_workspace_bytes)."""
    pack_frames_stride(height, width, channels, bits)
    need = int(_lib.load().kbn_pack_frames_workspace_bytes(int(n), int(width), int(height), int(channels), int(bits)))
    if need == 0:      # a refusal, not "no workspace"
        raise KbnError(f"pack_frames: no workspace for {n} frames")
    return need


@_on_tensor_device
def pack_frames(samples, bits=None, out=None, out_bytes=None, workspace=None):
    """The packed files of a batch of frames, encoded ON THE DEVICE (kbn_pack_frames_forward, csrc/pack_frames.hip) ->
    (out, out_bytes): out[i, :out_bytes[i]] is byte for byte loader.encode_frame of frame i.
      samples   N x H x W x C uint8 (C = 1, 3, 4), N x H x W uint8 or int16, or N x H x W x C int16 -- int16 holding the uint16 bit
                patterns, as export_pack returns them; dense, on the device
      bits      8 or 16, by default what the dtype says
      out       N x stride uint8, stride a multiple of 16 and >= pack_frames_stride(H, W, C, bits), 16-byte aligned, rows dense;
                a view of a larger buffer is welcome.  Bytes past out_bytes[i] keep what they held.
      out_bytes N int64 on the device: the sizes are known to the device alone, no host synchronisation here
      workspace a dense uint8 device tensor of at least pack_frames_workspace_bytes(...) bytes; allocated when None
    Three launches, whatever N is.  CPU tensors raise KbnError (no CPU fallback), so do shapes and dtypes that disagree, naming the
    offender."""
    fn = "pack_frames"
    if not isinstance(samples, torch.Tensor) or not samples.is_cuda:
        raise KbnError(f"{fn}: samples: expected a CUDA/HIP tensor (the HIP path has no CPU fallback)")
    t = samples.detach()
    if t.dtype not in (torch.uint8, torch.int16) or t.dim() not in (3, 4):
        raise KbnError(f"{fn}: samples is {t.dtype} {tuple(t.shape)}, expected N x H x W (x C) uint8 or int16 (uint16 bit patterns)")
    want_bits = 8 if t.dtype == torch.uint8 else 16
    if bits is not None and int(bits) != want_bits:
        raise KbnError(f"{fn}: bits {bits} with {t.dtype} samples (uint8 holds 8 bits, int16 the uint16 patterns of 16)")
    n, h, w = (int(v) for v in t.shape[:3])
    c = int(t.shape[3]) if t.dim() == 4 else 1
    if n < 1 or h < 1 or w < 1 or c < 1:
        raise KbnError(f"{fn}: samples is empty: {tuple(t.shape)}")
    if c not in (1, 3, 4):
        raise KbnError(f"{fn}: samples has {c} channels, expected 1, 3 or 4")
    t = t.contiguous()
    device = t.device
    stride = pack_frames_stride(h, w, c, want_bits)
    if out is None:
        out = torch.empty((n, stride), device=device, dtype=torch.uint8)
    else:
        if not isinstance(out, torch.Tensor) or not out.is_cuda or out.device != device:
            raise KbnError(f"{fn}: out: expected a tensor on {device} (the HIP path has no CPU fallback)")
        if out.dtype != torch.uint8 or out.dim() != 2 or out.shape[0] != n or out.stride(1) != 1:
            raise KbnError(f"{fn}: out is {out.dtype} {tuple(out.shape)}, expected uint8 {n} x stride with dense rows")
        if out.shape[1] < stride or out.shape[1] % 16 or (n > 1 and (out.stride(0) % 16 or out.stride(0) < out.shape[1])):
            raise KbnError(f"{fn}: out is {tuple(out.shape)} with rows {out.stride(0)} bytes apart: a slot is a multiple of 16 bytes and at least {stride}")
        if out.data_ptr() % 16:
            raise KbnError(f"{fn}: out is not 16-byte aligned")
    out_stride = int(out.stride(0)) if n > 1 else int(out.shape[1])
    if out_bytes is None:
        out_bytes = torch.empty((n,), device=device, dtype=torch.int64)
    elif (not isinstance(out_bytes, torch.Tensor) or not out_bytes.is_cuda or out_bytes.device != device or out_bytes.dtype != torch.int64
          or tuple(out_bytes.shape) != (n,) or not out_bytes.is_contiguous()):
        raise KbnError(f"{fn}: out_bytes: expected a contiguous int64 tensor of {n} on {device}")
    lib = _lib.load()
    need = int(lib.kbn_pack_frames_workspace_bytes(n, w, h, c, want_bits))
    if need == 0:      # a refusal, not "no workspace"
        raise KbnError(f"{fn}: no workspace for {n} frames of {h} x {w} x {c} samples")
    if workspace is None:
        workspace = torch.empty((need,), device=device, dtype=torch.uint8)
    elif (not isinstance(workspace, torch.Tensor) or not workspace.is_cuda or workspace.device != device or workspace.dtype != torch.uint8
          or not workspace.is_contiguous() or workspace.numel() < need):
        raise KbnError(f"{fn}: workspace: expected a dense uint8 tensor of at least {need} bytes on {device}")
    check(_launch("pack_frames", 0.0,
                  lambda: lib.kbn_pack_frames_forward(t.data_ptr(), n, w, h, c, want_bits, out.data_ptr(), out_stride, out_bytes.data_ptr(),
                                                      workspace.data_ptr(), workspace.numel(), _stream()),
                  nbytes=float(n * h * w * c) * (want_bits // 8) * 3.0), "kbn_pack_frames_forward")
    return out, out_bytes


POINT_RECORD_BYTES = {False: 12, True: 15}      # a PLY vertex: float x, y, z, and with colour uchar r, g, b; packed


def point_cloud_stride(height: int, width: int, colour: bool) -> int:
    """Bytes of one frame's slot in point_cloud's `out`: a record for every pixel (12 bytes, 15 with colour)."""
    height, width = int(height), int(width)
    if height < 1 or width < 1 or height * width > 0x7fffffff:
        raise KbnError(f"point_cloud: {height} x {width} pixels (sizes >= 1, at most 2^31 - 1 pixels a frame)")
    return height * width * POINT_RECORD_BYTES[bool(colour)]


def point_cloud_workspace_bytes(n: int, height: int, width: int) -> int:
    """Device bytes point_cloud needs as `workspace` for n such frames (kbn_point_cloud_workspace_bytes)."""
    need = int(_lib.load().kbn_point_cloud_workspace_bytes(int(n), int(height), int(width)))
    if need == 0:      # a refusal, not "no workspace"
        raise KbnError(f"point_cloud: no workspace for {n} frames of {height} x {width}")
    return need


@_on_tensor_device
def point_cloud(depth, intrinsics_inverse, image=None, *, min_depth: float = 0.0, max_depth: float = float("inf"), scale: float = 255.0,
                shift: float = 0.0, out=None, out_points=None, workspace=None):
    """A batch of depth maps backprojected to the vertex records of binary PLY files ON THE DEVICE (kbn_point_cloud_forward,
    csrc/point_cloud.hip) -> (records, points): records[i, :points[i] * record] holds frame i's kept pixels in row-major
    order as packed little-endian `float x, y, z` (12 bytes), followed by `uchar r, g, b` when an image is given (15 bytes).
      depth               N x 1 x H x W fp32 with dense planes (a channel slice of a wider tensor is welcome), or N x H x W
      intrinsics_inverse  N x 3 x 3 fp32: ops.intrinsics_inverse(K).  A point is ops.camera_coordinates' value times the depth,
                          one fp32 product a component
      image               None, or N x 3 x H x W fp32: the normalised image; the colour bytes are export_pack's under `scale` and
                          `shift` (loader.image_export_affine), i.e. the image file's pixels
      min_depth, max_depth  the closed range of kept depths; NaN, +-Inf, zero and negatives are never kept
      out        N x stride uint8 with dense rows, stride >= point_cloud_stride(H, W, image is not None); a view of a larger buffer
                 is welcome.  Bytes past points[i] * record keep what they held.
      out_points N int64 on the device: the counts are known to the device alone, no host synchronisation here
      workspace  a dense uint8 device tensor of at least point_cloud_workspace_bytes(N, H, W) bytes; allocated when None
    Three launches, whatever N is.  CPU tensors raise KbnError (no CPU fallback), so do shapes and dtypes that disagree, naming the
    offender."""
    fn = "point_cloud"
    _require(depth, f"{fn}: depth")
    d = depth.detach()
    if d.dim() == 3:
        d = d.unsqueeze(1)
    if d.dim() != 4 or d.shape[1] != 1:
        raise KbnError(f"{fn}: depth has shape {tuple(depth.shape)}, expected N x 1 x H x W or N x H x W")
    n, h, w = int(d.shape[0]), int(d.shape[2]), int(d.shape[3])
    if n < 1 or h < 1 or w < 1:
        raise KbnError(f"{fn}: depth is empty: {tuple(depth.shape)}")
    if d.stride(3) != 1 or d.stride(2) != w or (n > 1 and d.stride(0) < h * w):
        d = d.contiguous()
    device = d.device
    _require(intrinsics_inverse, f"{fn}: intrinsics_inverse")
    if tuple(intrinsics_inverse.shape) != (n, 3, 3):
        raise KbnError(f"{fn}: intrinsics_inverse has shape {tuple(intrinsics_inverse.shape)}, expected {(n, 3, 3)}")
    kinv = intrinsics_inverse.detach().contiguous()
    colour = image is not None
    if colour:
        _require(image, f"{fn}: image")
        if tuple(image.shape) != (n, 3, h, w):
            raise KbnError(f"{fn}: image has shape {tuple(image.shape)}, expected {(n, 3, h, w)} like depth")
        image = image.detach().contiguous()
    record = POINT_RECORD_BYTES[colour]
    stride = point_cloud_stride(h, w, colour)
    if out is None:
        out = torch.empty((n, stride), device=device, dtype=torch.uint8)
    else:
        if not isinstance(out, torch.Tensor) or not out.is_cuda or out.device != device:
            raise KbnError(f"{fn}: out: expected a tensor on {device} (the HIP path has no CPU fallback)")
        if out.dtype != torch.uint8 or out.dim() != 2 or out.shape[0] != n or out.stride(1) != 1:
            raise KbnError(f"{fn}: out is {out.dtype} {tuple(out.shape)}, expected uint8 {n} x stride with dense rows")
        if out.shape[1] < stride or (n > 1 and out.stride(0) < out.shape[1]):
            raise KbnError(f"{fn}: out is {tuple(out.shape)} with rows {out.stride(0)} bytes apart: a slot is at least {stride} bytes")
    out_stride = int(out.stride(0)) if n > 1 else int(out.shape[1])
    if out_points is None:
        out_points = torch.empty((n,), device=device, dtype=torch.int64)
    elif (not isinstance(out_points, torch.Tensor) or not out_points.is_cuda or out_points.device != device or out_points.dtype != torch.int64
          or tuple(out_points.shape) != (n,) or not out_points.is_contiguous()):
        raise KbnError(f"{fn}: out_points: expected a contiguous int64 tensor of {n} on {device}")
    need = point_cloud_workspace_bytes(n, h, w)
    if workspace is None:
        workspace = torch.empty((need,), device=device, dtype=torch.uint8)
    elif (not isinstance(workspace, torch.Tensor) or not workspace.is_cuda or workspace.device != device or workspace.dtype != torch.uint8
          or not workspace.is_contiguous() or workspace.numel() < need):
        raise KbnError(f"{fn}: workspace: expected a dense uint8 tensor of at least {need} bytes on {device}")
    lib = _lib.load()
    batch_stride = int(d.stride(0)) if n > 1 else h * w
    # algorithmic bytes: the depth read twice (count, emit), the image once, a record written per pixel at most
    check(_launch("point_cloud", 0.0,
                  lambda: lib.kbn_point_cloud_forward(d.data_ptr(), batch_stride, image.data_ptr() if colour else None, float(scale),
                                                      float(shift), kinv.data_ptr(), float(min_depth), float(max_depth), n, h, w,
                                                      out.data_ptr(), out_stride, out_points.data_ptr(), workspace.data_ptr(),
                                                      workspace.numel(), _stream()),
                  nbytes=float(n * h * w) * (8 + (12 if colour else 0) + record)), "kbn_point_cloud_forward")
    return out, out_points


_TRAIN_FRAME_RECORD = struct.Struct("@2q4i")     # _lib.TrainFrame's layout: two byte offsets, raw height, raw width, y_start, x_start
_PACKED_FRAME_RECORD = struct.Struct("@2q2I4i")     # _lib.PackedFrame's layout: two byte offsets, two file sizes, raw height, raw width, y_start, x_start
_SEQUENCE_FRAME_RECORD = struct.Struct("@4q4i")     # _lib.SequenceFrame's layout: three image offsets, the depth offset, height, width, y_start, x_start
_PACKED_SEQUENCE_FRAME_RECORD = struct.Struct("@4q4I4i")     # _lib.PackedSequenceFrame's layout: four byte offsets, four file sizes, height, width, y_start, x_start


def _unpack_records(fn, images_u8, depths_u8, frames, shape, channels, depth_bits, record, fields, place, max_raw_width=None, align=1,
                    thirds=3):
    """What the unpack_*_frames wrappers (`fn`) check, in one order: the arguments, then every frame, then where the
    tensors live -- a wrong frame is named on a machine without a GPU too.  `record`: the struct of one frame, its last four fields
    H, `thirds` x W, y_start, x_start (thirds 3: the record of a triplet file holds its raw width; 1: the sequence records hold a
    frame's); `fields`: the entries of a frame tuple, which end with H, W, y_start, x_start; `place(i, frame)` checks
    where the frame lies in the two buffers and returns the record's leading fields.  Returns h, w, frames, n and the records."""
    h, w = (int(v) for v in shape)
    if h < 1 or w < 1:
        raise KbnError(f"{fn}: the crop shape must be positive, got {h} x {w}")
    if channels not in (1, 3, 4):
        raise KbnError(f"{fn}: image channels must be 1, 3 or 4, got {channels}")
    if depth_bits not in (8, 16):
        raise KbnError(f"{fn}: depth samples must have 8 or 16 bits, got {depth_bits}")
    frames = [tuple(int(v) for v in f) for f in frames]
    n = len(frames)
    if n < 1:
        raise KbnError(f"{fn}: no frames")
    for name, t in (("images_u8", images_u8), ("depths_u8", depths_u8)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 1 or not t.is_contiguous():
            raise KbnError(f"{fn}: {name}: expected a dense 1-d uint8 tensor")
    records = bytearray(record.size * n)
    for i, f in enumerate(frames):
        if len(f) != fields.count(",") + 1:
            raise KbnError(f"{fn}: frame {i}: expected ({fields}), got {f}")
        H, W, y, x = f[-4:]
        if H < 1 or W < 1 or thirds * W > 0x7fffffff:
            raise KbnError(f"{fn}: frame {i}: raw size {H} x {W}")
        if max_raw_width is not None and thirds * W > max_raw_width:
            raise KbnError(f"{fn}: frame {i}: a packed {'triplet' if thirds == 3 else 'frame'} of {thirds * W} columns is wider than the kernel takes ({max_raw_width})")
        if y < 0 or y + h > H or x < 0 or x + w > W:
            raise KbnError(f"{fn}: frame {i}: the {h} x {w} crop at ({y}, {x}) leaves the {H} x {W} frame")
        record.pack_into(records, i * record.size, *place(i, f), H, thirds * W, y, x)
    for name, t in (("images_u8", images_u8), ("depths_u8", depths_u8)):
        if not t.is_cuda:
            raise KbnError(f"{fn}: {name}: expected a CUDA/HIP tensor (the HIP path has no CPU fallback)")
        if t.data_ptr() % align:
            raise KbnError(f"{fn}: {name}: the buffer must be {align}-byte aligned")
    if depths_u8.device != images_u8.device:
        raise KbnError(f"{fn}: tensors live on different devices ({images_u8.device} and {depths_u8.device})")
    return h, w, frames, n, records


def unpack_train_frames(images_u8, depths_u8, frames, shape, channels: int = 3, depth_bits: int = 16):
    """The decoded bytes of a batch of image triplets and depth maps on the device -> (image0, image1, image2, sparse_depth0): what
    the reference's KBNetTrainingDataset.__getitem__ returns (src/datasets.py:199-225), batched -- the images (t, t-1, t+1; the
    middle, left and right third of the triplet) N x 3 x h x w float32 in 0..255, the depth N x 1 x h x w float32 = sample / 256
    (kbn_unpack_train_frames_forward, csrc/unpack_train.hip: one launch per _lib.KBN_UNPACK_TRAIN_MAX_FRAMES frames).

    images_u8 / depths_u8: packed 1-d uint8 device buffers.  frames: one (image_offset, depth_offset, H, W, y_start, x_start) a
    frame -- the byte offsets of its H x 3 W x channels triplet and of its H x W depth samples (uint16 in host byte order for
    depth_bits 16, uint8 for 8) in the two buffers, and where its crop starts inside each third.  Frames may differ in size;
    shape = (h, w) is the crop of all of them (output pixel (y, x) is raw pixel (y_start + y, x_start + x)).  channels in 1, 3, 4
    (gray is replicated, alpha dropped).  What is wrong with a frame raises KbnError naming it; CPU tensors raise, there is no
    CPU fallback.  The records travel in the kernel arguments: nothing is allocated but the outputs, nothing copied, no wait."""
    fn = "unpack_train_frames"
    channels, depth_bits = int(channels), int(depth_bits)

    def place(i, f):
        io, do, H, W = f[:4]
        if io < 0 or io + H * 3 * W * channels > images_u8.numel():
            raise KbnError(f"{fn}: frame {i}: its {H} x {3 * W} x {channels} triplet at byte {io} leaves the image buffer of {images_u8.numel()} bytes")
        if do < 0 or do % (depth_bits // 8) or do + H * W * (depth_bits // 8) > depths_u8.numel():
            raise KbnError(f"{fn}: frame {i}: its {H} x {W} depth map of {depth_bits}-bit samples at byte {do} is misaligned or leaves "
                           f"the depth buffer of {depths_u8.numel()} bytes")
        return io, do

    h, w, frames, n, records = _unpack_records(fn, images_u8, depths_u8, frames, shape, channels, depth_bits, _TRAIN_FRAME_RECORD,
                                               "image_offset, depth_offset, H, W, y_start, x_start", place)
    device = images_u8.device
    image0, image1, image2 = (torch.empty((n, 3, h, w), device=device, dtype=torch.float32) for _ in range(3))
    depth = torch.empty((n, 1, h, w), device=device, dtype=torch.float32)
    lib = _lib.load()
    table = (_lib.TrainFrame * n).from_buffer(records)
    with torch.cuda.device(device):
        check(_launch("unpack_train_frames", 0.0,
                      lambda: lib.kbn_unpack_train_frames_forward(images_u8.data_ptr(), images_u8.numel(), depths_u8.data_ptr(), depths_u8.numel(),
                                                                  table, n, h, w, channels, depth_bits, image0.data_ptr(), image1.data_ptr(),
                                                                  image2.data_ptr(), depth.data_ptr(), _stream()),
                      nbytes=float(n * h * w) * (3 * channels + depth_bits // 8 + 40)), "kbn_unpack_train_frames_forward")
    return image0, image1, image2, depth


def unpack_packed_frames(images_u8, depths_u8, frames, shape, channels: int = 3, depth_bits: int = 16, middle_only: bool = False):
    """unpack_train_frames from PACKED files (kb.loader.encode_frame): the same four tensors, bit for bit, decoded on the
    device from the files' bytes (kbn_unpack_packed_frames_forward, csrc/unpack_packed.hip: one launch per
    _lib.KBN_UNPACK_TRAIN_MAX_FRAMES frames).

    images_u8 / depths_u8: 1-d uint8 device buffers, 16-byte aligned, that hold the files as they are on disk.  frames: one
    (image_offset, image_bytes, depth_offset, depth_bytes, H, W, y_start, x_start) a frame -- where its packed H x 3 W x channels
    triplet and its packed H x W depth map lie (offsets multiples of 16) and where its crop starts inside each third.  Every file
    must have passed kbn_frame_check (kb.loader.check_frame) on the host before its bytes were copied: that check is what keeps the
    kernel inside the files.  middle_only: returns (image0, sparse_depth0) and decodes only the middle third.  A raw width 3 W
    above _lib.KBN_UNPACK_PACKED_MAX_RAW_WIDTH raises KbnError (the kernel's LDS budget).  No CPU fallback."""
    fn = "unpack_packed_frames"
    channels, depth_bits = int(channels), int(depth_bits)

    def place(i, f):
        io, ib, do, db = f[:4]
        for what, at, size, buf in (("triplet", io, ib, images_u8), ("depth map", do, db, depths_u8)):
            if at < 0 or at % 16 or size < 1 or size > 0xffffffff or at + size > buf.numel():
                raise KbnError(f"{fn}: frame {i}: its packed {what} of {size} bytes at byte {at} is misaligned or leaves its buffer of {buf.numel()} bytes")
        return io, do, ib, db

    h, w, frames, n, records = _unpack_records(fn, images_u8, depths_u8, frames, shape, channels, depth_bits, _PACKED_FRAME_RECORD,
                                               "image_offset, image_bytes, depth_offset, depth_bytes, H, W, y_start, x_start", place,
                                               max_raw_width=_lib.KBN_UNPACK_PACKED_MAX_RAW_WIDTH, align=16)
    device = images_u8.device
    image0 = torch.empty((n, 3, h, w), device=device, dtype=torch.float32)
    image1, image2 = (None, None) if middle_only else (torch.empty((n, 3, h, w), device=device, dtype=torch.float32) for _ in range(2))
    depth = torch.empty((n, 1, h, w), device=device, dtype=torch.float32)
    lib = _lib.load()
    table = (_lib.PackedFrame * n).from_buffer(records)
    packed_bytes = float(sum(f[1] + f[3] for f in frames))
    with torch.cuda.device(device):
        check(_launch("unpack_packed_frames", 0.0,
                      lambda: lib.kbn_unpack_packed_frames_forward(images_u8.data_ptr(), images_u8.numel(), depths_u8.data_ptr(), depths_u8.numel(),
                                                                   table, n, h, w, channels, depth_bits, image0.data_ptr(),
                                                                   None if middle_only else image1.data_ptr(),
                                                                   None if middle_only else image2.data_ptr(), depth.data_ptr(), _stream()),
                      nbytes=packed_bytes + float(n * h * w) * (16 if middle_only else 40)), "kbn_unpack_packed_frames_forward")
    return (image0, depth) if middle_only else (image0, image1, image2, depth)


def unpack_sequence_frames(images_u8, depths_u8, frames, shape, channels: int = 3, depth_bits: int = 16):
    """unpack_train_frames for samples whose three frames lie at three places of their own (kb.loader.split_sample): the
    same four tensors, bit for bit what the triplet np.concatenate([previous, current, next], axis=1) gives there, and no triplet is
    assembled (kbn_unpack_sequence_frames_forward, csrc/unpack_sequence.hip: one launch per _lib.KBN_UNPACK_SEQUENCE_MAX_FRAMES samples).

    images_u8 / depths_u8: packed 1-d uint8 device buffers.  frames: one (previous_offset, current_offset, next_offset, depth_offset,
    H, W, y_start, x_start) a sample -- the byte offsets of its three H x W x channels frames (they may coincide, and samples may
    share frames) and of its H x W depth samples, and where its crop starts in every frame.  W is a frame's width.  Everything else
    as unpack_train_frames: image0 is `current`, image1 `previous`, image2 `next`.  No CPU fallback."""
    fn = "unpack_sequence_frames"
    channels, depth_bits = int(channels), int(depth_bits)

    def place(i, f):
        offsets, do, H, W = f[:3], f[3], f[4], f[5]
        for what, io in zip(("previous", "current", "next"), offsets):
            if io < 0 or io + H * W * channels > images_u8.numel():
                raise KbnError(f"{fn}: frame {i}: its {what} frame of {H} x {W} x {channels} at byte {io} leaves the image buffer of {images_u8.numel()} bytes")
        if do < 0 or do % (depth_bits // 8) or do + H * W * (depth_bits // 8) > depths_u8.numel():
            raise KbnError(f"{fn}: frame {i}: its {H} x {W} depth map of {depth_bits}-bit samples at byte {do} is misaligned or leaves "
                           f"the depth buffer of {depths_u8.numel()} bytes")
        return tuple(offsets) + (do,)

    h, w, frames, n, records = _unpack_records(fn, images_u8, depths_u8, frames, shape, channels, depth_bits, _SEQUENCE_FRAME_RECORD,
                                               "previous_offset, current_offset, next_offset, depth_offset, H, W, y_start, x_start", place,
                                               thirds=1)
    device = images_u8.device
    image0, image1, image2 = (torch.empty((n, 3, h, w), device=device, dtype=torch.float32) for _ in range(3))
    depth = torch.empty((n, 1, h, w), device=device, dtype=torch.float32)
    lib = _lib.load()
    table = (_lib.SequenceFrame * n).from_buffer(records)
    with torch.cuda.device(device):
        check(_launch("unpack_sequence_frames", 0.0,
                      lambda: lib.kbn_unpack_sequence_frames_forward(images_u8.data_ptr(), images_u8.numel(), depths_u8.data_ptr(), depths_u8.numel(),
                                                                     table, n, h, w, channels, depth_bits, image0.data_ptr(), image1.data_ptr(),
                                                                     image2.data_ptr(), depth.data_ptr(), _stream()),
                      nbytes=float(n * h * w) * (3 * channels + depth_bits // 8 + 40)), "kbn_unpack_sequence_frames_forward")
    return image0, image1, image2, depth


def unpack_packed_sequence_frames(images_u8, depths_u8, frames, shape, channels: int = 3, depth_bits: int = 16, middle_only: bool = False):
    """unpack_sequence_frames from PACKED files, one per frame (kbn_unpack_packed_sequence_frames_forward, csrc/unpack_sequence.hip:
    one launch per _lib.KBN_UNPACK_SEQUENCE_MAX_FRAMES samples): what unpack_packed_frames gives for the packed triplet, bit for bit.

    images_u8 / depths_u8: 1-d uint8 device buffers, 16-byte aligned, that hold the files as they are on disk.  frames: one
    (previous_offset, previous_bytes, current_offset, current_bytes, next_offset, next_bytes, depth_offset, depth_bytes, H, W,
    y_start, x_start) a sample -- where its three packed H x W x channels frames and its packed H x W depth map lie (offsets
    multiples of 16; they may coincide and be shared) and where its crop starts in every frame.  Every file must have passed
    kbn_frame_check (kb.loader.check_frame) on the host.  middle_only: returns (image0, sparse_depth0) and decodes only `current`
    (all three places are still checked).  A width above _lib.KBN_UNPACK_PACKED_MAX_RAW_WIDTH raises KbnError.  No CPU fallback."""
    fn = "unpack_packed_sequence_frames"
    channels, depth_bits = int(channels), int(depth_bits)

    def place(i, f):
        files = (("previous frame", f[0], f[1], images_u8), ("current frame", f[2], f[3], images_u8), ("next frame", f[4], f[5], images_u8),
                 ("depth map", f[6], f[7], depths_u8))
        for what, at, size, buf in files:
            if at < 0 or at % 16 or size < 1 or size > 0xffffffff or at + size > buf.numel():
                raise KbnError(f"{fn}: frame {i}: its packed {what} of {size} bytes at byte {at} is misaligned or leaves its buffer of {buf.numel()} bytes")
        return f[0], f[2], f[4], f[6], f[1], f[3], f[5], f[7]

    h, w, frames, n, records = _unpack_records(fn, images_u8, depths_u8, frames, shape, channels, depth_bits, _PACKED_SEQUENCE_FRAME_RECORD,
                                               "previous_offset, previous_bytes, current_offset, current_bytes, next_offset, next_bytes, "
                                               "depth_offset, depth_bytes, H, W, y_start, x_start", place,
                                               max_raw_width=_lib.KBN_UNPACK_PACKED_MAX_RAW_WIDTH, align=16, thirds=1)
    device = images_u8.device
    image0 = torch.empty((n, 3, h, w), device=device, dtype=torch.float32)
    image1, image2 = (None, None) if middle_only else (torch.empty((n, 3, h, w), device=device, dtype=torch.float32) for _ in range(2))
    depth = torch.empty((n, 1, h, w), device=device, dtype=torch.float32)
    lib = _lib.load()
    table = (_lib.PackedSequenceFrame * n).from_buffer(records)
    packed_bytes = float(sum(f[3] + f[7] if middle_only else f[1] + f[3] + f[5] + f[7] for f in frames))
    with torch.cuda.device(device):
        check(_launch("unpack_packed_sequence_frames", 0.0,
                      lambda: lib.kbn_unpack_packed_sequence_frames_forward(images_u8.data_ptr(), images_u8.numel(), depths_u8.data_ptr(),
                                                                            depths_u8.numel(), table, n, h, w, channels, depth_bits,
                                                                            image0.data_ptr(), None if middle_only else image1.data_ptr(),
                                                                            None if middle_only else image2.data_ptr(), depth.data_ptr(), _stream()),
                      nbytes=packed_bytes + float(n * h * w) * (16 if middle_only else 40)), "kbn_unpack_packed_sequence_frames_forward")
    return (image0, depth) if middle_only else (image0, image1, image2, depth)


@_on_tensor_device
def eval_metrics(output_depth, ground_truth, ground_truth_validity, min_evaluate_depth: float,
                 max_evaluate_depth: float):
    """Per-frame (MAE [mm], RMSE [mm], iMAE [1/km], iRMSE [1/km]) as an N x 4 fp64 tensor, computed on
    the device (reference src/kbnet.py:932-950 does this on the host after a D2H copy).  A frame in which no pixel passes the mask
    (validity > 0, min < ground truth < max) gives four NaNs, as the reference's np.mean over an empty selection does; a mean over
    the rows (inference.run, validation.validate) is then NaN exactly where the reference's is."""
    lib = _lib.load()
    o = output_depth.contiguous()
    _require(o, "output_depth")
    g = ground_truth.contiguous()
    v = ground_truth_validity.contiguous()
    _require(g, "ground_truth")
    _require(v, "ground_truth_validity")
    n, h, w = o.shape[0], o.shape[-2], o.shape[-1]
    if g.numel() != o.numel() or v.numel() != o.numel():
        raise KbnError("ground truth must have one value per output pixel")
    sums = torch.zeros((n, 5), device=o.device, dtype=torch.float64)
    check(lib.kbn_eval_accumulate(o.data_ptr(), g.data_ptr(), v.data_ptr(), sums.data_ptr(), n, h, w,
                                  float(min_evaluate_depth), float(max_evaluate_depth), _stream()),
          "kbn_eval_accumulate")
    mean = sums[:, :4] / sums[:, 4:5]      # 0 / 0: a frame without an evaluated pixel is NaN, as np.mean of nothing is
    return torch.stack([mean[:, 0], mean[:, 1].sqrt(), mean[:, 2], mean[:, 3].sqrt()], dim=1)


# ------------------------------------------------------------------ the objective: its sums and their gradient
_LOSS_ARGS = ("image0", "image1", "image2", "output_depth", "sparse_depth", "validity_map", "intrinsics", "pose01", "pose02")
_LOSS_TRAINED = ("output_depth", "pose01", "pose02")   # what the reference trains through; everything else is data


def _loss_inputs(fn: str, tensors):
    """The argument checks `photometric_loss` and `photometric_loss_backward` share -> (n, h, w, the nine dense tensors)."""
    for t, name in zip(tensors, _LOSS_ARGS):
        if not isinstance(t, torch.Tensor):
            raise KbnError(f"{fn}: {name} must be a tensor, got {type(t).__name__}")
    image0 = tensors[0]
    if image0.dim() != 4 or image0.shape[1] != 3:
        raise KbnError(f"{fn}: image0 must be N x 3 x H x W, got {tuple(image0.shape)}")
    n, _, h, w = image0.shape
    if n < 1 or h < 3 or w < 3:
        raise KbnError(f"{fn}: needs at least one frame of at least 3 x 3 pixels (SSIM pools 3 x 3 windows), got {tuple(image0.shape)}")
    want = {"image1": (n, 3, h, w), "image2": (n, 3, h, w), "output_depth": (n, 1, h, w), "sparse_depth": (n, 1, h, w),
            "validity_map": (n, 1, h, w), "intrinsics": (n, 3, 3), "pose01": (n, 4, 4), "pose02": (n, 4, 4)}
    for t, name in zip(tensors, _LOSS_ARGS):
        if name in want and tuple(t.shape) != want[name]:
            raise KbnError(f"{fn}: {name} must be {want[name]} beside image0 {tuple(image0.shape)}, got {tuple(t.shape)}")
    if torch.is_grad_enabled():
        for t, name in zip(tensors, _LOSS_ARGS):
            if name not in _LOSS_TRAINED and t.requires_grad:
                raise KbnError(f"{fn}: {name} requires grad, but it is data and gets no gradient (gradients exist for "
                               + ", ".join(_LOSS_TRAINED) + "); detach it")
    for t, name in zip(tensors, _LOSS_ARGS):
        _require(t, name)
    return n, h, w, tuple(t.detach().contiguous() for t in tensors)


def _photometric_loss_launch(n, h, w, dense, return_images):
    lib = _lib.load()
    i0, i1, i2, d, s, v, k, p1, p2 = dense
    sums = torch.empty((n, 8), device=i0.device, dtype=torch.float64)   # the entry zeroes it on the stream
    w1 = torch.empty_like(i0) if return_images else None
    w2 = torch.empty_like(i0) if return_images else None
    check(lib.kbn_photometric_loss_forward(i0.data_ptr(), i1.data_ptr(), i2.data_ptr(), d.data_ptr(), s.data_ptr(), v.data_ptr(),
                                           k.data_ptr(), p1.data_ptr(), p2.data_ptr(), sums.data_ptr(),
                                           w1.data_ptr() if return_images else None, w2.data_ptr() if return_images else None,
                                           n, h, w, _stream()), "kbn_photometric_loss_forward")
    return (sums, w1, w2) if return_images else sums


class _PhotometricLoss(torch.autograd.Function):
    """The N x 8 sums as a differentiable node: forward is the forward launch, backward one launch of
    kbn_photometric_loss_backward.  Saved for backward: the nine inputs, nothing the forward computed."""

    @staticmethod
    def forward(ctx, shape, return_images, *tensors):
        ctx.save_for_backward(*tensors)
        out = _photometric_loss_launch(*shape, tuple(t.detach().contiguous() for t in tensors), return_images)
        if return_images:
            ctx.mark_non_differentiable(out[1], out[2])   # logging outputs: nothing trains through the warped images
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_sums, *_):
        grads = photometric_loss_backward(*ctx.saved_tensors, grad_sums)
        need = ctx.needs_input_grad[2:]
        by_name = dict(zip(_LOSS_TRAINED, grads))
        return (None, None) + tuple(by_name[name] if name in by_name and need[i] else None for i, name in enumerate(_LOSS_ARGS))


@_on_tensor_device
def photometric_loss(image0, image1, image2, output_depth, sparse_depth, validity_map, intrinsics, pose01, pose02,
                     return_images: bool = False):
    """The sums behind KBNetModel.compute_loss (reference src/kbnet_model.py:188-304) in one kernel: an N x 8 fp64 tensor
    {sum |image01 - image0|, sum |image02 - image0|, sum ssim01, sum ssim02, sum v |sparse - depth|, sum v, sum wx |dx depth|,
    sum wy |dy depth|} per frame (kbn_photometric_loss_forward), where image01 / image02 are image1 / image2 sampled where the
    depth and the relative poses put each pixel of image0.  `return_images`: also the two warped images (N x 3 x H x W), which the
    reference hands back for logging; without it nothing image-sized is written.

    Differentiable with respect to output_depth, pose01 and pose02 (what the reference trains through): when grad mode is on and
    one of them requires grad, the sums come from an autograd node whose backward is one launch (`photometric_loss_backward`) and
    which saves its inputs only.  The warped images are outputs for logging and carry no gradient.  Any other argument that
    requires grad is an error, not a silent None."""
    tensors = (image0, image1, image2, output_depth, sparse_depth, validity_map, intrinsics, pose01, pose02)
    n, h, w, dense = _loss_inputs("photometric_loss", tensors)
    if torch.is_grad_enabled() and any(t.requires_grad for t in (output_depth, pose01, pose02)):
        return _PhotometricLoss.apply((n, h, w), bool(return_images), *tensors)
    return _photometric_loss_launch(n, h, w, dense, return_images)


@_on_tensor_device
def photometric_loss_backward(image0, image1, image2, output_depth, sparse_depth, validity_map, intrinsics, pose01, pose02, grad_sums,
                              out=None):
    """The gradient of `photometric_loss`'s sums, in one kernel (kbn_photometric_loss_backward): `grad_sums` (N x 8, the gradient
    of the sums) -> (grad_depth N x 1 x H x W, grad_pose01, grad_pose02 N x 4 x 4), fp32.  The kernel reduces the gradient with
    respect to T = rows 0-2 of (K | 0) pose in fp64 (N x 2 x 12); grad_pose[:3] = K^T grad_T is formed here in fp64 torch on those
    24 numbers per frame and rounded once; row 3 of a pose gradient is zero.  `out`: (grad_depth, grad_T) buffers to write
    into, an fp32 N x 1 x H x W and an fp64 N x 2 x 12 device tensor, both contiguous."""
    lib = _lib.load()
    tensors = (image0, image1, image2, output_depth, sparse_depth, validity_map, intrinsics, pose01, pose02)
    n, h, w, dense = _loss_inputs("photometric_loss_backward", tensors)
    if not isinstance(grad_sums, torch.Tensor) or not grad_sums.is_cuda or not grad_sums.is_floating_point() or tuple(grad_sums.shape) != (n, 8):
        raise KbnError(f"photometric_loss_backward: grad_sums must be a floating-point CUDA/HIP tensor of shape {(n, 8)}, got "
                       + (f"{tuple(grad_sums.shape)} {grad_sums.dtype} on {grad_sums.device}" if isinstance(grad_sums, torch.Tensor)
                          else type(grad_sums).__name__))
    i0, i1, i2, d, s, v, k, p1, p2 = dense
    gs = grad_sums.detach().to(torch.float64).contiguous()
    if out is None:
        grad_depth = torch.empty_like(d)                                          # every element is written by the kernel
        grad_t = torch.empty((n, 2, 12), device=d.device, dtype=torch.float64)    # the entry zeroes it on the stream
    else:
        grad_depth, grad_t = out
        _require(grad_depth, "out[0]", 4)
        if tuple(grad_depth.shape) != (n, 1, h, w) or not grad_depth.is_contiguous():
            raise KbnError(f"photometric_loss_backward: out[0] must be a contiguous {(n, 1, h, w)} tensor, got {tuple(grad_depth.shape)}")
        if not isinstance(grad_t, torch.Tensor) or not grad_t.is_cuda or grad_t.dtype != torch.float64 or tuple(grad_t.shape) != (n, 2, 12) \
                or not grad_t.is_contiguous():
            raise KbnError(f"photometric_loss_backward: out[1] must be a contiguous float64 CUDA/HIP tensor of shape {(n, 2, 12)}")
    check(lib.kbn_photometric_loss_backward(i0.data_ptr(), i1.data_ptr(), i2.data_ptr(), d.data_ptr(), s.data_ptr(), v.data_ptr(),
                                            k.data_ptr(), p1.data_ptr(), p2.data_ptr(), gs.data_ptr(), grad_depth.data_ptr(),
                                            grad_t.data_ptr(), n, h, w, _stream()), "kbn_photometric_loss_backward")
    grad_pose = torch.zeros((2, n, 4, 4), device=d.device, dtype=torch.float64)
    grad_pose[:, :, :3] = torch.matmul(k.double().transpose(1, 2)[None], grad_t.reshape(n, 2, 3, 4).transpose(0, 1))
    grad_pose = grad_pose.float()
    return grad_depth, grad_pose[0], grad_pose[1]


def loss_terms(sums: torch.Tensor, height: int, width: int) -> torch.Tensor:
    """N x 8 sums of `photometric_loss` -> N x 4 fp64 (colour, structure, sparse depth, smoothness) of each frame, normalised as the
    reference normalises the batch (src/losses.py): colour and structure sum the 3 channels and divide by H W (three times a
    per-channel mean); sparse depth divides by the frame's number of valid points (NaN for a frame without one, as in the
    reference); smoothness is mean over H (W-1) plus mean over (H-1) W.  The batch's terms are the means of the columns."""
    hw = float(height * width)
    return torch.stack([(sums[:, 0] + sums[:, 1]) / hw, (sums[:, 2] + sums[:, 3]) / hw, sums[:, 4] / sums[:, 5],
                        sums[:, 6] / float(height * (width - 1)) + sums[:, 7] / float((height - 1) * width)], dim=1)


def pose_matrix(v: torch.Tensor) -> torch.Tensor:
    """N x 6 -> N x 4 x 4 as the reference's net_utils.pose_matrix (src/net_utils.py:1493-1595): the FIRST three entries are the
    axis-angle rotation and the LAST three the translation (its docstring says the opposite; the code decides), axis = r / (|r| + 1e-7),
    M = T(t) R.  Plain torch on the tensor's device and in its dtype: 16 numbers per frame.  |r| is written out (see below): at most 1 ulp
    of the angle from the reference's torch.norm, whose rounding is torch's and the device's own."""
    if not isinstance(v, torch.Tensor) or v.dim() != 2 or v.shape[1] != 6:
        raise KbnError(f"pose_matrix: expected an N x 6 tensor, got {tuple(v.shape) if isinstance(v, torch.Tensor) else type(v).__name__}")
    r, t = v[:, :3], v[:, 3:]
    # sqrt((r0 r0 + r1 r1) + r2 r2), every product and sum an operation of its own -- what pose_from_dof (csrc/posenet.hip) evaluates.
    # torch.norm / linalg.vector_norm round their sum another way, and not the same way on the CPU and on the device (1 ulp of the
    # angle for about one vector in nine): with them this function had no fixed bits for the head kernel to reproduce.
    angle = torch.sqrt((r[:, 0:1] * r[:, 0:1] + r[:, 1:2] * r[:, 1:2]) + r[:, 2:3] * r[:, 2:3])
    axis = r / (angle + 1e-7)
    ca, sa = torch.cos(angle[:, 0]), torch.sin(angle[:, 0])
    c = 1 - ca
    x, y, z = axis[:, 0], axis[:, 1], axis[:, 2]
    xs, ys, zs = x * sa, y * sa, z * sa
    xc, yc, zc = x * c, y * c, z * c
    xyc, yzc, zxc = x * yc, y * zc, z * xc
    zero, one = torch.zeros_like(ca), torch.ones_like(ca)
    rows = [x * xc + ca, xyc - zs, zxc + ys, t[:, 0],
            xyc + zs, y * yc + ca, yzc - xs, t[:, 1],
            zxc - ys, yzc + xs, z * zc + ca, t[:, 2],
            zero, zero, zero, one]
    return torch.stack(rows, dim=1).reshape(-1, 4, 4)


# ------------------------------------------------------------------ pose network (eval mode)
def _pack_pose_weight(fn: str, family: str, sizes_text: str, weight: torch.Tensor, out: Optional[torch.Tensor]) -> torch.Tensor:
    """The three pose-network pack wrappers: OIHW -> the blob of kbn_<family>_pack_weight, sized by kbn_<family>_packed_weight_bytes."""
    lib = _lib.load()
    w = _weight(weight)
    oc, cin, kh, kw = w.shape
    if kh != kw:
        raise KbnError("square kernels only")
    nbytes = getattr(lib, f"kbn_{family}_packed_weight_bytes")(oc, cin, kh)
    if nbytes == 0:
        raise KbnError(f"{fn}: unsupported weight shape {tuple(w.shape)} (kernel size {sizes_text})")
    pack = getattr(lib, f"kbn_{family}_pack_weight")
    return _pack_into(out, nbytes, w, lambda p: pack(w.data_ptr(), p, oc, cin, kh, _stream()), f"kbn_{family}_pack_weight")


def _conv_inputs(fn: str, inputs):
    """The one or two N x C_i x H x W tensors a pose conv reads in place -> (inputs, sources, n, h, w, total channels)."""
    inputs = list(inputs)
    if not 1 <= len(inputs) <= 2:
        raise KbnError(f"{fn}: one or two inputs, got {len(inputs)}")
    srcs = [tensor_src(t.detach() if isinstance(t, torch.Tensor) else t, f"inputs[{i}]") for i, t in enumerate(inputs)]
    n, _, h, w = inputs[0].shape
    for i, t in enumerate(inputs[1:], 1):
        if t.shape[0] != n or tuple(t.shape[2:]) != (h, w):
            raise KbnError(f"{fn}: inputs[{i}] is {tuple(t.shape)} beside inputs[0] {tuple(inputs[0].shape)}")
    if n < 1 or h < 1 or w < 1 or any(s.channels < 1 for s in srcs):
        raise KbnError(f"{fn}: empty input {tuple(inputs[0].shape)}")
    return inputs, srcs, n, h, w, sum(s.channels for s in srcs)


def _affine_conv_args(fn: str, bytes_fn, inputs, packed_weight, scale, shift, out_channels: int, kernel_size: int):
    """What conv2d_s2_affine and conv2d_affine check alike: the inputs (_conv_inputs), the blob's size (`bytes_fn`: the family's
    kbn_*_packed_weight_bytes) and scale / shift -> (inputs, sources, n, h, w, total channels, floats in the blob)."""
    inputs, srcs, n, h, w, cin = _conv_inputs(fn, inputs)
    _require(packed_weight, "packed_weight", 1)
    want = bytes_fn(out_channels, cin, kernel_size) // 4
    if want == 0 or packed_weight.numel() != want or not packed_weight.is_contiguous():
        raise KbnError(f"{fn}: packed_weight holds {packed_weight.numel()} floats, a {out_channels} x {cin} x "
                       f"{kernel_size} x {kernel_size} weight packs into {want}")
    for t, name in ((scale, "scale"), (shift, "shift")):
        _require(t, name, 1)
        if t.numel() != out_channels or not t.is_contiguous():
            raise KbnError(f"{fn}: {name} must be {out_channels} contiguous floats, got {tuple(t.shape)}")
    return inputs, srcs, n, h, w, cin, want


@_on_tensor_device
def pack_conv2d_s2_affine_weight(weight: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """OIHW (k in {3, 5, 7}, any channel counts) -> the [filter tile][K chunk][16][filters] order conv2d_s2_affine reads
    (kbn_conv2d_s2_affine_pack_weight); `out`: an existing blob of the right size to re-pack into."""
    return _pack_pose_weight("conv2d_s2_affine", "conv2d_s2_affine", "3, 5 or 7", weight, out)


@_on_tensor_device
def conv2d_s2_affine(inputs: Sequence[torch.Tensor], packed_weight: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor,
                     out_channels: int, kernel_size: int, negative_slope: Optional[float] = 0.2,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act(conv_{k x k, stride 2, padding k // 2}(cat(inputs, 1)) * scale + shift) (kbn_conv2d_s2_affine_forward): the conv +
    eval-mode BatchNorm2d + activation of a PoseEncoder layer (reference src/net_utils.py:120-141) in one launch.  `inputs`: one
    or two N x C_i x H x W tensors read in place (no concat); `scale` / `shift`: out_channels floats; `negative_slope` None: no
    activation; `out`: an N x out_channels x ceil(H / 2) x ceil(W / 2) tensor or channel slice to write into."""
    lib = _lib.load()
    if kernel_size not in (3, 5, 7):
        raise KbnError(f"conv2d_s2_affine: kernel size 3, 5 or 7, got {kernel_size}")
    inputs, srcs, n, h, w, cin, _ = _affine_conv_args("conv2d_s2_affine", lib.kbn_conv2d_s2_affine_packed_weight_bytes, inputs,
                                                      packed_weight, scale, shift, out_channels, kernel_size)
    oh, ow = (h + 1) // 2, (w + 1) // 2
    out = _out_tensor(out, (n, out_channels, oh, ow), inputs[0].device, planes=True)
    optr, obs = _planes(out, "out")
    arr = (ConvSrc * len(srcs))(*srcs)
    k2 = kernel_size * kernel_size
    kpad = -(-cin * k2 // 16) * 16
    nt = 16 if out_channels <= 16 else (32 if out_channels <= 32 else 64)
    check(_launch(f"conv_s2_affine<{kernel_size},{nt // 16}>", 2.0 * n * oh * ow * cin * k2 * out_channels,
                  lambda: lib.kbn_conv2d_s2_affine_forward(arr, len(srcs), packed_weight.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                                                           optr, obs, n, out_channels, kernel_size, h, w,
                                                           *_act_args(negative_slope), _stream()),
                  executed=2.0 * (-(-n * oh * ow // 128) * 128) * kpad * (-(-out_channels // nt) * nt), pipe="fp32",
                  nbytes=_src_bytes(srcs, n) + 4.0 * n * oh * ow * out_channels), "kbn_conv2d_s2_affine_forward")
    return out


@_on_tensor_device
def pose_head(latent: torch.Tensor, weight: torch.Tensor, return_dof: bool = False, out: Optional[torch.Tensor] = None,
              dof_out: Optional[torch.Tensor] = None):
    """PoseDecoder.forward without hidden layers (reference src/networks.py:2067-2075) in one launch (kbn_pose_head_forward):
    latent N x C x h x w, weight 6 x C (x 1 x 1) -> N x 4 x 4 = pose_matrix(0.01 * mean_hw(conv1x1(latent))).  `return_dof`: also
    the N x 6 vector.  `out` / `dof_out`: contiguous N x 4 x 4 / N x 6 tensors to write into."""
    lib = _lib.load()
    ptr, bs = _planes(latent, "latent")
    n, c, h, w = latent.shape
    _require(weight, "weight")
    if weight.numel() != 6 * c or weight.shape[0] != 6 or not weight.is_contiguous():
        raise KbnError(f"pose_head: weight must be a contiguous 6 x {c} (x 1 x 1) tensor, got {tuple(weight.shape)}")
    if n < 1 or c < 1 or h < 1 or w < 1:
        raise KbnError(f"pose_head: empty latent {tuple(latent.shape)}")
    out = _out_tensor(out, (n, 4, 4), latent.device, "pose_head: out")
    if return_dof or dof_out is not None:
        dof_out = _out_tensor(dof_out, (n, 6), latent.device, "pose_head: dof_out")
    check(_launch("pose_head", 2.0 * n * h * w * c * 6,
                  lambda: lib.kbn_pose_head_forward(ptr, bs, weight.data_ptr(), out.data_ptr(),
                                                    dof_out.data_ptr() if dof_out is not None else None, n, c, h, w, _stream()),
                  nbytes=4.0 * n * c * h * w), "kbn_pose_head_forward")
    return (out, dof_out) if return_dof else out


# ------------------------------------------------------------------ conv gradients: the family that serves a (kernel size, stride)
# True: conv2d_s2_backward_data / conv2d_s2_backward_weight (csrc/posenet_backward.hip); False: conv2d_backward_data /
# conv2d_backward_weight (csrc/conv_affine_backward.hip).  Both weight gradients are the one kernel of csrc/conv_bwd_weight.hip.
# Every case list below and every choice between the two families reads this table.
_S2_FAMILY = {(3, 2): True, (5, 2): True, (7, 2): True, (3, 1): False, (1, 1): False, (1, 2): False}
_BACKWARD_CASES = tuple(ks for ks, s2 in _S2_FAMILY.items() if not s2)   # (3, 1), (1, 1), (1, 2): the error texts print them in this order
_KBNET_CASES = ((3, 1), (3, 2), (1, 1), (1, 2))                          # the depth network's convs, in the order its error text prints
assert set(_KBNET_CASES) <= set(_S2_FAMILY)


def _conv_backward_weight(fn: str, check_case, record: str, ks, inputs, grad_out, splits, out):
    """The one body of conv2d_s2_backward_weight and conv2d_backward_weight.  `ks`: (kernel size,) or (kernel size, stride) -- the
    arguments of `check_case(fn, *ks)`, of the C pair kbn_<fn> / kbn_<fn>_scratch_bytes in that place, and of the launch record
    `record`<ks, filter blocks>."""
    lib = _lib.load()
    check_case(fn, *ks)
    kernel_size, stride = ks[0], (ks[1] if len(ks) == 2 else 2)
    inputs, srcs, n, h, w, cin = _conv_inputs(fn, inputs)
    gptr, gbs = _planes(grad_out, "grad_out")
    oc, oh, ow = grad_out.shape[1], -(-h // stride), -(-w // stride)
    if oc < 1 or tuple(grad_out.shape) != (n, oc, oh, ow):
        raise KbnError(f"{fn}: grad_out is {tuple(grad_out.shape)}, the conv of inputs {tuple(inputs[0].shape)} "
                       f"has {n} frames of {oh} x {ow} maps")
    if splits is not None and (not isinstance(splits, int) or splits < 1):
        raise KbnError(f"{fn}: splits must be a positive integer or None, got {splits!r}")
    splits = 0 if splits is None else splits
    out = _out_tensor(out, (oc, cin, kernel_size, kernel_size), grad_out.device, f"{fn}: out")
    nbytes = getattr(lib, f"kbn_{fn}_scratch_bytes")(n, oc, cin, *ks, h, w, splits)
    scratch = torch.empty(nbytes // 4, device=grad_out.device, dtype=torch.float32) if nbytes else None
    arr = (ConvSrc * len(srcs))(*srcs)
    k2 = kernel_size * kernel_size
    mt = 16 if oc <= 16 else (32 if oc <= 32 else 64)
    check(_launch(f"{record}<{','.join(map(str, ks))},{mt // 16}>", 2.0 * n * oh * ow * cin * k2 * oc,
                  lambda: getattr(lib, f"kbn_{fn}")(arr, len(srcs), gptr, gbs, out.data_ptr(), n, oc, *ks, h, w, splits,
                                                    scratch.data_ptr() if scratch is not None else None, nbytes, _stream()),
                  executed=2.0 * (-(-n * oh * ow // 32) * 32) * (-(-cin * k2 // 64) * 64) * (-(-oc // mt) * mt), pipe="fp32",
                  nbytes=_src_bytes(srcs, n) + 4.0 * (n * oc * oh * ow + oc * cin * k2)), f"kbn_{fn}")
    return out


# ------------------------------------------------------------------ pose network (training: csrc/posenet_backward.hip)
def _s2_kernel_size(fn: str, kernel_size):
    if not _S2_FAMILY.get((kernel_size, 2)):
        raise KbnError(f"{fn}: kernel size 3, 5 or 7, got {kernel_size}")


@_on_tensor_device
def pack_conv2d_s2_backward_data_weight(weight: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """OIHW (k in {3, 5, 7}) -> the transposed order conv2d_s2_backward_data reads: [input-channel tile][(filter, tap) chunk][16]
    [input channels] (kbn_conv2d_s2_backward_data_pack_weight; not the forward's blob).  `out`: a blob to re-pack into."""
    return _pack_pose_weight("conv2d_s2_backward_data", "conv2d_s2_backward_data", "3, 5 or 7", weight, out)


@_on_tensor_device
def conv2d_s2_backward_data(grad_out: torch.Tensor, packed_weight: torch.Tensor, in_channels: Sequence[int], kernel_size: int,
                            in_height: int, in_width: int, out: Optional[Sequence[torch.Tensor]] = None) -> List[torch.Tensor]:
    """The gradient of conv_{k x k, stride 2, padding k // 2}(cat(inputs, 1)) with respect to its one or two inputs
    (kbn_conv2d_s2_backward_data): grad_out N x F x ceil(H / 2) x ceil(W / 2) -> [N x C_i x H x W for C_i in in_channels], the
    matching channel ranges of the concat's gradient.  `packed_weight`: pack_conv2d_s2_backward_data_weight of the F x sum(C_i) x k
    x k weight.  `out`: tensors or channel slices to write into.  One launch, all k x k taps with three quarters of them
    predicated to zero (an input pixel meets only the taps of its parity): `executed` in the launch record says so."""
    lib = _lib.load()
    _s2_kernel_size("conv2d_s2_backward_data", kernel_size)
    in_channels = [int(c) for c in in_channels]
    if not 1 <= len(in_channels) <= 2 or any(c < 1 for c in in_channels):
        raise KbnError(f"conv2d_s2_backward_data: one or two positive channel counts, got {in_channels}")
    if in_height < 1 or in_width < 1:
        raise KbnError(f"conv2d_s2_backward_data: empty input {in_height} x {in_width}")
    gptr, gbs = _planes(grad_out, "grad_out")
    n, oc, oh, ow = grad_out.shape
    if n < 1 or oc < 1 or (oh, ow) != ((in_height + 1) // 2, (in_width + 1) // 2):
        raise KbnError(f"conv2d_s2_backward_data: grad_out is {tuple(grad_out.shape)}, the conv of a {in_height} x {in_width} input "
                       f"has {(in_height + 1) // 2} x {(in_width + 1) // 2} maps")
    cin = sum(in_channels)
    _require(packed_weight, "packed_weight", 1)
    want = lib.kbn_conv2d_s2_backward_data_packed_weight_bytes(oc, cin, kernel_size) // 4
    if want == 0 or packed_weight.numel() != want or not packed_weight.is_contiguous():
        raise KbnError(f"conv2d_s2_backward_data: packed_weight holds {packed_weight.numel()} floats, a {oc} x {cin} x "
                       f"{kernel_size} x {kernel_size} weight packs into {want}")
    if out is not None and len(out) != len(in_channels):
        raise KbnError(f"conv2d_s2_backward_data: {len(out)} output tensors for {len(in_channels)} inputs")
    grads = [_out_tensor(None if out is None else out[i], (n, c, in_height, in_width), grad_out.device, f"out[{i}]", planes=True)
             for i, c in enumerate(in_channels)]
    ptrs = [_planes(g, f"out[{i}]") for i, g in enumerate(grads)]
    p1, bs1, c1 = (ptrs[1][0], ptrs[1][1], in_channels[1]) if len(grads) == 2 else (None, 0, 0)
    k2 = kernel_size * kernel_size
    nt = 16 if cin <= 16 else (32 if cin <= 32 else 64)
    check(_launch(f"conv_s2_bwd_data<{kernel_size},{nt // 16}>", 2.0 * n * oh * ow * cin * k2 * oc,
                  lambda: lib.kbn_conv2d_s2_backward_data(gptr, gbs, packed_weight.data_ptr(), ptrs[0][0], ptrs[0][1], in_channels[0],
                                                          p1, bs1, c1, n, oc, kernel_size, in_height, in_width, _stream()),
                  executed=2.0 * (-(-n * in_height * in_width // 128) * 128) * (-(-oc * k2 // 16) * 16) * (-(-cin // nt) * nt),
                  pipe="fp32", nbytes=4.0 * n * (oc * oh * ow + cin * in_height * in_width)), "kbn_conv2d_s2_backward_data")
    return grads


@_on_tensor_device
def conv2d_s2_backward_weight(inputs: Sequence[torch.Tensor], grad_out: torch.Tensor, kernel_size: int,
                              splits: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The gradient of conv_{k x k, stride 2, padding k // 2}(cat(inputs, 1)) with respect to its weight
    (kbn_conv2d_s2_backward_weight): -> F x sum(C_i) x k x k, plain OIHW.  The sum over the batch's output pixels is split over
    `splits` workgroups per tile (None: chosen from the shape) whose partial sums a second launch adds in split order: the bits
    are a function of the arguments (and of `splits`) alone."""
    return _conv_backward_weight("conv2d_s2_backward_weight", _s2_kernel_size, "conv_s2_bwd_weight", (kernel_size,), inputs, grad_out, splits, out)


def _channel_vector(fn: str, t, name: str, c: int) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise KbnError(f"{fn}: {name} must be a tensor, got {type(t).__name__}")
    v = t.detach()
    _require(v, name, 1)
    if v.numel() != c:
        raise KbnError(f"{fn}: {name} must hold {c} floats (one per channel), got {tuple(v.shape)}")
    return v.contiguous()


@_on_tensor_device
def batch_norm_stats(x: torch.Tensor):
    """(mean, biased variance) of an N x C x H x W tensor over N, H, W: C floats each (kbn_bn_stats_forward), what
    torch.nn.BatchNorm2d normalises with in train mode.  Two passes accumulated in fp64: no E[x^2] - mean^2."""
    lib = _lib.load()
    ptr, bs = _planes(x, "x")
    n, c, h, w = x.shape
    if n < 1 or c < 1 or h < 1 or w < 1:
        raise KbnError(f"batch_norm_stats: empty input {tuple(x.shape)}")
    mean = torch.empty(c, device=x.device, dtype=torch.float32)
    var = torch.empty(c, device=x.device, dtype=torch.float32)
    check(_launch("bn_stats", 0.0, lambda: lib.kbn_bn_stats_forward(ptr, bs, mean.data_ptr(), var.data_ptr(), n, c, h, w, _stream()),
                  nbytes=8.0 * n * c * h * w), "kbn_bn_stats_forward")
    return mean, var


def _bn_affine(fn: str, c: int, gamma, beta, mean, var, eps: float):
    """(scale = gamma rstd, shift = beta - mean scale, mean, rstd): C-length torch ops, as PoseConv2d.affine forms them."""
    g, b, m, v = (_channel_vector(fn, t, name, c) for t, name in ((gamma, "gamma"), (beta, "beta"), (mean, "mean"), (var, "var")))
    rstd = torch.rsqrt(v + eps)
    scale = g * rstd
    return scale, b - m * scale, m, rstd


def _bn_act_launch(u, scale, shift, negative_slope, out=None):
    lib = _lib.load()
    uptr, ubs = _planes(u, "u")
    n, c, h, w = u.shape
    out = _out_tensor(out, (n, c, h, w), u.device, "batch_norm_act: out", planes=True)
    optr, obs = _planes(out, "out")
    check(_launch("bn_act", 0.0, lambda: lib.kbn_bn_act_forward(uptr, ubs, scale.data_ptr(), shift.data_ptr(), optr, obs, n, c, h, w,
                                                                *_act_args(negative_slope), _stream()),
                  nbytes=8.0 * n * c * h * w), "kbn_bn_act_forward")
    return out


class _BatchNormAct(torch.autograd.Function):
    """act(batch_norm(u)) as a differentiable node.  Saved: u, gamma, beta and the two statistics vectors -- the normalised
    tensor and the activation's mask are recomputed from u in the backward (kbn_bn_act_backward)."""

    @staticmethod
    def forward(ctx, u, gamma, beta, mean, var, eps, negative_slope, batch):
        scale, shift, _, _ = _bn_affine("batch_norm_act", u.shape[1], gamma, beta, mean, var, eps)
        ctx.save_for_backward(u, gamma, beta, mean, var)
        ctx.args = (eps, negative_slope, batch)
        return _bn_act_launch(u.detach(), scale, shift, negative_slope)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        u, gamma, beta, mean, var = ctx.saved_tensors
        grad_u, grad_gamma, grad_beta = batch_norm_act_backward(u, grad_y, gamma, beta, mean, var, *ctx.args)
        need = ctx.needs_input_grad
        return (grad_u if need[0] else None, grad_gamma if need[1] else None, grad_beta if need[2] else None, None, None, None,
                None, None)


@_on_tensor_device
def batch_norm_act(u: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, mean: torch.Tensor, var: torch.Tensor,
                   eps: float = 1e-5, negative_slope: Optional[float] = 0.2, batch: bool = False,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act((u - mean) / sqrt(var + eps) * gamma + beta) per channel, act = max(v, slope v) (`negative_slope` None: none), as
    y = act(u * scale + shift) in one launch (kbn_bn_act_forward).  `mean` / `var`: the running statistics, or with `batch` the
    statistics of u itself (batch_norm_stats) -- the flag only tells the backward whether they depend on u.  Differentiable
    with respect to u, gamma and beta when grad mode is on and one of them requires grad (one node, no double backward); `mean`
    and `var` are data: one that requires grad is an error.  `out` (a tensor or channel slice to write into) only without autograd."""
    _require(u, "u", 4)
    if u.shape[0] < 1 or u.shape[1] < 1 or u.shape[2] < 1 or u.shape[3] < 1:
        raise KbnError(f"batch_norm_act: empty input {tuple(u.shape)}")
    for t, name in ((gamma, "gamma"), (beta, "beta"), (mean, "mean"), (var, "var")):
        _channel_vector("batch_norm_act", t, name, u.shape[1])
    if torch.is_grad_enabled():
        for t, name in ((mean, "mean"), (var, "var")):
            if t.requires_grad:
                raise KbnError(f"batch_norm_act: {name} requires grad, but it is data and gets no gradient (gradients exist for u, "
                               "gamma, beta); detach it")
        if any(t.requires_grad for t in (u, gamma, beta)):
            if out is not None:
                raise KbnError("batch_norm_act: `out` cannot be given when the call is recorded for autograd")
            _planes(u, "u")
            return _BatchNormAct.apply(u, gamma, beta, mean, var, float(eps), negative_slope, bool(batch))
    scale, shift, _, _ = _bn_affine("batch_norm_act", u.shape[1], gamma, beta, mean, var, eps)
    return _bn_act_launch(u.detach(), scale, shift, negative_slope, out)


@_on_tensor_device
def batch_norm_act_backward(u: torch.Tensor, grad_y: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, mean: torch.Tensor,
                            var: torch.Tensor, eps: float = 1e-5, negative_slope: Optional[float] = 0.2, batch: bool = False):
    """The gradient of `batch_norm_act`: (grad_u N x C x H x W, grad_gamma, grad_beta C floats each), two launches
    (kbn_bn_act_backward).  The first sums g_z and g_z xhat per channel in fp64 and a fixed order (g_z = grad_y where
    z = u scale + shift > 0, slope grad_y elsewhere; xhat recomputed from u); the second is elementwise.  With `batch` the
    statistics are functions of u (torch.nn.BatchNorm2d in train mode); without, constants."""
    lib = _lib.load()
    uptr, ubs = _planes(u.detach() if isinstance(u, torch.Tensor) else u, "u")
    n, c, h, w = u.shape
    if n < 1 or c < 1 or h < 1 or w < 1:
        raise KbnError(f"batch_norm_act_backward: empty input {tuple(u.shape)}")
    if not isinstance(grad_y, torch.Tensor) or tuple(grad_y.shape) != (n, c, h, w):
        raise KbnError(f"batch_norm_act_backward: grad_y must be {(n, c, h, w)} like u, got "
                       f"{tuple(grad_y.shape) if isinstance(grad_y, torch.Tensor) else type(grad_y).__name__}")
    gy = grad_y.detach()
    _require(gy, "grad_y", 4)
    gy = gy.contiguous()
    scale, shift, m, rstd = _bn_affine("batch_norm_act_backward", c, gamma, beta, mean, var, eps)
    sums = torch.empty(2 * c, device=u.device, dtype=torch.float64)
    grad_u = torch.empty((n, c, h, w), device=u.device, dtype=torch.float32)
    check(_launch("bn_act_backward", 0.0,
                  lambda: lib.kbn_bn_act_backward(uptr, ubs, gy.data_ptr(), c * h * w, scale.data_ptr(), shift.data_ptr(), m.data_ptr(),
                                                  rstd.data_ptr(), sums.data_ptr(), grad_u.data_ptr(), c * h * w, n, c, h, w,
                                                  *_act_args(negative_slope), 1 if batch else 0, _stream()),
                  nbytes=20.0 * n * c * h * w), "kbn_bn_act_backward")
    return grad_u, sums[c:].float(), sums[:c].float()


# ---- BatchNorm on the statistics of a batch spread over several ranks (csrc/bn_sync.hip) ----
# Everything between the ranks is an fp64 device vector; the four operators take the GATHERED buffers as arguments (row r: rank
# r's vector), so one process can stack the partial results of several shards and run the whole algebra without a collective.
def _gathered(fn: str, t, name: str, width: int) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float64:
        raise KbnError(f"{fn}: {name} must be a float64 CUDA/HIP tensor")
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] != width or not t.is_contiguous():
        raise KbnError(f"{fn}: {name} must be a contiguous ranks x {width} tensor, got {tuple(t.shape)} with strides {t.stride()}")
    return t


@_on_tensor_device
def batch_norm_moments(x: torch.Tensor) -> torch.Tensor:
    """This rank's record of an N x C x H x W tensor: 2 C + 1 doubles (N H W, the C means, the C sums of centred squares) -- the
    two fp64 passes of batch_norm_stats, not rounded to fp32 (kbn_bn_moments_forward)."""
    lib = _lib.load()
    ptr, bs = _planes(x, "x")
    n, c, h, w = x.shape
    if n < 1 or c < 1 or h < 1 or w < 1:
        raise KbnError(f"batch_norm_moments: empty input {tuple(x.shape)}")
    record = torch.empty(2 * c + 1, device=x.device, dtype=torch.float64)
    check(_launch("bn_moments", 0.0, lambda: lib.kbn_bn_moments_forward(ptr, bs, record.data_ptr(), n, c, h, w, _stream()),
                  nbytes=8.0 * n * c * h * w), "kbn_bn_moments_forward")
    return record


@_on_tensor_device
def batch_norm_moments_merge(gathered: torch.Tensor):
    """(mean, biased variance, unbiased variance), C floats each, of the frames of every rank from the ranks x (2 C + 1) records of
    batch_norm_moments: merged pairwise in row order in fp64 and rounded once (kbn_bn_moments_merge).  With one row, mean and
    biased variance are batch_norm_stats's.  The unbiased variance of a batch of one value per channel is not finite."""
    lib = _lib.load()
    if not isinstance(gathered, torch.Tensor) or gathered.dim() != 2 or gathered.shape[1] < 3 or gathered.shape[1] % 2 == 0:
        raise KbnError("batch_norm_moments_merge: gathered must be a ranks x (2 C + 1) tensor")
    world, c = gathered.shape[0], (gathered.shape[1] - 1) // 2
    g = _gathered("batch_norm_moments_merge", gathered, "gathered", 2 * c + 1)
    mean, var, unbiased = (torch.empty(c, device=g.device, dtype=torch.float32) for _ in range(3))
    check(_launch("bn_moments_merge", 0.0, lambda: lib.kbn_bn_moments_merge(g.data_ptr(), world, c, mean.data_ptr(), var.data_ptr(),
                                                                            unbiased.data_ptr(), _stream()),
                  nbytes=8.0 * g.numel()), "kbn_bn_moments_merge")
    return mean, var, unbiased


def _bn_backward_args(fn: str, u, grad_y):
    uptr, ubs = _planes(u.detach() if isinstance(u, torch.Tensor) else u, "u")
    n, c, h, w = u.shape
    if n < 1 or c < 1 or h < 1 or w < 1:
        raise KbnError(f"{fn}: empty input {tuple(u.shape)}")
    if not isinstance(grad_y, torch.Tensor) or tuple(grad_y.shape) != (n, c, h, w):
        raise KbnError(f"{fn}: grad_y must be {(n, c, h, w)} like u, got "
                       f"{tuple(grad_y.shape) if isinstance(grad_y, torch.Tensor) else type(grad_y).__name__}")
    gptr, gbs = _planes(grad_y.detach(), "grad_y")
    return uptr, ubs, gptr, gbs, n, c, h, w


@_on_tensor_device
def batch_norm_act_backward_sums(u: torch.Tensor, grad_y: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, mean: torch.Tensor,
                                 var: torch.Tensor, eps: float = 1e-5, negative_slope: Optional[float] = 0.2) -> torch.Tensor:
    """The first launch of batch_norm_act_backward alone (kbn_bn_act_backward_sums): 2 C doubles, sum g_z (this rank's gradient
    of beta) then sum g_z xhat (of gamma) over this rank's frames, xhat on the given -- merged -- statistics."""
    lib = _lib.load()
    uptr, ubs, gptr, gbs, n, c, h, w = _bn_backward_args("batch_norm_act_backward_sums", u, grad_y)
    scale, shift, m, rstd = _bn_affine("batch_norm_act_backward_sums", c, gamma, beta, mean, var, eps)
    sums = torch.empty(2 * c, device=u.device, dtype=torch.float64)
    check(_launch("bn_act_backward_sums", 0.0,
                  lambda: lib.kbn_bn_act_backward_sums(uptr, ubs, gptr, gbs, scale.data_ptr(), shift.data_ptr(), m.data_ptr(),
                                                       rstd.data_ptr(), sums.data_ptr(), n, c, h, w, *_act_args(negative_slope), _stream()),
                  nbytes=8.0 * n * c * h * w), "kbn_bn_act_backward_sums")
    return sums


@_on_tensor_device
def batch_norm_act_backward_sync(u: torch.Tensor, grad_y: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, mean: torch.Tensor,
                                 var: torch.Tensor, gathered_sums: torch.Tensor, gathered_moments: torch.Tensor, rank: int,
                                 eps: float = 1e-5, negative_slope: Optional[float] = 0.2) -> torch.Tensor:
    """grad_u of rank `rank` (kbn_bn_act_backward_sync_apply): scale (g_z - (S1 + xhat S2) / c_rank) with S the sum of the rows of
    `gathered_sums` (ranks x 2 C, from batch_norm_act_backward_sums) weighted c_r / M in row order; the counts are column 0 of
    `gathered_moments` (ranks x (2 C + 1), what the forward merged).  The divisor is the rank's own count: with per-rank losses
    that are means over the rank's frames, GradientAverager's n_r / n weights then give the gradient of the global mean."""
    lib = _lib.load()
    fn = "batch_norm_act_backward_sync"
    uptr, ubs, gptr, gbs, n, c, h, w = _bn_backward_args(fn, u, grad_y)
    gs = _gathered(fn, gathered_sums, "gathered_sums", 2 * c)
    gm = _gathered(fn, gathered_moments, "gathered_moments", 2 * c + 1)
    world, rank = gs.shape[0], int(rank)
    if gm.shape[0] != world or not 0 <= rank < world:
        raise KbnError(f"{fn}: rank {rank} with {world} rows of sums and {gm.shape[0]} of moments")
    scale, shift, m, rstd = _bn_affine(fn, c, gamma, beta, mean, var, eps)
    grad_u = torch.empty((n, c, h, w), device=u.device, dtype=torch.float32)
    check(_launch("bn_act_backward_sync_apply", 0.0,
                  lambda: lib.kbn_bn_act_backward_sync_apply(uptr, ubs, gptr, gbs, scale.data_ptr(), shift.data_ptr(), m.data_ptr(),
                                                             rstd.data_ptr(), gs.data_ptr(), gm.data_ptr(), world, rank,
                                                             grad_u.data_ptr(), c * h * w, n, c, h, w, *_act_args(negative_slope),
                                                             _stream()),
                  nbytes=12.0 * n * c * h * w), "kbn_bn_act_backward_sync_apply")
    return grad_u


def _bn_act_sync_forward(u, gamma, beta, group, eps, negative_slope):
    gathered = group.gather(batch_norm_moments(u))
    mean, var, unbiased = batch_norm_moments_merge(gathered)
    scale, shift, _, _ = _bn_affine("batch_norm_act_sync", u.shape[1], gamma, beta, mean, var, eps)
    return _bn_act_launch(u, scale, shift, negative_slope), mean, var, unbiased, gathered


class _BatchNormActSync(torch.autograd.Function):
    """_BatchNormAct on the statistics of every rank's frames: one collective in the forward (the records), one in the backward
    (the sums).  Saved: u, gamma, beta, the merged statistics and the gathered records (the counts)."""

    @staticmethod
    def forward(ctx, u, gamma, beta, group, eps, negative_slope):
        y, mean, var, unbiased, gathered = _bn_act_sync_forward(u.detach(), gamma, beta, group, eps, negative_slope)
        ctx.save_for_backward(u, gamma, beta, mean, var, gathered)
        ctx.args = (group, eps, negative_slope)
        ctx.mark_non_differentiable(mean, var, unbiased)
        return y, mean, var, unbiased

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y, *_):
        u, gamma, beta, mean, var, gathered = ctx.saved_tensors
        group, eps, negative_slope = ctx.args
        c = u.shape[1]
        grad_y = grad_y.contiguous()
        sums = batch_norm_act_backward_sums(u, grad_y, gamma, beta, mean, var, eps, negative_slope)
        need = ctx.needs_input_grad
        grad_u = None
        if need[0] or group.collective:      # every rank takes part in the collective, whatever it needs itself
            gathered_sums = group.gather(sums)
        if need[0]:
            grad_u = batch_norm_act_backward_sync(u, grad_y, gamma, beta, mean, var, gathered_sums, gathered, group.rank, eps, negative_slope)
        return (grad_u if need[0] else None, sums[c:].float() if need[1] else None, sums[:c].float() if need[2] else None, None, None, None)


@_on_tensor_device
def batch_norm_act_sync(u: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, group, eps: float = 1e-5,
                        negative_slope: Optional[float] = 0.2, return_stats: bool = False):
    """batch_norm_act(batch=True) on the statistics of the frames of EVERY rank of `group` (a kb.dist.BatchNormGroup): each rank's
    fp64 moments are gathered and merged in rank order, so all ranks normalise with the same bits and compute what one process
    computes on the whole batch.  Differentiable with respect to u, gamma and beta (one node, no double backward); the backward
    gathers the ranks' two per-channel sums.  grad_gamma and grad_beta are this rank's own sums, and grad_u is in the units of
    this rank's loss: GradientAverager.average(n_local, n_global) completes them.  Every rank must make the same calls in the same
    order -- in the backward too -- and hold at least one frame.  `return_stats`: (y, mean, biased variance, unbiased variance),
    the merged statistics a running-statistics update needs."""
    _require(u, "u", 4)
    if u.shape[0] < 1 or u.shape[1] < 1 or u.shape[2] < 1 or u.shape[3] < 1:
        raise KbnError(f"batch_norm_act_sync: empty input {tuple(u.shape)} (a rank without frames cannot join the collectives)")
    for t, name in ((gamma, "gamma"), (beta, "beta")):
        _channel_vector("batch_norm_act_sync", t, name, u.shape[1])
    _planes(u, "u")
    if torch.is_grad_enabled() and any(t.requires_grad for t in (u, gamma, beta)):
        out = _BatchNormActSync.apply(u, gamma, beta, group, float(eps), negative_slope)
    else:
        out = _bn_act_sync_forward(u.detach(), gamma, beta, group, float(eps), negative_slope)[:4]
    return out if return_stats else out[0]


_UNIT_AFFINE = {}


def _unit_affine(device, c: int):
    key = (device, c)
    if key not in _UNIT_AFFINE:
        _UNIT_AFFINE[key] = (torch.ones(c, device=device, dtype=torch.float32), torch.zeros(c, device=device, dtype=torch.float32))
    return _UNIT_AFFINE[key]


def _conv2d_s2_launch(inputs, weight, packed):
    oc, _, k, _ = weight.shape
    if packed is None:
        packed = pack_conv2d_s2_affine_weight(weight)
    ones, zeros = _unit_affine(weight.device, oc)
    return conv2d_s2_affine([t.detach() for t in inputs], packed, ones, zeros, oc, k, negative_slope=None)


@_on_tensor_device
def conv2d_s2(inputs: Sequence[torch.Tensor], weight: torch.Tensor, packed: Optional[torch.Tensor] = None, packed_t=None) -> torch.Tensor:
    """conv_{k x k, stride 2, padding k // 2}(cat(inputs, 1)), no bias (k in {3, 5, 7}): conv2d_s2_affine's kernel with unit
    scale, zero shift and no activation.  Differentiable with respect to the weight and to every input that requires grad (one
    node, no double backward).  `packed`: the weight's pack_conv2d_s2_affine_weight blob when the caller caches it; `packed_t`:
    a callable weight -> its pack_conv2d_s2_backward_data_weight blob, asked only when a data gradient is needed."""
    inputs = list(inputs)
    w = _weight(weight)
    if w.shape[2] != w.shape[3]:
        raise KbnError("square kernels only")
    _s2_kernel_size("conv2d_s2", w.shape[2])
    _, _, _, _, _, cin = _conv_inputs("conv2d_s2", inputs)
    if cin != w.shape[1]:
        raise KbnError(f"conv2d_s2: the inputs hold {cin} channels, the weight {tuple(w.shape)} takes {w.shape[1]}")
    if torch.is_grad_enabled() and (weight.requires_grad or any(t.requires_grad for t in inputs)):
        return _RecordedConv.apply(lambda ins, wt: _conv2d_s2_launch(ins, wt, packed), False, None, 2, packed_t, weight, *inputs)
    return _conv2d_s2_launch(inputs, w, packed)


def pose_head_recorded(latent: torch.Tensor, weight: torch.Tensor):
    """`pose_head` restated in torch operations that autograd records (N x C x a handful of pixels): (pose N x 4 x 4, dof N x 6)
    = (pose_matrix(dof), 0.01 * mean_hw(latent) W^T), the mean before the product as the kernel takes it.  Used only when
    gradients are on; the values agree with pose_head's within the dof gate, not bit for bit."""
    _require(latent, "latent", 4)
    _require(weight, "weight")
    c = latent.shape[1]
    if weight.numel() != 6 * c or weight.shape[0] != 6:
        raise KbnError(f"pose_head_recorded: weight must be 6 x {c} (x 1 x 1), got {tuple(weight.shape)}")
    dof = 0.01 * (latent.mean(dim=(2, 3)) @ weight.reshape(6, c).t())
    return pose_matrix(dof), dof


# ------------------------------------------------------------------ ResNet pose networks (eval mode)
@_on_tensor_device
def pack_conv2d_affine_weight(weight: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """OIHW (k in {1, 3, 7}, any channel counts) -> the [filter tile][K chunk][k][filters] order conv2d_affine reads
    (kbn_conv2d_affine_pack_weight; not the blob of conv2d_s2_affine); `out`: an existing blob of the right size to re-pack into."""
    return _pack_pose_weight("conv2d_affine", "conv2d_affine", "1, 3 or 7", weight, out)


@_on_tensor_device
def conv2d_affine(inputs: Sequence[torch.Tensor], packed_weight: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor,
                  out_channels: int, kernel_size: int, stride: int = 1, negative_slope: Optional[float] = 0.2,
                  residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act(act(conv_{k x k, stride, padding k // 2}(cat(inputs, 1)) * scale + shift) + residual) (kbn_conv2d_affine_forward): a
    net_utils.Conv2d with eval-mode BatchNorm2d (reference src/net_utils.py:120-141) and, with `residual`, the add and the
    second activation that end a ResNetBlock (src/net_utils.py:643-667), in one launch.  Without `residual`: one activation.
    `inputs`: one or two N x C_i x H x W tensors read in place; k in {1, 3, 7}, stride in {1, 2}; `scale` / `shift`: out_channels
    floats; `negative_slope` None: no activation at all; `residual` / `out`: N x out_channels x ceil(H / stride) x ceil(W / stride)
    tensors or channel slices."""
    lib = _lib.load()
    if kernel_size not in (1, 3, 7):
        raise KbnError(f"conv2d_affine: kernel size 1, 3 or 7, got {kernel_size}")
    if stride not in (1, 2):
        raise KbnError(f"conv2d_affine: stride 1 or 2, got {stride}")
    inputs, srcs, n, h, w, cin, want = _affine_conv_args("conv2d_affine", lib.kbn_conv2d_affine_packed_weight_bytes, inputs,
                                                         packed_weight, scale, shift, out_channels, kernel_size)
    oh, ow = -(-h // stride), -(-w // stride)
    rptr, rbs = None, 0
    if residual is not None:
        rptr, rbs = _planes(residual, "residual")
        if tuple(residual.shape) != (n, out_channels, oh, ow):
            raise KbnError(f"conv2d_affine: residual is {tuple(residual.shape)}, the output {(n, out_channels, oh, ow)}")
    out = _out_tensor(out, (n, out_channels, oh, ow), inputs[0].device, planes=True)
    optr, obs = _planes(out, "out")
    arr = (ConvSrc * len(srcs))(*srcs)
    k2 = kernel_size * kernel_size
    # `want` = padded K x padded filter count, whatever the kernel's K chunk and filter tile are: no copy of its constants here
    check(_launch(f"conv_affine<{kernel_size},{stride}>", 2.0 * n * oh * ow * cin * k2 * out_channels,
                  lambda: lib.kbn_conv2d_affine_forward(arr, len(srcs), packed_weight.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                                                        rptr, rbs, optr, obs, n, out_channels, kernel_size, stride, h, w,
                                                        *_act_args(negative_slope), _stream()),
                  executed=2.0 * (-(-n * oh * ow // 128) * 128) * want, pipe="fp32",
                  nbytes=_src_bytes(srcs, n) + 4.0 * n * oh * ow * out_channels * (2 if residual is not None else 1)),
          "kbn_conv2d_affine_forward")
    return out


def _maxpool3x3s2_launch(x, out):
    lib = _lib.load()
    ptr, bs = _planes(x, "x")
    n, c, h, w = x.shape
    if n < 1 or c < 1 or h < 1 or w < 1:
        raise KbnError(f"maxpool3x3s2: empty input {tuple(x.shape)}")
    oh, ow = (h + 1) // 2, (w + 1) // 2
    out = _out_tensor(out, (n, c, oh, ow), x.device, planes=True)
    optr, obs = _planes(out, "out")
    check(_launch("maxpool3x3s2", 8.0 * n * c * oh * ow,
                  lambda: lib.kbn_maxpool3x3s2_forward(ptr, bs, optr, obs, n, c, h, w, _stream()),
                  nbytes=4.0 * n * c * (h * w + oh * ow)), "kbn_maxpool3x3s2_forward")
    return out


@_on_tensor_device
def maxpool3x3s2(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """torch.nn.MaxPool2d(3, stride=2, padding=1) (kbn_maxpool3x3s2_forward; reference src/networks.py:747): N x C x H x W ->
    N x C x ceil(H / 2) x ceil(W / 2).  Padding never wins; a NaN in the window is the result.  `out`: a tensor or channel slice,
    only without autograd.  Differentiable with respect to x when grad mode is on and x requires grad (maxpool3x3s2_backward)."""
    if isinstance(x, torch.Tensor) and x.requires_grad and torch.is_grad_enabled():
        if out is not None:
            raise KbnError("maxpool3x3s2: `out` cannot be given when the call is recorded for autograd")
        _planes(x, "x")
        return _MaxPool3x3S2.apply(x)
    return _maxpool3x3s2_launch(x, out)


# ------------------------------------------------------------------ ResNet pose networks (training: csrc/conv_affine_backward.hip)
def _backward_case(fn: str, kernel_size, stride):
    if (kernel_size, stride) not in _BACKWARD_CASES:
        raise KbnError(f"{fn}: (kernel size, stride) one of {_BACKWARD_CASES}, got ({kernel_size}, {stride}); the 3 x 3 and 7 x 7 convs "
                       "at stride 2 have conv2d_s2_backward_data / conv2d_s2_backward_weight")


@_on_tensor_device
def conv2d_backward_weight(inputs: Sequence[torch.Tensor], grad_out: torch.Tensor, kernel_size: int, stride: int,
                           splits: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The gradient of conv_{k x k, stride, padding k // 2}(cat(inputs, 1)) with respect to its weight for (k, stride) in
    {(3, 1), (1, 1), (1, 2)} (kbn_conv2d_backward_weight): -> F x sum(C_i) x k x k, plain OIHW.  The contract of
    conv2d_s2_backward_weight: the sum over the batch's output pixels is split over `splits` workgroups per tile (None: chosen
    from the shape) whose partial sums a second launch adds in split order; the bits are a function of the arguments (and of
    `splits`) alone."""
    return _conv_backward_weight("conv2d_backward_weight", _backward_case, "conv_bwd_weight", (kernel_size, stride), inputs, grad_out, splits, out)


@_on_tensor_device
def pack_conv2d_backward_data_weight(weight: torch.Tensor, stride: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """OIHW -> the blob conv2d_backward_data reads at this stride (kbn_conv2d_backward_data_pack_weight).  Stride 1 (k 1 or 3): the
    weight transposed (O <-> I) with both tap axes flipped, in conv2d_affine's packed order, and a unit scale and zero shift
    behind it -- the data gradient is then that forward conv of grad_out.  (1, 2): the weight as it is.  `out`: a blob to re-pack into."""
    lib = _lib.load()
    w = _weight(weight)
    oc, cin, kh, kw = w.shape
    if kh != kw:
        raise KbnError("square kernels only")
    _backward_case("pack_conv2d_backward_data_weight", kh, stride)
    nbytes = lib.kbn_conv2d_backward_data_packed_weight_bytes(oc, cin, kh, stride)
    if nbytes == 0:
        raise KbnError(f"pack_conv2d_backward_data_weight: unsupported weight shape {tuple(w.shape)}")
    return _pack_into(out, nbytes, w, lambda p: lib.kbn_conv2d_backward_data_pack_weight(w.data_ptr(), p, oc, cin, kh, stride, _stream()),
                      "kbn_conv2d_backward_data_pack_weight")


@_on_tensor_device
def conv2d_backward_data(grad_out: torch.Tensor, packed_weight: torch.Tensor, in_channels: int, kernel_size: int, stride: int,
                         in_height: int, in_width: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The gradient of conv_{k x k, stride, padding k // 2}(x) with respect to its one input for (k, stride) in {(3, 1), (1, 1),
    (1, 2)} (kbn_conv2d_backward_data): grad_out N x F x ceil(H / stride) x ceil(W / stride) -> N x in_channels x H x W, every
    element written by the one launch (at (1, 2): zeros at the pixels the conv never read).  `packed_weight`:
    pack_conv2d_backward_data_weight of the F x in_channels x k x k weight at this stride.  `out`: a tensor or channel slice."""
    lib = _lib.load()
    _backward_case("conv2d_backward_data", kernel_size, stride)
    in_channels = int(in_channels)
    if in_channels < 1 or in_height < 1 or in_width < 1:
        raise KbnError(f"conv2d_backward_data: empty input {in_channels} x {in_height} x {in_width}")
    gptr, gbs = _planes(grad_out, "grad_out")
    n, oc, oh, ow = grad_out.shape
    if n < 1 or oc < 1 or (oh, ow) != (-(-in_height // stride), -(-in_width // stride)):
        raise KbnError(f"conv2d_backward_data: grad_out is {tuple(grad_out.shape)}, the conv of a {in_height} x {in_width} input at "
                       f"stride {stride} has {-(-in_height // stride)} x {-(-in_width // stride)} maps")
    _require(packed_weight, "packed_weight", 1)
    want = lib.kbn_conv2d_backward_data_packed_weight_bytes(oc, in_channels, kernel_size, stride) // 4
    if want == 0 or packed_weight.numel() != want or not packed_weight.is_contiguous():
        raise KbnError(f"conv2d_backward_data: packed_weight holds {packed_weight.numel()} floats, a {oc} x {in_channels} x "
                       f"{kernel_size} x {kernel_size} weight packs into {want} at stride {stride}")
    out = _out_tensor(out, (n, in_channels, in_height, in_width), grad_out.device, planes=True)
    optr, obs = _planes(out, "out")
    k2 = kernel_size * kernel_size
    name = f"conv_affine<{kernel_size},1> (data gradient)" if stride == 1 else "conv1x1s2_bwd_data"
    check(_launch(name, 2.0 * n * oh * ow * in_channels * k2 * oc,
                  lambda: lib.kbn_conv2d_backward_data(gptr, gbs, packed_weight.data_ptr(), optr, obs, n, oc, in_channels, kernel_size,
                                                       stride, in_height, in_width, _stream()),
                  executed=2.0 * (-(-n * oh * ow // 128) * 128) * (want - 2 * in_channels) if stride == 1 else None,
                  pipe="fp32" if stride == 1 else None, nbytes=4.0 * n * (oc * oh * ow + in_channels * in_height * in_width)),
          "kbn_conv2d_backward_data")
    return out


def _conv2d_pose_launch(inputs, weight, stride, packed):
    oc, _, k, _ = weight.shape
    if packed is None:
        packed = pack_conv2d_affine_weight(weight)
    ones, zeros = _unit_affine(weight.device, oc)
    return conv2d_affine([t.detach() for t in inputs], packed, ones, zeros, oc, k, stride=stride, negative_slope=None)


# ------------------------------------------------------------------ conv gradients: one dispatch, one recorded node
def _weight_gradient(inputs, g, k, stride):
    """The weight gradient of a conv over one to three concatenated inputs through the entry points that take two: it is linear in
    the input-channel blocks, so a third input is a second call and the results are joined along dim 1."""
    fn = (lambda ins: conv2d_s2_backward_weight(ins, g, k)) if _S2_FAMILY[(k, stride)] else (lambda ins: conv2d_backward_weight(ins, g, k, stride))
    if len(inputs) <= 2:
        return fn(inputs)
    return torch.cat([fn(inputs[:2]), fn(inputs[2:])], dim=1)


@_on_tensor_device
def pack_conv2d_data_gradient_weight(weight: torch.Tensor, stride: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """OIHW -> the blob the data gradient of conv_{k x k, stride, padding k // 2} reads: pack_conv2d_s2_backward_data_weight for k in
    {3, 5, 7} at stride 2, pack_conv2d_backward_data_weight(weight, stride) at (3, 1), (1, 1) and (1, 2).  `out`: a blob to re-pack into."""
    k = weight.shape[2] if isinstance(weight, torch.Tensor) and weight.dim() == 4 else None
    if _S2_FAMILY.get((k, stride)):
        return pack_conv2d_s2_backward_data_weight(weight, out)
    return pack_conv2d_backward_data_weight(weight, stride, out)


def _data_gradient(g, weight, k, stride, cin, h, w, packed_t):
    """One launch over all `cin` channels into one buffer (the caller slices it by input).  `packed_t`: weight -> its
    pack_conv2d_data_gradient_weight blob, from the caller's cache; None: packed here."""
    blob = packed_t(weight) if packed_t is not None else pack_conv2d_data_gradient_weight(weight, stride)
    if _S2_FAMILY[(k, stride)]:
        return conv2d_s2_backward_data(g, blob, [cin], k, h, w)[0]
    return conv2d_backward_data(g, blob, cin, k, stride, h, w)


class _RecordedConv(torch.autograd.Function):
    """[act](conv(cat(inputs))), no bias, as the one differentiable conv node of the three networks.  `launch(inputs, weight)` is
    the network's forward launch; `epilogue`: that launch applied the activation `negative_slope`, so the output y is saved too (the
    activation's branch is its sign) and the backward starts with add_act_backward.  Saved otherwise: the weight and the inputs,
    nothing the forward computed.  Backward: the weight gradient through the two-input entry points, and -- only when an input asks
    -- ONE data-gradient launch over all channels, returned as channel slices of its buffer."""

    @staticmethod
    def forward(ctx, launch, epilogue, negative_slope, stride, packed_t, weight, *inputs):
        y = launch(inputs, weight.detach())
        ctx.save_for_backward(weight, *inputs, *([y] if epilogue else []))
        ctx.args = (epilogue, negative_slope, stride, packed_t)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        epilogue, slope, stride, packed_t = ctx.args
        weight, *inputs = ctx.saved_tensors
        g = grad_y.contiguous()
        if epilogue:
            g = add_act_backward(inputs.pop(), g, slope)
        k = weight.shape[2]
        need = ctx.needs_input_grad[5:]
        grad_w = _weight_gradient(inputs, g, k, stride) if need[0] else None
        grads = [None] * len(inputs)
        if any(need[1:]):
            h, w = inputs[0].shape[2:]
            buf = _data_gradient(g, weight, k, stride, weight.shape[1], h, w, packed_t)
            at = 0
            for i, t in enumerate(inputs):
                if need[1 + i]:
                    grads[i] = buf[:, at:at + t.shape[1]]
                at += t.shape[1]
        return (None,) * 5 + (grad_w,) + tuple(grads)


@_on_tensor_device
def conv2d_pose(inputs: Sequence[torch.Tensor], weight: torch.Tensor, stride: int, packed: Optional[torch.Tensor] = None,
                packed_t=None) -> torch.Tensor:
    """conv_{k x k, stride, padding k // 2}(cat(inputs, 1)), no bias, k in {1, 3, 7} at stride 1 or 2: conv2d_affine's kernel with
    unit scale, zero shift and no activation.  Differentiable with respect to the weight and to every input that requires grad
    (one node, no double backward); a data gradient at (k, stride) outside (3, 2) and (7, 2) takes ONE input.  `packed`: the
    weight's pack_conv2d_affine_weight blob when the caller caches it; `packed_t`: a callable weight -> the data gradient's blob
    (pack_conv2d_s2_backward_data_weight at (3, 2) and (7, 2), pack_conv2d_backward_data_weight(weight, stride) elsewhere), asked
    only when a data gradient is needed."""
    inputs = list(inputs)
    w = _weight(weight)
    if w.shape[2] != w.shape[3]:
        raise KbnError("square kernels only")
    k = w.shape[2]
    if k not in (1, 3, 7) or stride not in (1, 2):
        raise KbnError(f"conv2d_pose: kernel size 1, 3 or 7 at stride 1 or 2, got {k} at {stride}")
    _, _, _, _, _, cin = _conv_inputs("conv2d_pose", inputs)
    if cin != w.shape[1]:
        raise KbnError(f"conv2d_pose: the inputs hold {cin} channels, the weight {tuple(w.shape)} takes {w.shape[1]}")
    if torch.is_grad_enabled() and (weight.requires_grad or any(t.requires_grad for t in inputs)):
        if (k, stride) not in _S2_FAMILY:
            raise KbnError(f"conv2d_pose: no backward pass for kernel size {k} at stride {stride}")
        if any(t.requires_grad for t in inputs) and len(inputs) > 1 and not _S2_FAMILY[(k, stride)]:
            raise KbnError(f"conv2d_pose: the data gradient at kernel size {k}, stride {stride} takes one input, got {len(inputs)}")
        return _RecordedConv.apply(lambda ins, wt: _conv2d_pose_launch(ins, wt, stride, packed), False, None, stride, packed_t, weight, *inputs)
    return _conv2d_pose_launch(inputs, w, stride, packed)


@_on_tensor_device
def maxpool3x3s2_backward(x: torch.Tensor, grad_out: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The gradient of maxpool3x3s2 (kbn_maxpool3x3s2_backward): x N x C x H x W (the pool's input), grad_out N x C x ceil(H / 2) x
    ceil(W / 2) -> N x C x H x W.  Every window's gradient goes to its FIRST maximum in row-major order (the forward's own scan;
    ties are the rule behind a relu); a pixel sums the at most four windows that chose it in (oy, ox) order.  One launch, no atomics."""
    lib = _lib.load()
    xptr, xbs = _planes(x.detach() if isinstance(x, torch.Tensor) else x, "x")
    n, c, h, w = x.shape
    if n < 1 or c < 1 or h < 1 or w < 1:
        raise KbnError(f"maxpool3x3s2_backward: empty input {tuple(x.shape)}")
    oh, ow = (h + 1) // 2, (w + 1) // 2
    gptr, gbs = _planes(grad_out, "grad_out")
    if tuple(grad_out.shape) != (n, c, oh, ow):
        raise KbnError(f"maxpool3x3s2_backward: grad_out is {tuple(grad_out.shape)}, the pool of {tuple(x.shape)} is {(n, c, oh, ow)}")
    out = _out_tensor(out, (n, c, h, w), x.device, planes=True)
    optr, obs = _planes(out, "out")
    check(_launch("maxpool3x3s2_bwd", 0.0,
                  lambda: lib.kbn_maxpool3x3s2_backward(xptr, xbs, gptr, gbs, optr, obs, n, c, h, w, _stream()),
                  nbytes=4.0 * n * c * (2 * h * w + oh * ow)), "kbn_maxpool3x3s2_backward")
    return out


class _MaxPool3x3S2(torch.autograd.Function):
    """maxpool3x3s2 as a differentiable node.  Saved: x -- the backward rescans the windows, no index tensor is kept."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return _maxpool3x3s2_launch(x.detach(), None)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        (x,) = ctx.saved_tensors
        return maxpool3x3s2_backward(x, grad_out.contiguous())


def _add_act_args(fn: str, a, b, names):
    for t, name in zip((a, b), names):
        _require(t, name)
    if a.shape != b.shape or a.numel() < 1:
        raise KbnError(f"{fn}: {names[0]} {tuple(a.shape)} and {names[1]} {tuple(b.shape)} must be one non-empty shape")
    if not a.is_contiguous() or not b.is_contiguous():
        raise KbnError(f"{fn}: {names[0]} and {names[1]} must be contiguous")


def _add_act_launch(a, b, negative_slope):
    lib = _lib.load()
    y = torch.empty_like(a)
    check(_launch("add_act", 0.0, lambda: lib.kbn_add_act_forward(a.data_ptr(), b.data_ptr(), y.data_ptr(), a.numel(),
                                                                 *_act_args(negative_slope), _stream()),
                  nbytes=12.0 * a.numel()), "kbn_add_act_forward")
    return y


@_on_tensor_device
def add_act_backward(y: torch.Tensor, grad_y: torch.Tensor, negative_slope: Optional[float] = 0.2) -> torch.Tensor:
    """The gradient of add_act with respect to EITHER addend (kbn_add_act_backward): grad_y where y > 0, negative_slope grad_y
    elsewhere -- y <= 0 takes the slope, so slope 0 puts exact zeros there, as torch.nn.functional.leaky_relu does.
    `negative_slope` None: grad_y itself, no launch."""
    _add_act_args("add_act_backward", y, grad_y, ("y", "grad_y"))
    if negative_slope is None:
        return grad_y
    lib = _lib.load()
    g = torch.empty_like(y)
    check(_launch("add_act_bwd", 0.0, lambda: lib.kbn_add_act_backward(y.data_ptr(), grad_y.data_ptr(), g.data_ptr(), y.numel(),
                                                                      *_act_args(negative_slope), _stream()),
                  nbytes=12.0 * y.numel()), "kbn_add_act_backward")
    return g


class _AddAct(torch.autograd.Function):
    """act(a + b) as a differentiable node.  Saved: y only (its sign is the sign of a + b for a slope >= 0)."""

    @staticmethod
    def forward(ctx, a, b, negative_slope):
        y = _add_act_launch(a.detach(), b.detach(), negative_slope)
        ctx.save_for_backward(y)
        ctx.slope = negative_slope
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        (y,) = ctx.saved_tensors
        g = add_act_backward(y, grad_y.contiguous(), ctx.slope)
        need = ctx.needs_input_grad
        return g if need[0] else None, g if need[1] else None, None


@_on_tensor_device
def add_act(a: torch.Tensor, b: torch.Tensor, negative_slope: Optional[float] = 0.2) -> torch.Tensor:
    """act(a + b) in one launch (kbn_add_act_forward), act = max(v, slope v), `negative_slope` None: the sum alone: the add and
    second activation that end a ResNetBlock (reference src/net_utils.py:666-667).  Two contiguous fp32 tensors of one shape.
    Differentiable with respect to both (one node, no double backward)."""
    _add_act_args("add_act", a, b, ("a", "b"))
    if negative_slope is not None and negative_slope < 0:
        raise KbnError(f"add_act: negative_slope must be >= 0 (the backward reads the branch from y's sign), got {negative_slope}")
    if torch.is_grad_enabled() and (a.requires_grad or b.requires_grad):
        return _AddAct.apply(a, b, negative_slope)
    return _add_act_launch(a.detach(), b.detach(), negative_slope)


# ------------------------------------------------------------------ depth network (training: csrc/kbnet_backward.hip)
def _resize_args(fn: str, t: torch.Tensor, name: str, small, large):
    ptr, bs = _planes(t, name)
    (h, w), (H, W) = small, large
    if min(t.shape) < 1 or h < 1 or w < 1:
        raise KbnError(f"{fn}: empty {name} {tuple(t.shape)}")
    if H < h or W < w:
        raise KbnError(f"{fn}: the resized map {H} x {W} must be at least the source's {h} x {w}")
    return ptr, bs


@_on_tensor_device
def resize_nearest_forward(x: torch.Tensor, height: int, width: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """torch.nn.functional.interpolate(x, size=(height, width), mode='nearest') for height >= H, width >= W
    (kbn_resize_nearest_forward): the index rule the forward convs resize by, as a tensor of its own.  x: N x C x H x W dense planes."""
    lib = _lib.load()
    n, c, h, w = x.shape if isinstance(x, torch.Tensor) and x.dim() == 4 else (0, 0, 0, 0)
    height, width = int(height), int(width)
    xptr, xbs = _resize_args("resize_nearest_forward", x, "x", (h, w), (height, width))
    out = _out_tensor(out, (n, c, height, width), x.device, "resize_nearest_forward: out", planes=True)
    optr, obs = _planes(out, "out")
    check(_launch("resize_nearest", 0.0, lambda: lib.kbn_resize_nearest_forward(xptr, xbs, optr, obs, n, c, h, w, height, width, _stream()),
                  nbytes=4.0 * n * c * (h * w + height * width)), "kbn_resize_nearest_forward")
    return out


@_on_tensor_device
def resize_nearest_backward(grad_out: torch.Tensor, height: int, width: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The gradient of resize_nearest_forward (kbn_resize_nearest_backward): grad_out N x C x H' x W' -> N x C x height x width, the
    SOURCE size.  A gather: every source pixel sums, in row-major order, the destination pixels the index rule maps to it."""
    lib = _lib.load()
    n, c, H, W = grad_out.shape if isinstance(grad_out, torch.Tensor) and grad_out.dim() == 4 else (0, 0, 0, 0)
    height, width = int(height), int(width)
    gptr, gbs = _resize_args("resize_nearest_backward", grad_out, "grad_out", (height, width), (H, W))
    out = _out_tensor(out, (n, c, height, width), grad_out.device, "resize_nearest_backward: out", planes=True)
    optr, obs = _planes(out, "out")
    check(_launch("resize_nearest_bwd", 0.0,
                  lambda: lib.kbn_resize_nearest_backward(gptr, gbs, optr, obs, n, c, height, width, H, W, _stream()),
                  nbytes=4.0 * n * c * (height * width + H * W)), "kbn_resize_nearest_backward")
    return out


class _ResizeNearest(torch.autograd.Function):
    """The nearest resize as a differentiable node; nothing is saved but the source size."""

    @staticmethod
    def forward(ctx, x, height, width):
        ctx.size = tuple(x.shape[2:])
        return resize_nearest_forward(x.detach(), height, width)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        return resize_nearest_backward(grad_out.contiguous(), *ctx.size), None, None


@_on_tensor_device
def resize_nearest(x: torch.Tensor, height: int, width: int) -> torch.Tensor:
    """resize_nearest_forward, differentiable with respect to x when grad mode is on and x requires grad (one node)."""
    if isinstance(x, torch.Tensor) and x.requires_grad and torch.is_grad_enabled():
        _planes(x, "x")
        return _ResizeNearest.apply(x, int(height), int(width))
    return resize_nearest_forward(x, height, width)


@_on_tensor_device
def kb_xyz_backward(z: torch.Tensor, coordinates: torch.Tensor, grad_xyz: torch.Tensor, negative_slope: Optional[float] = 0.2,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The gradient of xyz = coordinates * z, z = act(pre), with respect to `pre` (kbn_kb_xyz_backward): act'(z) sum_c coordinates_c
    grad_xyz_c, the branch read from z (z <= 0 takes the slope; `negative_slope` None: no activation).  z N x 1 x H x W; coordinates
    and grad_xyz N x 3 x H x W, either may be a channel slice."""
    lib = _lib.load()
    zptr, zbs = _planes(z, "z")
    n, _, h, w = z.shape
    if n < 1 or h < 1 or w < 1 or z.shape[1] != 1:
        raise KbnError(f"kb_xyz_backward: z must be a non-empty N x 1 x H x W tensor, got {tuple(z.shape)}")
    cptr, cbs = _planes(coordinates, "coordinates")
    gptr, gbs = _planes(grad_xyz, "grad_xyz")
    for t, name in ((coordinates, "coordinates"), (grad_xyz, "grad_xyz")):
        if tuple(t.shape) != (n, 3, h, w):
            raise KbnError(f"kb_xyz_backward: {name} is {tuple(t.shape)}, expected {(n, 3, h, w)}")
    out = _out_tensor(out, (n, 1, h, w), z.device, "kb_xyz_backward: out", planes=True)
    optr, obs = _planes(out, "out")
    check(_launch("kb_xyz_bwd", 0.0, lambda: lib.kbn_kb_xyz_backward(zptr, zbs, cptr, cbs, gptr, gbs, optr, obs, n, h, w,
                                                                     *_act_args(negative_slope), _stream()),
                  nbytes=4.0 * n * h * w * 8), "kbn_kb_xyz_backward")
    return out


@_on_tensor_device
def depth_map_backward(logits: torch.Tensor, depth: torch.Tensor, grad_depth: torch.Tensor, min_predict_depth: float,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The gradient of depth = d_min / (sigmoid(logits) + d_min / d_max) with respect to the logits (kbn_depth_map_backward):
    -grad_depth depth^2 / d_min * s (1 - s).  Three contiguous fp32 tensors of one shape: what depth_head(return_logits=True) gave
    and the incoming gradient.  `out`: a contiguous tensor of that shape to write into."""
    for t, name in ((logits, "logits"), (depth, "depth"), (grad_depth, "grad_depth")):
        _require(t, name)
        if t.shape != logits.shape or not t.is_contiguous() or t.numel() < 1:
            raise KbnError(f"depth_map_backward: {name} must be contiguous, non-empty and of one shape with logits, got {tuple(t.shape)}")
    if not min_predict_depth > 0:
        raise KbnError(f"depth_map_backward: min_predict_depth must be positive, got {min_predict_depth}")
    lib = _lib.load()
    g = _out_tensor(out, tuple(logits.shape), logits.device, "depth_map_backward: out")
    check(_launch("depth_map_bwd", 0.0, lambda: lib.kbn_depth_map_backward(logits.data_ptr(), depth.data_ptr(), grad_depth.data_ptr(),
                                                                          g.data_ptr(), logits.numel(), float(min_predict_depth), _stream()),
                  nbytes=16.0 * logits.numel()), "kbn_depth_map_backward")
    return g


def _kbnet_conv_launch(inputs, weight, stride, negative_slope, packed):
    oc, _, k, _ = weight.shape
    if packed is None:
        packed = pack_conv_weight(weight, stride)
    n, _, h, w = inputs[0].shape
    out = torch.empty((n, oc, -(-h // stride), -(-w // stride)), device=weight.device, dtype=torch.float32)
    return conv2d([tensor_src(t.detach(), f"inputs[{i}]") for i, t in enumerate(inputs)], packed, n, oc, k, stride, h, w, out,
                  negative_slope=negative_slope)


@_on_tensor_device
def conv2d_kbnet(inputs: Sequence[torch.Tensor], weight: torch.Tensor, stride: int, negative_slope: Optional[float] = 0.2,
                 packed: Optional[torch.Tensor] = None, packed_t=None) -> torch.Tensor:
    """act(conv_{k x k, stride, padding k // 2}(cat(inputs, 1))), no bias, act = max(v, slope v) in the conv's epilogue
    (`negative_slope` None: none), for (k, stride) in {(3, 1), (3, 2), (1, 1), (1, 2)} and one to three inputs read in place
    (kbn_conv2d_forward): a conv of the depth network.  Differentiable with respect to the weight and to every input that requires
    grad -- any of the inputs may be data -- as one node, no double backward.  `packed`: the weight's pack_conv_weight blob when the
    caller caches it; `packed_t`: a callable weight -> the data gradient's blob (pack_conv2d_s2_backward_data_weight at (3, 2),
    pack_conv2d_backward_data_weight(weight, stride) elsewhere), asked only when a data gradient is needed."""
    inputs = list(inputs)
    w = _weight(weight)
    if w.shape[2] != w.shape[3]:
        raise KbnError("square kernels only")
    k = w.shape[2]
    if (k, stride) not in _KBNET_CASES:
        raise KbnError(f"conv2d_kbnet: (kernel size, stride) one of {_KBNET_CASES}, got ({k}, {stride})")
    if not 1 <= len(inputs) <= 3:
        raise KbnError(f"conv2d_kbnet: one to three inputs, got {len(inputs)}")
    if negative_slope is not None and negative_slope < 0:
        raise KbnError(f"conv2d_kbnet: negative_slope must be >= 0 (the backward reads the branch from y's sign), got {negative_slope}")
    for i, t in enumerate(inputs):
        _planes(t, f"inputs[{i}]")
        if t.shape[0] != inputs[0].shape[0] or t.shape[2:] != inputs[0].shape[2:] or min(t.shape) < 1:
            raise KbnError(f"conv2d_kbnet: inputs[{i}] is {tuple(t.shape)} beside inputs[0] {tuple(inputs[0].shape)}")
    cin = sum(t.shape[1] for t in inputs)
    if cin != w.shape[1]:
        raise KbnError(f"conv2d_kbnet: the inputs hold {cin} channels, the weight {tuple(w.shape)} takes {w.shape[1]}")
    if torch.is_grad_enabled() and (weight.requires_grad or any(t.requires_grad for t in inputs)):
        return _RecordedConv.apply(lambda ins, wt: _kbnet_conv_launch(ins, wt, stride, negative_slope, packed), True, negative_slope, stride,
                                   packed_t, weight, *inputs)
    return _kbnet_conv_launch(inputs, w, stride, negative_slope, packed)


class _KbXyz(torch.autograd.Function):
    """xyz = coordinates * act(proj_depth(depth)) of a KB layer as a differentiable node.  Saved: depth, the weight, z and the
    coordinates the forward multiplied by.  Backward: kb_xyz_backward gives the pre-activation's gradient, then the 1 x 1 conv's two
    gradients."""

    @staticmethod
    def forward(ctx, depth, weight, coordinates, negative_slope, packed, packed_t):
        z = _kbnet_conv_launch([depth], weight.detach(), 1, negative_slope, packed)
        ctx.save_for_backward(depth, weight, z, coordinates)
        ctx.args = (negative_slope, packed_t)
        ctx.mark_non_differentiable(z)
        return scale_planes(coordinates, z), z

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_xyz, _):
        depth, weight, z, coordinates = ctx.saved_tensors
        slope, packed_t = ctx.args
        need = ctx.needs_input_grad
        # autograd hands over any layout (the stride-0 expand behind .sum(), channels-last, a step in W): dense planes -- KBNet's
        # channel slice of the fused conv's data-gradient buffer -- are read in place, anything else (what _planes refuses) is made
        # dense first
        n, c, h, w = grad_xyz.shape
        if grad_xyz.stride(3) != 1 or grad_xyz.stride(2) != w or grad_xyz.stride(1) != h * w:
            grad_xyz = grad_xyz.contiguous()
        g = kb_xyz_backward(z, coordinates, grad_xyz, slope)
        grad_w = _weight_gradient([depth], g, 1, 1) if need[1] else None
        grad_d = None
        if need[0]:
            h, w = depth.shape[2:]
            grad_d = _data_gradient(g, weight, 1, 1, depth.shape[1], h, w, packed_t)
        return grad_d, grad_w, None, None, None, None


@_on_tensor_device
def kb_xyz(depth: torch.Tensor, weight: torch.Tensor, coordinates: torch.Tensor, negative_slope: Optional[float] = 0.2,
           packed: Optional[torch.Tensor] = None, packed_t=None):
    """(xyz, z) of a KB layer (reference src/net_utils.py:1352-1359): z = act(conv_{1 x 1}(depth)) with `weight` 1 x C x 1 x 1,
    xyz = coordinates * z (scale_planes).  Differentiable with respect to depth and the weight (one node); `coordinates`
    (N x 3 x H x W, camera_coordinates) are data.  z is returned for inspection and carries no gradient."""
    w = _weight(weight)
    _planes(depth, "depth")
    if tuple(w.shape) != (1, depth.shape[1], 1, 1):
        raise KbnError(f"kb_xyz: weight must be 1 x {depth.shape[1]} x 1 x 1, got {tuple(w.shape)}")
    if coordinates.requires_grad:
        raise KbnError("kb_xyz: coordinates require grad, but they are data and get no gradient; detach them")
    if negative_slope is not None and negative_slope < 0:
        raise KbnError(f"kb_xyz: negative_slope must be >= 0, got {negative_slope}")
    if torch.is_grad_enabled() and (weight.requires_grad or depth.requires_grad):
        return _KbXyz.apply(depth, weight, coordinates, negative_slope, packed, packed_t)
    z = _kbnet_conv_launch([depth], w, 1, negative_slope, packed)
    return scale_planes(coordinates, z), z


_IDENTITY_TAP = {}


class _DepthMap(torch.autograd.Function):
    """depth = d_min / (sigmoid(logits) + d_min / d_max) as a differentiable node.  Saved: the logits and the depth."""

    @staticmethod
    def forward(ctx, logits, min_predict_depth, max_predict_depth):
        dev = logits.device
        if dev not in _IDENTITY_TAP:   # the head kernel over the one plane with an identity tap: 1.0 * logit + eight exact zeros
            _IDENTITY_TAP[dev] = torch.nn.functional.pad(torch.ones((1, 1, 1, 1), device=dev, dtype=torch.float32), (1, 1, 1, 1))
        lg = logits.detach().contiguous()
        depth = depth_head(lg, _IDENTITY_TAP[dev], min_predict_depth, max_predict_depth)
        ctx.save_for_backward(lg, depth)
        ctx.dmin = min_predict_depth
        return depth

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_depth):
        logits, depth = ctx.saved_tensors
        return depth_map_backward(logits, depth, grad_depth.contiguous(), ctx.dmin), None, None


@_on_tensor_device
def depth_map(logits: torch.Tensor, min_predict_depth: float, max_predict_depth: float) -> torch.Tensor:
    """KBNetModel.forward's mapping of the N x 1 x H x W logits (reference src/kbnet_model.py:181-184), differentiable (one node)."""
    _require(logits, "logits", 4)
    if logits.shape[1] != 1:
        raise KbnError(f"depth_map: logits must be N x 1 x H x W, got {tuple(logits.shape)}")
    return _DepthMap.apply(logits, float(min_predict_depth), float(max_predict_depth))


# ------------------------------------------------------------------ the optimizer
ADAM_TABLE_CAPACITY = _lib.KBN_ADAM_TABLE_CAPACITY   # tensors one launch of kbn_adam_step carries in its kernel arguments
ADAM_PASS_ELEMENTS = _lib.KBN_ADAM_PASS_ELEMENTS     # elements of one tensor the widest grid covers before its stride loop repeats


def _per_tensor(fn: str, value, name: str, count: int):
    """`value` as one host number per tensor: a number for all of them, or a sequence of `count` numbers."""
    if isinstance(value, torch.Tensor):
        raise KbnError(f"{fn}: {name} must be a host number (or one per tensor), not a tensor")
    if isinstance(value, (int, float)):
        return [float(value)] * count
    values = [float(v) for v in value]
    if len(values) != count:
        raise KbnError(f"{fn}: {name} has {len(values)} entries for {count} tensors")
    return values


_ADAM_RECORD = struct.Struct("@PPPPq7f4x")      # _lib.AdamTensor's layout: four pointers, numel, seven floats, padding to 72 bytes


def _adam_refuse(fn: str, i: int, p, g, m, v, device):
    """Raises for tensor i of an adam_step call, naming what is wrong with it (the call's checks found something)."""
    for t, name in ((p, "params"), (g, "grads"), (m, "exp_avgs"), (v, "exp_avg_sqs")):
        _require(t, f"{fn}: {name}[{i}]")
        if t.device != device:
            raise KbnError(f"{fn}: tensors live on different devices ({device} and {t.device})")
        if t.shape != p.shape:
            raise KbnError(f"{fn}: {name}[{i}] has shape {tuple(t.shape)}, params[{i}] {tuple(p.shape)}")
        if name != "grads" and not t.is_contiguous():
            raise KbnError(f"{fn}: {name}[{i}] must be dense (contiguous), got strides {t.stride()}: it is updated in place")
    raise KbnError(f"{fn}: tensor {i} was refused")


def adam_step(params: Sequence[torch.Tensor], grads: Sequence[torch.Tensor], exp_avgs: Sequence[torch.Tensor],
              exp_avg_sqs: Sequence[torch.Tensor], steps: Sequence[int], *, lr, betas, eps, weight_decay) -> None:
    """One Adam step over a list of tensors, in place (kbn_adam_step; torch's _single_tensor_adam with L2 weight decay, no amsgrad, no
    maximize, no decoupled decay).  Per element, in fp32:
        g' = g + weight_decay * p;  m += (1 - beta1) (g' - m);  v = beta2 v + (1 - beta2) g'^2;  p -= step_size m / (sqrt(v) / bc2_sqrt + eps)
    with step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t) computed here in fp64 from steps[i] = t >= 1, the number of THIS
    step for tensor i (tensors may be at different steps).  lr, eps and weight_decay are host numbers, one for all tensors or a
    sequence with one per tensor (param groups); betas a (beta1, beta2) pair or a sequence of pairs.

    params[i], exp_avgs[i], exp_avg_sqs[i] (all written) and grads[i] (read) are fp32 tensors of one shape on one HIP device.
    Parameters and states must be dense (contiguous; any storage offset -- a tensor that is not 16-byte aligned takes the kernel's
    scalar path): KbnError otherwise, since a copy would not be updated.  A gradient that is not dense is copied.  Empty tensors are
    skipped.  CPU tensors raise: there is no CPU fallback.  The work goes to torch's current stream of the tensors' device in
    ceil(non-empty tensors / ADAM_TABLE_CAPACITY) launches, with no host synchronisation, no allocation and no copy (but that of a
    gradient that is not dense); each launch is
    one ops.PROFILE record ("adam_step", nbytes = 28 B an element: p, g, m, v read, p, m, v written).

    THE VERSION CONTRACT.  The kernel writes the parameters through raw pointers, which torch's version counters do not see, and
    the packed-weight caches (modules._PackedBlob, GraphedForward's re-pack before a replay) follow nothing but a parameter's
    `_version`.  So this function bumps the version of every parameter it wrote (torch.autograd.graph.increment_version), and so
    must anything else that writes a parameter through a pointer: without the bump every later forward runs on stale weights,
    silently.  (The bump also makes autograd refuse a backward through a graph recorded before the step, as after torch's own
    in-place update.)  Not capturable into a HIP graph: the bias corrections are host numbers."""
    fn = "adam_step"
    lists = [list(params), list(grads), list(exp_avgs), list(exp_avg_sqs)]
    count = len(lists[0])
    steps = list(steps)
    if any(len(x) != count for x in lists) or len(steps) != count:
        raise KbnError(f"{fn}: params, grads, exp_avgs, exp_avg_sqs and steps must have one length, got "
                       f"{[len(x) for x in lists] + [len(steps)]}")
    if count == 0:
        return
    lrs, epss, wds = (_per_tensor(fn, v, k, count) for v, k in ((lr, "lr"), (eps, "eps"), (weight_decay, "weight_decay")))
    betas = list(betas)
    if len(betas) == 2 and all(isinstance(b, (int, float)) for b in betas):
        betas = [betas] * count
    if len(betas) != count:
        raise KbnError(f"{fn}: betas has {len(betas)} entries for {count} tensors")
    device = lists[0][0].device if isinstance(lists[0][0], torch.Tensor) else None
    f32 = torch.float32
    records = bytearray(_ADAM_RECORD.size * count)     # kbn_adam_tensor[count], packed in one call a tensor
    written, keep, used, scalars = [], [], 0, {}     # keep: the dense copies of gradients, alive until the launches are enqueued
    for i, (p, g, m, v) in enumerate(zip(*lists)):
        try:
            shape = p.shape
            ok = (p.is_cuda and p.dtype is f32 and g.dtype is f32 and m.dtype is f32 and v.dtype is f32 and g.shape == shape
                  and m.shape == shape and v.shape == shape and p.device == device and g.device == device and m.device == device
                  and v.device == device and p.is_contiguous() and m.is_contiguous() and v.is_contiguous())
        except AttributeError:
            ok = False
        if not ok:
            _adam_refuse(fn, i, p, g, m, v, device)
        numel = p.numel()
        if numel == 0:
            continue
        if not g.is_contiguous():
            g = g.contiguous()
            keep.append(g)
        t = int(steps[i])
        if t < 1 or t != steps[i]:
            raise KbnError(f"{fn}: steps[{i}] must be a whole number >= 1 (the number of this step), got {steps[i]!r}")
        beta1, beta2 = betas[i]
        key = (t, lrs[i], beta1, beta2)
        sc = scalars.get(key)
        if sc is None:
            beta1, beta2 = float(beta1), float(beta2)
            sc = scalars[key] = (1.0 - beta1, beta2, 1.0 - beta2, lrs[i] / (1.0 - beta1 ** t), (1.0 - beta2 ** t) ** 0.5)
        try:
            _ADAM_RECORD.pack_into(records, used * _ADAM_RECORD.size, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), numel,
                                   wds[i], sc[0], sc[1], sc[2], sc[3], sc[4], epss[i])
        except (struct.error, OverflowError):
            raise KbnError(f"{fn}: a scalar of tensor {i} is outside the fp32 range (lr {lrs[i]}, eps {epss[i]}, weight_decay {wds[i]}, "
                           f"step_size {sc[3]})") from None
        used += 1
        written.append(p)
    if not used:
        return
    lib = _lib.load()
    table = (_lib.AdamTensor * used).from_buffer(records)
    with torch.cuda.device(device):
        stream = _stream()
        if PROFILE is None:
            check(lib.kbn_adam_step(table, used, stream), "kbn_adam_step")
        else:    # one entry-point call a launch, so that each record times one launch
            for start in range(0, used, ADAM_TABLE_CAPACITY):
                n = min(ADAM_TABLE_CAPACITY, used - start)
                chunk = C.cast(C.byref(table, start * _ADAM_RECORD.size), C.POINTER(_lib.AdamTensor))
                elements = sum(table[j].numel for j in range(start, start + n))
                check(_launch("adam_step", 0.0, lambda: lib.kbn_adam_step(chunk, n, stream), nbytes=28.0 * elements), "kbn_adam_step")
    torch.autograd.graph.increment_version(written)


# ------------------------------------------------------------------ the data-parallel step's gradient pack
MULTI_COPY_TABLE_CAPACITY = _lib.KBN_MULTI_COPY_TABLE_CAPACITY   # tensors one launch of kbn_multi_tensor_scale_copy carries
MULTI_COPY_PASS_ELEMENTS = _lib.KBN_MULTI_COPY_PASS_ELEMENTS     # elements of one tensor the widest grid covers before its stride loop repeats
_COPY_RECORD = struct.Struct("@PPq")      # _lib.CopyTensor's layout: two pointers, numel


def multi_tensor_scale_copy(srcs: Sequence[torch.Tensor], dsts: Sequence[torch.Tensor], scale: float = 1.0) -> None:
    """dsts[i] = srcs[i] * float32(scale), element by element in memory order, over two lists of fp32 tensors
    (kbn_multi_tensor_scale_copy, csrc/multi_copy.hip): the pack and unpack pass of kb.dist.GradientAverager.  One fp32 multiply an
    element: the bits of srcs[i] * torch.tensor(scale, dtype=torch.float32), the source's own bits for scale == 1, and a NaN or Inf
    element stays in its own element.

    srcs[i] and dsts[i] are fp32 tensors on one HIP device with the same number of elements (shapes may differ: a parameter and its
    segment of a flat buffer).  Every destination must be dense (contiguous; any storage offset -- a pair that is not 16-byte aligned
    takes the kernel's scalar path): KbnError otherwise, since a copy would not be written.  A source that is not dense is copied and
    the copy kept alive until the launches are enqueued.  Empty tensors are skipped.  CPU tensors raise: there is no CPU fallback.
    The work goes to torch's current stream of the tensors' device in ceil(non-empty tensors / MULTI_COPY_TABLE_CAPACITY) launches,
    with no host synchronisation and no allocation; each launch is one ops.PROFILE record ("multi_tensor_scale_copy", nbytes = 8 B an
    element: read once, written once).

    A destination that is a parameter (an nn.Parameter, or any tensor that requires grad) is written through a raw pointer, so by
    adam_step's VERSION CONTRACT its version counter is bumped here."""
    fn = "multi_tensor_scale_copy"
    srcs, dsts = list(srcs), list(dsts)
    count = len(srcs)
    if len(dsts) != count:
        raise KbnError(f"{fn}: {count} sources and {len(dsts)} destinations")
    if count == 0:
        return
    try:
        scale = float(scale)
        struct.pack("f", scale)
    except (TypeError, ValueError, struct.error, OverflowError):
        raise KbnError(f"{fn}: scale must be a host number inside the fp32 range, got {scale!r}") from None
    device = srcs[0].device if isinstance(srcs[0], torch.Tensor) else None
    f32 = torch.float32
    records = bytearray(_COPY_RECORD.size * count)     # kbn_copy_tensor[count], packed in one call a tensor
    written, keep, used = [], [], 0     # keep: the dense copies of sources, alive until the launches are enqueued
    for i, (s, d) in enumerate(zip(srcs, dsts)):
        for t, name in ((s, "srcs"), (d, "dsts")):
            _require(t, f"{fn}: {name}[{i}]")
            if t.device != device:
                raise KbnError(f"{fn}: tensors live on different devices ({device} and {t.device})")
        numel = d.numel()
        if s.numel() != numel:
            raise KbnError(f"{fn}: srcs[{i}] has {s.numel()} elements, dsts[{i}] {numel}")
        if not d.is_contiguous():
            raise KbnError(f"{fn}: dsts[{i}] must be dense (contiguous), got strides {d.stride()}: it is written in place")
        if numel == 0:
            continue
        if not s.is_contiguous():
            s = s.detach().contiguous()
            keep.append(s)
        _COPY_RECORD.pack_into(records, used * _COPY_RECORD.size, s.data_ptr(), d.data_ptr(), numel)
        used += 1
        if d.requires_grad or isinstance(d, torch.nn.Parameter):
            written.append(d)
    if not used:
        return
    lib = _lib.load()
    table = (_lib.CopyTensor * used).from_buffer(records)
    with torch.cuda.device(device):
        stream = _stream()
        if PROFILE is None:
            check(lib.kbn_multi_tensor_scale_copy(table, used, scale, stream), "kbn_multi_tensor_scale_copy")
        else:    # one entry-point call a launch, so that each record times one launch
            for start in range(0, used, MULTI_COPY_TABLE_CAPACITY):
                n = min(MULTI_COPY_TABLE_CAPACITY, used - start)
                chunk = C.cast(C.byref(table, start * _COPY_RECORD.size), C.POINTER(_lib.CopyTensor))
                elements = sum(table[j].numel for j in range(start, start + n))
                check(_launch(fn, 0.0, lambda: lib.kbn_multi_tensor_scale_copy(chunk, n, scale, stream), nbytes=8.0 * elements),
                      "kbn_multi_tensor_scale_copy")
    if written:
        torch.autograd.graph.increment_version(written)


# ------------------------------------------------------------------ the augmentation
AUGMENT_FLIP_HORIZONTAL, AUGMENT_FLIP_VERTICAL, AUGMENT_REMOVE, AUGMENT_NOISE = 1, 2, 4, 8     # the bits of a frame's flags
_AUGMENT_RECORD = struct.Struct("@PP4q4i")      # _lib.AugmentTensor's layout: two pointers, four strides, channels, role, map index, reserved
_AUGMENT_RANGES = {(0.0, 255.0): _lib.KBN_AUGMENT_RANGE_0_255, (0.0, 1.0): _lib.KBN_AUGMENT_RANGE_0_1, (-1.0, 1.0): _lib.KBN_AUGMENT_RANGE_M1_1}
_AUGMENT_NOISES = {"none": _lib.KBN_AUGMENT_NOISE_NONE, "gaussian": _lib.KBN_AUGMENT_NOISE_GAUSSIAN, "uniform": _lib.KBN_AUGMENT_NOISE_UNIFORM}


def augment(images: Sequence[torch.Tensor], range_maps: Sequence[torch.Tensor], validity_maps: Sequence[torch.Tensor], flags: Sequence[int],
            densities: Optional[torch.Tensor], *, normalized_image_range=(0, 255), noise_type: str = "none", noise_spread: float = 0.0,
            seed: int = 0, call: int = 0, frame_base: int = 0):
    """The device part of the reference's Transforms.transform (src/transforms.py:61-183) over three lists of N x C x H x W fp32
    tensors (kbn_augment_forward, csrc/augment.hip).  Returns (images, range_maps, validity_maps) as lists of NEW dense tensors; no
    input is written (the reference flips in place).

    flags: one host integer a frame -- AUGMENT_FLIP_HORIZONTAL | AUGMENT_FLIP_VERTICAL (every tensor), AUGMENT_REMOVE | AUGMENT_NOISE
    (range maps only).  Images are normalised to `normalized_image_range` ([0, 1]: x / 255; [-1, 1]: 2 (x / 255) - 1; [0, 255]: as
    they came; anything else ValueError).  Removal: of the elements > 0 of frame b of a range map (count of them), the
    k = trunc(fp32(densities[b]) * fp32(count)) with the smallest (key, element index in the source frame) become 0.  Noise, after
    removal: out = (v + noise_spread * noise) * (v > 0), noise_type 'gaussian' or 'uniform' (anything else ValueError once a frame
    has the bit).  Every random word is Philox4x32-10 of (seed; element, frame, call, purpose | map index << 8): the same
    arguments give the same bits, and tests/transforms_oracle.py computes them on the host.

    frame_base: the tensors are frames [frame_base, frame_base + N) of a larger batch (a rank's shard of a data-parallel step), and
    the counter's frame word is frame_base + the frame's index here (kbn_augment_forward_at).  With the slices of the larger batch's
    flags and densities the outputs are, bit for bit, the slices of what one call over the larger batch returns.  0: the frames
    are the batch.  KbnError when frame_base is negative or frame_base + N exceeds 2^32 - 1.

    densities: an fp32 DEVICE tensor of N, needed when a frame has AUGMENT_REMOVE and there is a range map, else None.  It is read
    on the device: the count and k never reach the host.  Inputs may be any views (a view that is not 16-byte aligned or whose rows
    are not dense takes the kernel's scalar path); CPU tensors raise, there is no CPU fallback.  The call enqueues at most two
    launches on torch's current stream of the tensors' device -- selection (ops.PROFILE record "augment_select") and apply
    ("augment_apply", nbytes = 8 B an element) -- and, besides the outputs and (with AUGMENT_REMOVE) a workspace of the size of
    two range maps (the candidate lists of the selection), allocates nothing, copies nothing from or to the host, and never waits
    for the device: the flags travel in the kernel arguments."""
    fn = "augment"
    lists = [list(images), list(range_maps), list(validity_maps)]
    rng = tuple(float(v) for v in normalized_image_range)
    if rng not in _AUGMENT_RANGES:
        raise ValueError("Unsupported normalization range: {}".format(list(normalized_image_range)))
    names = ("images", "range_maps", "validity_maps")
    first = None
    for lst, name in zip(lists, names):     # what is wrong with a tensor is named before where it lives: a CPU box can test the refusals
        for i, t in enumerate(lst):
            if not isinstance(t, torch.Tensor):
                raise KbnError(f"{fn}: {name}[{i}]: expected a tensor, got {type(t).__name__}")
            if t.dtype != torch.float32:
                raise KbnError(f"{fn}: {name}[{i}]: expected float32, got {t.dtype}")
            if t.dim() != 4:
                raise ValueError("Unsupported number of dimensions: {}".format(t.dim()))
            first = t if first is None else first
            if t.shape[0] != first.shape[0] or t.shape[2:] != first.shape[2:] or t.shape[1] < 1:
                raise KbnError(f"{fn}: {name}[{i}] has shape {tuple(t.shape)}, expected ({first.shape[0]}, c >= 1, {first.shape[2]}, "
                               f"{first.shape[3]}) as the first tensor's")
    if first is None:
        return [], [], []
    n, _, h, w = first.shape
    flags = [int(f) for f in flags]
    if len(flags) != n or any(f < 0 or f > 15 for f in flags):
        raise KbnError(f"{fn}: flags must hold one value in 0..15 for each of the {n} frames, got {flags}")
    frame_base = int(frame_base)
    if frame_base < 0 or frame_base + n > 0xFFFFFFFF:
        raise KbnError(f"{fn}: frame_base {frame_base} with {n} frames: the frame word of the random counter is 32 bits")
    any_remove = any(f & AUGMENT_REMOVE for f in flags) and bool(lists[1])
    any_noise = any(f & AUGMENT_NOISE for f in flags) and bool(lists[1])
    if noise_type not in ("gaussian", "uniform"):
        if any_noise:
            raise ValueError("Unsupported noise type: {}".format(noise_type))
        noise_type = "none"     # never applied in this call
    for lst, name in zip(lists, names):
        for i, t in enumerate(lst):
            _require(t, f"{fn}: {name}[{i}]")
            if t.device != first.device:
                raise KbnError(f"{fn}: tensors live on different devices ({first.device} and {t.device})")
    device = first.device
    if any_remove:
        _require(densities, f"{fn}: densities")
        if densities.device != device or tuple(densities.shape) != (n,) or not densities.is_contiguous():
            raise KbnError(f"{fn}: densities must be a dense tensor of {n} numbers on {device}, got {tuple(densities.shape)} on {densities.device}")
    count = sum(len(lst) for lst in lists)
    records = bytearray(_AUGMENT_RECORD.size * count)
    outs = [[], [], []]
    used = elements = 0
    for role, lst in enumerate(lists):
        for i, t in enumerate(lst):
            out = torch.empty(t.shape, device=device, dtype=torch.float32)
            outs[role].append(out)
            _AUGMENT_RECORD.pack_into(records, used * _AUGMENT_RECORD.size, t.data_ptr(), out.data_ptr(), *t.stride(), t.shape[1], role,
                                      i if role == _lib.KBN_AUGMENT_ROLE_RANGE else 0, 0)
            used += 1
            elements += t.numel()
    if n * h * w == 0:
        return tuple(outs)
    lib = _lib.load()
    table = (_lib.AugmentTensor * used).from_buffer(records)
    workspace = None
    if any_remove:      # a 16-byte record and a list of 8 bytes an element for every frame of every range map
        need = lib.kbn_augment_workspace_bytes(table, used, n, h, w)
        if need == 0 and lists[_lib.KBN_AUGMENT_ROLE_RANGE]:      # a refusal; without range maps there is nothing to select from
            raise KbnError(f"{fn}: no workspace for {n} frames of {h} x {w} range maps")
        workspace = torch.empty(need // 8, device=device, dtype=torch.int64)
    with torch.cuda.device(device):
        stream = _stream()

        def run(stages):
            return lib.kbn_augment_forward_at(table, used, bytes(flags), n, h, w, densities.data_ptr() if any_remove else None,
                                              workspace.data_ptr() if any_remove else None, workspace.numel() * 8 if any_remove else 0,
                                              _AUGMENT_RANGES[rng], _AUGMENT_NOISES[noise_type], float(noise_spread),
                                              int(seed) & 0xFFFFFFFFFFFFFFFF, int(call) & 0xFFFFFFFF, frame_base, stages, stream)
        if PROFILE is None:
            check(run(_lib.KBN_AUGMENT_STAGE_SELECT | _lib.KBN_AUGMENT_STAGE_APPLY), "kbn_augment_forward_at")
        else:    # one entry-point call a stage, so that each record times one stage
            if any_remove:
                check(_launch("augment_select", 0.0, lambda: run(_lib.KBN_AUGMENT_STAGE_SELECT)), "kbn_augment_forward_at")
            check(_launch("augment_apply", 0.0, lambda: run(_lib.KBN_AUGMENT_STAGE_APPLY), nbytes=8.0 * elements), "kbn_augment_forward_at")
    return tuple(outs)


# ------------------------------------------------------------------ the training loop's image summaries
_SUMMARY_SOURCES = {_lib.KBN_SUMMARY_CELL_ZERO: 0, _lib.KBN_SUMMARY_CELL_COPY: 1, _lib.KBN_SUMMARY_CELL_DEPTH: 1, _lib.KBN_SUMMARY_CELL_PHOTO_ERR: 2,
                    _lib.KBN_SUMMARY_CELL_REL_ERR: 3}
SUMMARY_COLORMAPS = {"viridis": _lib.KBN_SUMMARY_COLORMAP_VIRIDIS, "inferno": _lib.KBN_SUMMARY_COLORMAP_INFERNO}


def _summary_n_display(fn: str, n_display) -> int:
    if isinstance(n_display, bool) or not isinstance(n_display, int) or n_display < 1:
        raise KbnError(f"{fn}: n_display must be an integer of at least 1 (the panel's columns), got {n_display!r}")
    return n_display


def _summary_inputs(fn: str, given, channels):
    """The argument checks of the two panels: `given` name -> tensor or None, `channels` name -> the channel count the reference's
    torch.cat needs.  What is wrong with a tensor is named before where it lives (a CPU box can test the refusals) -> (N, H, W)."""
    first = first_name = None
    for name, t in given.items():
        if t is None:
            continue
        if not isinstance(t, torch.Tensor):
            raise KbnError(f"{fn}: {name} must be a tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise KbnError(f"{fn}: {name}: expected float32, got {t.dtype}")
        if t.dim() != 4:
            raise KbnError(f"{fn}: {name}: expected N x C x H x W, got {tuple(t.shape)}")
        if t.shape[1] != channels[name]:
            raise KbnError(f"{fn}: {name} has {t.shape[1]} channels, expected {channels[name]} (shape {tuple(t.shape)})")
        if first is None:
            first, first_name = t, name
        elif t.shape[0] != first.shape[0] or t.shape[2:] != first.shape[2:]:
            raise KbnError(f"{fn}: {name} has shape {tuple(t.shape)}, but {first_name} has {tuple(first.shape)}: N, H and W must agree")
    for name, t in given.items():
        if t is not None:
            _require(t, f"{fn}: {name}")
            if t.device != first.device:
                raise KbnError(f"{fn}: tensors live on different devices ({first.device} and {t.device})")
    return (first.shape[0], first.shape[2], first.shape[3]) if first is not None else (0, 0, 0)


def summary_panel_shape(n_rows: int, frames: int, height: int, width: int):
    """(3, Hg, Wg) of a panel of `frames` tiles of n_rows x 2 cells: make_grid's padding of 2 around and between the tiles of several
    frames, the tile itself for one frame."""
    pad = 2 if frames > 1 else 0
    return 3, n_rows * height + 2 * pad, frames * (2 * width + pad) + pad


def _summary_panel(fn: str, rows, n: int, h: int, w: int, n_display: int, max_predict_depth: float, out: Optional[torch.Tensor]):
    """One kbn_summary_panel_forward launch.  rows: [(left kind, [tensors]), (right kind, [tensors])] per row; None for fewer than
    two rows (the reference logs no image then)."""
    if len(rows) < 2:
        return None
    if n < 1 or h < 1 or w < 1:
        raise KbnError(f"{fn}: nothing to show in tensors of {n} x . x {h} x {w}")
    frames = min(n_display, n)
    device = rows[0][0][1][0].device
    records = (_lib.SummaryRow * len(rows))()
    for record, (left, right) in zip(records, rows):
        for cell, (kind, tensors) in ((record.left, left), (record.right, right)):
            assert len(tensors) == _SUMMARY_SOURCES[kind]
            cell.kind = kind
            for src, t in zip(cell.src, tensors):
                src.data = t.data_ptr()
                src.stride_n, src.stride_c, src.stride_h, src.stride_w = t.stride()
                src.channels = t.shape[1]
    panel = _out_tensor(out, summary_panel_shape(len(rows), frames, h, w), device, f"{fn}: out")
    if panel.device != device:
        raise KbnError(f"{fn}: out lives on {panel.device}, the inputs on {device}")
    lib = _lib.load()
    with torch.cuda.device(device):
        stream = _stream()
        cells = 2.0 * len(rows) * frames * h * w
        check(_launch(fn, 0.0, lambda: lib.kbn_summary_panel_forward(records, len(rows), frames, h, w, float(max_predict_depth), panel.data_ptr(),
                                                                       stream), nbytes=4.0 * 3 * panel.shape[1] * panel.shape[2] + 4.0 * 1.5 * cells),
              "kbn_summary_panel_forward")
    return panel


def summary_image_panel(image0, image01=None, image02=None, n_display: int = 4, out: Optional[torch.Tensor] = None):
    """The image panel of the reference's log_summary (src/kbnet_model.py:474-531, 636-642) as one 3 x Hg x Wg fp32 device tensor,
    written by ONE launch (kbn_summary_panel_forward, csrc/summary.hip): what
        torchvision.utils.make_grid(torch.cat(rows, dim=2), nrow=n_display)
    returns for the rows  image0 | 0,  image01 | inferno(mean_c |image0 - image01| / 0.10),  image02 | the same for image02  of the
    first min(n_display, N) frames.  A row exists where the reference's `if` holds (image01 and image02 need image0); with fewer than
    two rows the reference logs no image and this returns None.  The inputs (N x 3 x H x W fp32, any views) are never written and
    only their first min(n_display, N) frames are read.  `out`: write into this dense tensor of the panel's shape
    (summary_panel_shape) instead of a new one.  CPU tensors raise: there is no CPU fallback."""
    fn = "summary_image_panel"
    n_display = _summary_n_display(fn, n_display)
    n, h, w = _summary_inputs(fn, {"image0": image0, "image01": image01, "image02": image02}, {"image0": 3, "image01": 3, "image02": 3})
    rows = []
    if image0 is not None:
        rows.append(((_lib.KBN_SUMMARY_CELL_COPY, [image0]), (_lib.KBN_SUMMARY_CELL_ZERO, [])))
        for warped in (image01, image02):
            if warped is not None:
                rows.append(((_lib.KBN_SUMMARY_CELL_COPY, [warped]), (_lib.KBN_SUMMARY_CELL_PHOTO_ERR, [image0, warped])))
    return _summary_panel(fn, rows, n, h, w, n_display, 1.0, out)


def summary_depth_panel(output_depth0, max_predict_depth: float, image0=None, sparse_depth0=None, validity_map0=None, ground_truth0=None,
                        n_display: int = 4, out: Optional[torch.Tensor] = None):
    """The depth panel of the reference's log_summary (src/kbnet_model.py:474-487, 533-617, 644-650), one launch as
    summary_image_panel.  Rows, each where the reference's `if` holds:
        image0 | 0                                                                 image0 given
        viridis(output / max_predict_depth) | 0                                    output_depth0 given
        viridis(sparse / max) | inferno(rel(output, sparse, validity) / 0.05)      output, sparse_depth0 and validity_map0 given
        viridis(gt[:, 0] / max) | inferno(rel(output, gt[:, 0], gt[:, 1]) / 0.05)  output and ground_truth0 (N x 2 x H x W) given
    with rel(o, r, v) = (|o - r| + 1e-8) / (r + 1e-8) where v == 1, else v.  None with fewer than two rows.  The ground truth's two
    planes are read in place (no copy)."""
    fn = "summary_depth_panel"
    n_display = _summary_n_display(fn, n_display)
    given = {"image0": image0, "output_depth0": output_depth0, "sparse_depth0": sparse_depth0, "validity_map0": validity_map0,
             "ground_truth0": ground_truth0}
    n, h, w = _summary_inputs(fn, given, {"image0": 3, "output_depth0": 1, "sparse_depth0": 1, "validity_map0": 1, "ground_truth0": 2})
    zero = (_lib.KBN_SUMMARY_CELL_ZERO, [])
    rows = []
    if image0 is not None:
        rows.append(((_lib.KBN_SUMMARY_CELL_COPY, [image0]), zero))
    if output_depth0 is not None:
        rows.append(((_lib.KBN_SUMMARY_CELL_DEPTH, [output_depth0]), zero))
        if sparse_depth0 is not None and validity_map0 is not None:
            rows.append(((_lib.KBN_SUMMARY_CELL_DEPTH, [sparse_depth0]), (_lib.KBN_SUMMARY_CELL_REL_ERR, [output_depth0, sparse_depth0, validity_map0])))
        if ground_truth0 is not None:
            depth, validity = ground_truth0[:, 0:1], ground_truth0[:, 1:2]
            rows.append(((_lib.KBN_SUMMARY_CELL_DEPTH, [depth]), (_lib.KBN_SUMMARY_CELL_REL_ERR, [output_depth0, depth, validity])))
    return _summary_panel(fn, rows, n, h, w, n_display, float(max_predict_depth), out)


@_on_tensor_device
def summary_colorize(x: torch.Tensor, colormap: str) -> torch.Tensor:
    """matplotlib's Colormap.__call__ on an N x 1 x H x W fp32 device tensor -> N x 3 x H x W (kbn_summary_colorize_forward): entry
    (int)(x * 256), entry 0 below 0, entry 255 from 1 on, (0, 0, 0) for NaN.  'viridis' and 'inferno' only."""
    if colormap not in SUMMARY_COLORMAPS:
        raise ValueError(f"summary_colorize: colormap {colormap!r} is not built in (have: {', '.join(SUMMARY_COLORMAPS)})")
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != 1:
        raise KbnError(f"summary_colorize: expected an N x 1 x H x W tensor, got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}")
    _require(x, "summary_colorize: T", 4)
    n, _, h, w = x.shape
    out = torch.empty((n, 3, h, w), device=x.device, dtype=torch.float32)
    for first in range(0, n if h * w else 0, 65535):    # a launch's grid carries 65535 frames
        part = x[first:first + 65535]
        check(_lib.load().kbn_summary_colorize_forward(part.data_ptr(), part.stride(0), part.stride(2), part.stride(3), part.shape[0], h, w,
                                                       SUMMARY_COLORMAPS[colormap], out[first:].data_ptr(), _stream()), "kbn_summary_colorize_forward")
    return out


# ------------------------------------------------------------------------------------------------ TensorBoard's histogram
HISTOGRAM_BINS = _lib.KBN_HISTOGRAM_BINS
_HISTOGRAM_EDGES = None
_HISTOGRAM_TABLES = {}    # device index -> (the positive edges as a float64 device tensor, the workspace)


def histogram_edges():
    """The 1549 bucket edges of SummaryWriter.add_histogram(bins='tensorflow') as a tuple of Python floats: 1e-12 multiplied by 1.1
    again and again while below 1e20 (float64, repeated multiplication -- not a power), mirrored negative, 0 between."""
    global _HISTOGRAM_EDGES
    if _HISTOGRAM_EDGES is None:
        positive = []
        v = 1e-12
        while v < 1e20:
            positive.append(v)
            v *= 1.1
        _HISTOGRAM_EDGES = tuple([-e for e in reversed(positive)] + [0.0] + positive)
        assert len(positive) == _lib.KBN_HISTOGRAM_POSITIVE_EDGES and len(_HISTOGRAM_EDGES) == HISTOGRAM_BINS + 1
    return _HISTOGRAM_EDGES


@_on_tensor_device
def histogram_tensorflow(values: torch.Tensor):
    """TensorBoard's default histogram of an fp32 device tensor (kbn_histogram_forward, csrc/histogram.hip) -> (counts, stats):
    counts HISTOGRAM_BINS int32 = np.histogram(values.astype(float), bins=histogram_edges())[0], stats 4 float64 = min, max (NaN
    propagates), sum, sum of squares over all values.  Both are views of ONE device buffer of 6224 bytes (`counts._base`); nothing is
    copied to the host and nothing waits for the device.  Any view is accepted: a view that is not contiguous is copied to a dense
    tensor first, a contiguous one is read in place with 16-byte loads from its first 16-byte boundary on.  An empty tensor raises
    ValueError('The input has no element.') as TensorBoard does, a CPU tensor KbnError (no CPU fallback).  Two calls give the same
    bits.  The calls of one device share the edge table and a 32 KB workspace: issue them on one stream, torch's current one."""
    fn = "histogram_tensorflow"
    _require(values, f"{fn}: values")
    n = values.numel()
    if n == 0:
        raise ValueError("The input has no element.")
    x = values.detach().contiguous()
    index = x.device.index
    if index not in _HISTOGRAM_TABLES:
        positive = histogram_edges()[_lib.KBN_HISTOGRAM_POSITIVE_EDGES + 1:]
        _HISTOGRAM_TABLES[index] = (torch.tensor(positive, dtype=torch.float64).to(x.device),
                                    torch.empty(_lib.KBN_HISTOGRAM_WORKSPACE_BYTES // 8, dtype=torch.float64, device=x.device))
    table, workspace = _HISTOGRAM_TABLES[index]
    out = torch.empty(HISTOGRAM_BINS + 8, dtype=torch.int32, device=x.device)
    counts, stats = out[:HISTOGRAM_BINS], out[HISTOGRAM_BINS:].view(torch.float64)
    lib = _lib.load()
    check(_launch("histogram", 0.0,
                  lambda: lib.kbn_histogram_forward(x.data_ptr(), n, table.data_ptr(), counts.data_ptr(), stats.data_ptr(), workspace.data_ptr(),
                                                    workspace.numel() * 8, _stream()),
                  nbytes=4.0 * n), "kbn_histogram_forward")
    return counts, stats
