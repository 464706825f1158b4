"""Frame sharding across GPUs: one process per GPU, RCCL over xGMI.

Frames are independent (no normalisation layers, per-frame intrinsics), so the path
shards on the batch dimension with NO data-path collective; the only exchange is one
all-gather of the N/world x 1 x H x W depth maps per step (1.7 MB per KITTI frame).
This replaces the reference's three `torch.nn.DataParallel` wrappers
(reference src/kbnet_model.py:408-415), which scatter/replicate/gather per module
and per forward inside a single process.

Training takes the same form (`GradientAverager`): the weights resident on every rank, each rank differentiating its own frames,
and one all-reduce of all gradients, packed into one flat buffer, per step.  The pose networks' BatchNorm layers in 'batch' mode are
the one place where frames are not independent: `BatchNormGroup` gathers their statistics over the ranks.

Works with backend "nccl" (= RCCL on ROCm) on GPUs and "gloo" on CPU (tests).
"""

from __future__ import annotations

import os
from typing import Callable, Optional, Sequence, Tuple

import torch
import torch.distributed as dist

from ._lib import KbnError


def env_world() -> Tuple[int, int, int]:
    """(rank, local_rank, world_size) from the torchrun environment (1 process => 0, 0, 1)."""
    return (int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0")),
            int(os.environ.get("WORLD_SIZE", "1")))


def init(backend: Optional[str] = None) -> Tuple[int, int, int]:
    rank, local_rank, world = env_world()
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        if backend is None:
            backend = "nccl" if torch.cuda.is_available() else "gloo"
        if backend == "nccl":
            torch.cuda.set_device(local_rank)
        dist.init_process_group(backend=backend, rank=rank, world_size=world)
    return rank, local_rank, world


def shard_bounds(n_frames: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous, balanced partition of frame indices; the first n % world ranks get one extra."""
    q, r = divmod(n_frames, world)
    start = rank * q + min(rank, r)
    return start, start + q + (1 if rank < r else 0)


def shard_frames(tensors: Sequence[torch.Tensor], rank: int, world: int):
    lo, hi = shard_bounds(tensors[0].shape[0], rank, world)
    return [t[lo:hi] for t in tensors]


class ShardedRunner:
    """Runs `forward_fn` on this rank's frames and all-gathers the outputs.

    forward_fn(image, sparse_depth, validity, intrinsics) -> N_local x 1 x H x W.
    Gather buffers are allocated once per output shape and re-used; ranks may hold different
    frame counts (ragged tail) -- then the gather goes through padded slots.

    Lifetime of returned tensors: they are views of the runner's own buffers.  `step()` / `step_mixed()`
    results are overwritten by the next call with the same output shape; `step_pipelined()` results by the
    next-but-one call when a collective runs (they live in the runner's two gather buffers) -- and by the NEXT call
    without one (a single rank: the result is then the forward's own output tensor, which with rotating graph outputs
    is the tensor the next replay writes).  Clone what must live longer."""

    def __init__(self, forward_fn: Callable, rank: int, world: int, gather_single: bool = False):
        """`gather_single`: run the collectives even with one rank (a one-rank RCCL group is legal): lets a single-GPU
        box exercise the whole RCCL path -- stream ordering against graph replays included -- in tests."""
        self.forward_fn = forward_fn
        self.rank, self.world = rank, world
        self.collective = world > 1 or (gather_single and dist.is_initialized())
        self._bufs = {}        # (per, shape[1:], device) -> gather buffer
        self._ring = None      # pipelined mode: [(staging, gathered, work)] x 2
        self._step = 0

    # ---- fixed-shape stream, gather of step i overlapped with the forward of step i+1 -------------------
    def step_pipelined(self, local_inputs):
        """Forward of this step + an ASYNCHRONOUS all-gather of its outputs, overlapped with the
        next step's forward (RCCL runs on its own stream; xGMI traffic hides behind the MFMAs).
        Every rank must hold the same number of frames (checked once).  Returns the gathered
        N_total x 1 x H x W tensor of the PREVIOUS step (None on the first call); `drain()` returns the last."""
        # A forward with `rotating_outputs` >= 2 (GraphedForward(outputs=2): the captured graph exists once per output tensor and
        # calls alternate between them) hands back a tensor nothing overwrites before the next-but-one call: the all-gather
        # reads it in place and the ring's staging copy (55 MB per rank and step at 32 KITTI frames) is skipped.  The gather
        # that read the tensor this call is about to overwrite was issued two steps ago; it is awaited here, BEFORE the forward.
        rotating = int(getattr(self.forward_fn, "rotating_outputs", 0) or 0) >= 2
        if rotating and self._ring is not None:
            # by tensor identity, not by step parity: somebody else may have called the forward in between (bench.py's gather check
            # does), which shifts the rotation against this runner's step count
            nxt = self.forward_fn.next_output() if hasattr(self.forward_fn, "next_output") else None
            for stale in self._ring:
                if stale[2] is not None and (nxt is None or stale[0] is None or stale[0].data_ptr() == nxt.data_ptr()):
                    stale[2].wait()
                    stale[2] = None
        out = self.forward_fn(*local_inputs)
        if self._ring is None:
            if self.collective:   # a ragged shard would hang or fail inside the collective: check once
                n = torch.tensor([out.shape[0], -out.shape[0]], device=out.device, dtype=torch.int64)
                dist.all_reduce(n, op=dist.ReduceOp.MAX)
                if int(n[0]) != -int(n[1]):
                    raise ValueError(f"step_pipelined needs equal shards on every rank (min {-int(n[1])}, "
                                     f"max {int(n[0])} frames); use step() / step_mixed() for ragged batches")
            gathered = lambda: (torch.empty((self.world * out.shape[0],) + tuple(out.shape[1:]),
                                            device=out.device, dtype=out.dtype) if self.collective else None)
            self._ring = [[None if rotating else torch.empty_like(out), gathered(), None] for _ in range(2)]
        slot = self._ring[self._step & 1]
        if slot[2] is not None:
            slot[2].wait()                      # the gather that used this slot two steps ago
        if rotating:
            slot[0] = out                       # the forward's own (rotating) output tensor: no copy
        else:
            slot[0].copy_(out)                  # `out` may be a graph's ONE static buffer: detach it
        if self.collective:
            slot[2] = dist.all_gather_into_tensor(slot[1], slot[0], async_op=True)
        prev = self._ring[(self._step & 1) ^ 1]
        self._step += 1
        if self._step == 1:
            return None
        return self._finish(prev)

    def _finish(self, slot):
        if not self.collective:
            return slot[0]
        if slot[2] is not None:
            slot[2].wait()                      # orders the consumer after the gather
        return slot[1]

    def drain(self):
        if self._ring is None or self._step == 0:
            return None
        return self._finish(self._ring[(self._step - 1) & 1])

    # ---- one batch, any split ----------------------------------------------------------------------------
    def _slots(self, out, per, bucket=0):
        # `bucket`: several gathers of one step_mixed call are in flight at once, so two buckets of the same frame
        # shape and slot size must not share a buffer (the second collective would overwrite the first)
        key = (per, tuple(out.shape[1:]), out.device, out.dtype, bucket)
        buf = self._bufs.get(key)
        if buf is None:
            buf = self._bufs[key] = torch.empty((self.world * per,) + tuple(out.shape[1:]), device=out.device,
                                                dtype=out.dtype)
        return buf

    def _gather_start(self, out, n_total, bucket=0):
        """-> (buffer, work, per): `out` (N_local frames, N_local possibly 0 < per) into padded slots."""
        per = -(-n_total // self.world)          # slot size (max frames on any rank)
        buf = self._slots(out, per, bucket)
        if out.shape[0] == per:
            src = out.contiguous()
        else:
            src = torch.zeros((per,) + tuple(out.shape[1:]), device=out.device, dtype=out.dtype)
            src[:out.shape[0]] = out
        return buf, dist.all_gather_into_tensor(buf, src, async_op=True), per

    def _gather_finish(self, buf, work, per, n_total):
        work.wait()
        if n_total == self.world * per:
            return buf
        parts = []
        for r in range(self.world):
            lo, hi = shard_bounds(n_total, r, self.world)
            parts.append(buf[r * per:r * per + (hi - lo)])
        return torch.cat(parts, dim=0)

    def step(self, local_inputs, n_total: Optional[int] = None, gather: bool = True):
        out = self.forward_fn(*local_inputs)
        if not self.collective or not gather:
            return out
        n_total = n_total if n_total is not None else out.shape[0] * self.world
        lo, hi = shard_bounds(n_total, self.rank, self.world)
        if out.shape[0] != hi - lo:
            raise ValueError(f"rank {self.rank} holds {out.shape[0]} frames, shard_bounds gives {hi - lo} of {n_total}")
        return self._gather_finish(*self._gather_start(out, n_total), n_total)

    # ---- mixed-shape stream (BASELINE config 5) ----------------------------------------------------------
    def step_mixed(self, buckets: Sequence[Tuple[Callable, Optional[Sequence[torch.Tensor]], int, Tuple[int, ...]]]):
        """One step of a stream that mixes frame shapes (VOID 480x640 / NYUv2 416x576 / KITTI 352x1216, each
        with its own weights and per-frame intrinsics).  `buckets`: one entry per shape, in the SAME order on
        every rank: (forward_fn, this rank's inputs of that shape or None, n_total frames of that shape over all
        ranks, output shape per frame e.g. (1, H, W)).  Frames of a bucket are split with `shard_bounds`, so a
        rank may hold fewer frames than its neighbours or none (it then contributes an empty, padded slot).
        One all-gather per shape bucket into that bucket's own buffer; the gather of bucket i is in flight
        while bucket i+1 computes.  Returns the list of N_total x ... tensors, bucket order."""
        pending = []
        for bucket, (forward_fn, inputs, n_total, frame_shape) in enumerate(buckets):
            lo, hi = shard_bounds(n_total, self.rank, self.world)
            out = None
            if inputs is not None and hi > lo:
                out = forward_fn(*inputs)
                if out.shape[0] != hi - lo or tuple(out.shape[1:]) != tuple(frame_shape):
                    raise ValueError(f"bucket {tuple(frame_shape)}: forward returned {tuple(out.shape)}, this rank's "
                                     f"share is {hi - lo} frames")
            elif hi > lo:
                raise ValueError(f"rank {self.rank} owns {hi - lo} frames of bucket {tuple(frame_shape)} but got no inputs")
            if not self.collective:
                pending.append((out, None, 0, n_total))
                continue
            if out is None:   # nothing of this shape here: still take part in the collective
                ref = inputs[0] if inputs is not None else None
                dev = ref.device if ref is not None else self._default_device()
                out = torch.empty((0,) + tuple(frame_shape), device=dev, dtype=torch.float32)
            pending.append(self._gather_start(out, n_total, bucket) + (n_total,))
        results = []
        for buf, work, per, n_total in pending:
            results.append(buf if work is None else self._gather_finish(buf, work, per, n_total))
        return results

    def _default_device(self):
        if dist.is_initialized() and dist.get_backend() == "nccl":
            return torch.device("cuda", torch.cuda.current_device())
        return torch.device("cpu")


# ------------------------------------------------------------------------------------ data-parallel training
def bucket_layout(numels: Sequence[int]) -> Tuple[list, int]:
    """(offsets, total) of GradientAverager's flat buffer, in elements: tensor i owns [offsets[i], offsets[i] + numels[i]), every
    offset and the total a multiple of four, so that each segment of an fp32 buffer starts 16-byte aligned (the vector paths of
    ops.multi_tensor_scale_copy and ops.adam_step).  The padding of at most three elements after a segment belongs to nobody.  An
    empty tensor gets the next tensor's offset and no room."""
    offsets, at = [], 0
    for n in numels:
        n = int(n)
        if n < 0:
            raise KbnError(f"bucket_layout: a tensor of {n} elements")
        offsets.append(at)
        at += (n + 3) & ~3
    return offsets, at


class GradientAverager:
    """The data-parallel training step: one process per GPU, the weights resident on each, ONE all-reduce a step (in place of the
    reference's torch.nn.DataParallel, src/kbnet_model.py:408-415, which replicates the weights and gathers the gradients inside
    one process per forward).

        averager = kb.dist.GradientAverager(depth_model.parameters() + pose_model.parameters(), rank, world)
        averager.broadcast_parameters()
        for b, batch in enumerate(loader):                         # TrainingFrameLoader(..., rank=rank, world=world)
            ...                                                    # forward and compute_loss on this rank's frames
            optimizer.zero_grad(); loss.backward()
            averager.average(n_local, loader.global_batch_size(b)); optimizer.step()

    `parameters`: the list the optimizer steps -- dense fp32 tensors on one HIP device (KbnError otherwise) -- or (name, tensor)
    pairs, whose names the error messages then use.  Construction makes one flat fp32 buffer laid out by `bucket_layout` and zeroes
    it once; the padding between segments is never written, so it stays zero through every SUM.

    average(n_local, n_global), between loss.backward() and optimizer.step(): every .grad is packed into its segment scaled by
    float32(n_local / n_global) (ops.multi_tensor_scale_copy: ceil(tensors / its table capacity) launches), the buffer goes through
    one all_reduce(SUM) (not AVG: gloo has none), and each packed parameter's .grad is rebound to its segment's view, so
    optimizer.step() reads the reduced gradients where they are: there is no unpack pass.  The call enqueues and returns, without a
    host synchronisation but the first call's agreement check below (and what the backend's all_reduce itself does).  A .grad that
    already is its view (optimizer.zero_grad(set_to_none=False)) is scaled in place.

    The weights are n_local / n_global, not 1 / world: TrainingFrameLoader keeps the ragged last batch, and with per-rank losses
    that are means over the rank's n_local frames the weighted sum is the gradient of the mean over the n_global frames -- what one
    process computes on the whole batch.  A rank with n_local == 0 (its shard of a short last batch is empty) runs no forward and no
    backward: it zero-fills the buffer with one memset, takes part in the collective and binds the same views, so every rank applies
    the same Adam step and the replicas stay bit-identical.

    Parameters without a gradient (calibrated_backprojection4.conv_image, the `projection` of identity-skip ResNet blocks) keep
    .grad None on every rank, so Adam skips them as in one process, and their segments stay zero.  Which parameters have gradients
    follows from the architecture alone.  The FIRST average call agrees the set across ranks with one small blocking all-reduce (MAX)
    of the mask and of its complement; a rank with n_local == 0 contributes to neither.  If two ranks disagree, EVERY rank raises
    KbnError naming the first such parameter, after the collective: none is left waiting in the next one.  Later calls compare the
    local set with the agreed one on the host before packing; a mismatch there raises on THAT RANK ONLY (the others then wait in
    their all-reduce until the backend's timeout) -- it can only come from ranks that built different models.

    broadcast_parameters(src=0) makes every rank's parameters rank `src`'s: packed into the buffer (scale 1), one broadcast, copied
    back by the same op, which bumps the parameters' version counters (the packed-weight caches follow them); the buffer is zeroed
    again afterwards.  The modules' floating-point BUFFERS -- BatchNorm running statistics -- are not broadcast: they stay per rank,
    and rank 0's are the ones a checkpoint holds, which is what the reference's DataParallel does (replica statistics are dropped,
    device 0's module keeps its own).  With per-rank statistics in 'batch' mode the reduced gradient of a pose network is NOT the
    whole batch's: `BatchNormGroup` below, through the pose models' sync_batch_norm, is what makes it so.

    With world == 1 and no `reduce_single` no collective runs (as in ShardedRunner) and broadcast_parameters does nothing;
    `reduce_single=True` runs the collectives on a one-rank group, for tests.  Any initialised backend that moves device tensors
    works: "nccl" (RCCL), and "gloo" with ranks that share a device.  One buffer, one all-reduce: there is no bucket size."""

    def __init__(self, parameters, rank: int, world: int, reduce_single: bool = False):
        what = "GradientAverager"
        names, params = [], []
        for i, entry in enumerate(parameters):
            name, p = entry if isinstance(entry, (tuple, list)) else (None, entry)
            if not isinstance(p, torch.Tensor):
                raise KbnError(f"{what}: parameter {i} is {type(p).__name__}, not a tensor")
            names.append(str(name) if name is not None else f"parameter {i} {tuple(p.shape)}")
            params.append(p)
        if not params:
            raise KbnError(f"{what}: no parameters")
        rank, world = int(rank), int(world)
        if world < 1 or not 0 <= rank < world:
            raise KbnError(f"{what}: rank {rank} of world {world}")
        device = params[0].device
        for name, p in zip(names, params):
            if not p.is_cuda:
                raise KbnError(f"{what}: {name} is on {p.device}: a CUDA/HIP device is required (no CPU fallback)")
            if p.dtype is not torch.float32:
                raise KbnError(f"{what}: {name} is {p.dtype}, expected float32")
            if p.device != device:
                raise KbnError(f"{what}: parameters live on different devices ({device} and {p.device})")
            if not p.is_contiguous():
                raise KbnError(f"{what}: {name} must be dense (contiguous), got strides {p.stride()}")
        if world > 1 and not (dist.is_initialized() and dist.get_world_size() == world and dist.get_rank() == rank):
            raise KbnError(f"{what}: rank {rank} of world {world} needs an initialised process group of that size (kb.dist.init)")
        self.names, self.params = names, params
        self.rank, self.world = rank, world
        self.collective = world > 1 or (bool(reduce_single) and dist.is_initialized())
        self.offsets, self.total = bucket_layout([p.numel() for p in params])
        self.buffer = torch.zeros(max(self.total, 4), dtype=torch.float32, device=device)
        self.views = [self.buffer[o:o + p.numel()].view(p.shape) for o, p in zip(self.offsets, params)]
        self._agreed = None      # per parameter: has a gradient (a tuple of bool), once the first average call has settled it

    @torch.no_grad()
    def broadcast_parameters(self, src: int = 0) -> None:
        if not self.collective:
            return
        from . import ops
        data = [p.detach() for p in self.params]
        ops.multi_tensor_scale_copy(data, self.views, 1.0)
        dist.broadcast(self.buffer, src=int(src))
        ops.multi_tensor_scale_copy(self.views, self.params, 1.0)
        self.buffer.zero_()      # the segments of parameters without a gradient must be zero in average()

    def _agree(self, mask) -> None:
        """The first average call's check; `mask` None on a rank without frames."""
        n = len(self.params)
        if not self.collective:
            self._agreed = mask
            return
        votes = torch.zeros(2 * n, dtype=torch.int32)
        if mask is not None:
            has = torch.tensor(mask, dtype=torch.int32)
            votes[:n], votes[n:] = has, 1 - has
        votes = votes.to(self.buffer.device)
        dist.all_reduce(votes, op=dist.ReduceOp.MAX)
        votes = votes.cpu()
        has, has_not = votes[:n], votes[n:]
        split = torch.nonzero(has * has_not)
        if split.numel():      # every rank reads the same reduced votes: all of them raise, none waits in the next collective
            i = int(split[0])
            raise KbnError(f"GradientAverager: the ranks disagree on which parameters have a gradient, first on {self.names[i]} "
                           f"(rank {self.rank} {'has no frames' if mask is None else 'has one' if mask[i] else 'has none'}): they built different "
                           "models, or one of them skipped a part of its backward pass")
        if bool((has + has_not).all()):
            self._agreed = tuple(bool(v) for v in has.tolist())

    def average(self, n_local: int, n_global: int) -> None:
        what = "GradientAverager.average"
        n_local, n_global = int(n_local), int(n_global)
        if n_global < 1 or not 0 <= n_local <= n_global:
            raise KbnError(f"{what}: {n_local} local frames of {n_global}")
        if n_local == 0 and not self.collective:
            raise KbnError(f"{what}: no frames and no other rank")
        mask = tuple(p.grad is not None for p in self.params) if n_local else None
        if self._agreed is None:
            self._agree(mask)
        elif mask is not None and mask != self._agreed:
            i = next(j for j, (a, b) in enumerate(zip(mask, self._agreed)) if a != b)
            raise KbnError(f"{what}: {self.names[i]} has {'a' if mask[i] else 'no'} gradient on rank {self.rank}, on the first call it "
                           f"had {'one' if self._agreed[i] else 'none'}")
        bound = self._agreed if self._agreed is not None else mask
        if n_local:
            from . import ops
            ops.multi_tensor_scale_copy([p.grad for p, m in zip(self.params, mask) if m], [v for v, m in zip(self.views, mask) if m],
                                        n_local / n_global)
        else:
            self.buffer.zero_()
        if self.collective:
            dist.all_reduce(self.buffer, op=dist.ReduceOp.SUM)
        if bound is not None:
            for p, v, m in zip(self.params, self.views, bound):
                if m:
                    p.grad = v


def every_rank_has_frames(n_global: int, world: int) -> bool:
    """Does `shard_bounds` give every rank at least one of `n_global` frames?  The same answer on every rank: a training loop
    whose pose networks run synchronised BatchNorm skips a short last batch for which it is False (a rank without frames runs no
    forward and cannot join BatchNormGroup's collectives)."""
    return int(n_global) >= int(world)


class BatchNormGroup:
    """The ranks whose frames one BatchNorm2d layer in 'batch' mode normalises over: what PoseNetModel.sync_batch_norm and
    ResNetPoseNetModel.sync_batch_norm take, next to GradientAverager in the data-parallel training step.

        group = kb.dist.BatchNormGroup(rank, world)
        pose_model.requires_grad_(True).set_batch_norm("batch").sync_batch_norm(group)

    Without it each rank normalises with the statistics of its own shard (the reference's torch.nn.DataParallel does the same,
    src/kbnet_model.py:408-415), and the all-reduced gradient is that of another function than the one a single process
    differentiates on the whole batch.  With it every layer's forward gathers the ranks' fp64 (count, mean, M2) records and every
    backward the ranks' two fp64 per-channel sums (ops.batch_norm_act_sync): `gather` below, one all_gather_into_tensor each, enqueued
    without a host synchronisation.  The merges run in rank order on every rank, so the result does not depend on the backend.

    Every rank must hold at least one frame (`every_rank_has_frames`) and make the same forward -- and backward -- calls in the same
    order; a mismatch waits in a collective until the backend's timeout.  With world == 1 and no `reduce_single` no collective runs
    (as in GradientAverager); `reduce_single=True` runs them on a one-rank group, for tests and timings.  Backends: "nccl" (RCCL),
    and "gloo" with device tensors (ranks that share a device)."""

    def __init__(self, rank: int, world: int, reduce_single: bool = False):
        rank, world = int(rank), int(world)
        if world < 1 or not 0 <= rank < world:
            raise KbnError(f"BatchNormGroup: rank {rank} of world {world}")
        if world > 1 and not (dist.is_initialized() and dist.get_world_size() == world and dist.get_rank() == rank):
            raise KbnError(f"BatchNormGroup: rank {rank} of world {world} needs an initialised process group of that size (kb.dist.init)")
        self.rank, self.world = rank, world
        self.collective = world > 1 or (bool(reduce_single) and dist.is_initialized())

    def gather(self, vector: torch.Tensor) -> torch.Tensor:
        """world x len(vector): row r is rank r's `vector` (a dense fp64 device vector of the same length on every rank)."""
        if vector.dtype is not torch.float64 or vector.dim() != 1 or not vector.is_cuda or not vector.is_contiguous():
            raise KbnError(f"BatchNormGroup.gather: a dense float64 CUDA/HIP vector, got {vector.dtype} {tuple(vector.shape)} on {vector.device}")
        if not self.collective:
            return vector.unsqueeze(0)
        out = torch.empty(self.world * vector.numel(), dtype=torch.float64, device=vector.device)      # flat: gloo chunks it by rank
        dist.all_gather_into_tensor(out, vector)
        return out.view(self.world, vector.numel())


def barrier():
    if dist.is_initialized():
        dist.barrier()


def max_over_ranks(value: float, device) -> float:
    if not dist.is_initialized():
        return value
    t = torch.tensor([value], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def gather_over_ranks(value: float, device) -> list:
    """`value` of every rank, rank order (a one-element list without a process group): per-rank rates of a run."""
    if not dist.is_initialized():
        return [float(value)]
    world = dist.get_world_size()
    t = torch.zeros(world, dtype=torch.float64, device=device)
    t[dist.get_rank()] = value
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return [float(v) for v in t.tolist()]


def sum_over_ranks(values: torch.Tensor) -> torch.Tensor:
    """Element-wise sum of a small tensor over all ranks (in place; identity without a process group)."""
    if dist.is_initialized():
        dist.all_reduce(values, op=dist.ReduceOp.SUM)
    return values


def mean_metrics_over_ranks(per_frame: torch.Tensor) -> torch.Tensor:
    """The reference's evaluation summary over a sharded run: it averages the per-sample MAE / RMSE / iMAE / iRMSE over
    ALL samples (reference src/kbnet.py:952-984, np.mean over the arrays filled at :932-950).  `per_frame`: this
    rank's N_local x 4 metrics from ops.eval_metrics (N_local may be 0 and may differ between ranks); returns the 4
    means over the frames of every rank (fp64, on per_frame's device).  ONE all-reduce of five numbers."""
    acc = torch.zeros(5, dtype=torch.float64, device=per_frame.device)
    if per_frame.numel():
        acc[:4] = per_frame.to(torch.float64).sum(dim=0)
    acc[4] = per_frame.shape[0]
    sum_over_ranks(acc)
    return acc[:4] / acc[4].clamp_min(1.0)


# ------------------------------------------------------------------------------------ what kb.training.train_ranks(rank, world) adds
def broadcast_rng_state(src: int = 0) -> None:
    """Rank `src`'s random state becomes everybody's: NumPy's global state, torch's CPU generator and the generator of the current
    HIP device (where one is visible), in one broadcast_object_list.  After it the ranks draw the same np.random and torch.rand
    numbers -- what Transforms.transform(shard=...) and TrainingFrameLoader(crops="global") need to build, between them, the batch
    one process builds.  torch.initial_seed() is not part of a generator's state: pass rank `src`'s Transforms.seed explicitly
    (kb.training.train_ranks does).  Nothing happens without a process group."""
    if not dist.is_initialized():
        return
    import numpy as np
    on_device = torch.cuda.is_available()
    state = [None]
    if dist.get_rank() == int(src):
        state = [(np.random.get_state(), torch.get_rng_state(), torch.cuda.get_rng_state() if on_device else None)]
    dist.broadcast_object_list(state, src=int(src))
    if dist.get_rank() != int(src):
        numpy_state, cpu_state, device_state = state[0]
        np.random.set_state(numpy_state)
        torch.set_rng_state(cpu_state)
        if on_device and device_state is not None:
            torch.cuda.set_rng_state(device_state)


def broadcast_object(value, src: int = 0):
    """Rank `src`'s picklable `value` on every rank (itself without a process group)."""
    if not dist.is_initialized():
        return value
    box = [value if dist.get_rank() == int(src) else None]
    dist.broadcast_object_list(box, src=int(src))
    return box[0]


class StopVote:
    """How the ranks of a run in sessions (kb.training.train_ranks_resumable) agree to stop on the same step: vote(wish) is True on
    every rank when any rank wishes -- one all-reduce (MAX) of one integer on a CPU tensor over gloo, so nothing waits for the
    device.  Signals and clocks differ between ranks, and a rank that left the loop alone would leave the others waiting in the
    next step's all-reduce; so every rank calls vote() after every step, whether it wishes or not: a collective only some ranks
    enter is the one way to hang.

    Construction is itself a collective where the default group is not gloo's (RCCL moves device tensors only): every rank makes the
    gloo group beside it (new_group), in the same place.  Under gloo the default group carries the vote.  With world == 1 no
    collective runs and vote(wish) is wish."""

    def __init__(self, rank: int, world: int):
        rank, world = int(rank), int(world)
        if world < 1 or not 0 <= rank < world:
            raise KbnError(f"StopVote: rank {rank} of world {world}")
        if world > 1 and not (dist.is_initialized() and dist.get_world_size() == world and dist.get_rank() == rank):
            raise KbnError(f"StopVote: rank {rank} of world {world} needs an initialised process group of that size (kb.dist.init)")
        self.rank, self.world = rank, world
        self.collective = world > 1
        self.group = None
        if self.collective and dist.get_backend() != "gloo":
            self.group = dist.new_group(backend="gloo")
        self._box = torch.zeros(1, dtype=torch.int64)

    def vote(self, wish) -> bool:
        if not self.collective:
            return bool(wish)
        self._box[0] = 1 if wish else 0
        dist.all_reduce(self._box, op=dist.ReduceOp.MAX, group=self.group)
        return bool(int(self._box[0]))


def gather_frames(tensor: torch.Tensor, n_global: int, rank: int, world: int) -> torch.Tensor:
    """This rank's `shard_bounds` frames of a global batch -> all n_global frames, in rank order -- which is batch order, the shards
    being contiguous -- on every rank: one all_gather_into_tensor through slots of the largest shard's size.  For the summaries of
    kb.training.train_ranks, every n_summary steps; not a hot path.  `tensor` itself (detached) when world == 1."""
    tensor = tensor.detach()
    if int(world) == 1:
        return tensor
    lo, hi = shard_bounds(int(n_global), int(rank), int(world))
    if tensor.shape[0] != hi - lo:
        raise KbnError(f"gather_frames: rank {rank} holds {tensor.shape[0]} frames, shard_bounds gives {hi - lo} of {n_global}")
    per = -(-int(n_global) // int(world))
    slot = torch.zeros((per,) + tuple(tensor.shape[1:]), device=tensor.device, dtype=tensor.dtype)
    slot[:hi - lo] = tensor
    out = torch.empty((int(world) * per,) + tuple(tensor.shape[1:]), device=tensor.device, dtype=tensor.dtype)
    dist.all_gather_into_tensor(out.view(-1), slot.view(-1))      # flat: gloo chunks it by rank
    parts = []
    for r in range(int(world)):
        lo, hi = shard_bounds(int(n_global), r, int(world))
        parts.append(out[r * per:r * per + (hi - lo)])
    return torch.cat(parts, dim=0)
