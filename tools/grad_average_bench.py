#!/usr/bin/env python3
"""Times kb.dist.GradientAverager over the parameters the reference trains -- the KITTI preset KBNetModel plus ResNetPoseNetModel(18)
at full widths, the list tools/adam_bench.py steps -- with synthetic gradients (N(0, 1): the time does not depend on their values):

  * the pack launches alone (ops.multi_tensor_scale_copy of every gradient into the flat buffer, csrc/multi_copy.hip), with their
    achieved bytes per second from ops.PROFILE records (8 B an element) against the guide's measured HBM rate;
  * the whole average() on one rank without a process group (pack + rebinding every .grad, no collective);
  * with --ranks N (N >= 2 visible devices, one process each, RCCL): the all-reduce of the buffer alone and the whole average(),
    the slowest rank's figure.

    python tools/grad_average_bench.py [--out FILE] [--quick] [--ranks N]

Method: tools/adam_bench.py's -- device events around a loop after a warm-up, median [min, max] of 5 windows of 30 calls; host =
wall time of the same loop per call.  Before each average() the gradients are bound to their own tensors again, as a backward pass
leaves them (130-odd attribute writes on the host, inside the host figure)."""
import argparse
import os
import socket
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import kbnet_amd as kb  # noqa: E402

HBM_TBS = 6.29     # MI355X, measured float4 copy (8.0 TB/s peak)


def timed(step, iters):
    """(median, min, max) over 5 windows of the mean device-event time of one call [us], and the host's wall time per call [us]."""
    for _ in range(5):
        step()
    torch.cuda.synchronize()
    windows, host = [], []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        t0 = time.perf_counter()
        for _ in range(iters):
            step()
        host.append((time.perf_counter() - t0) / iters * 1e6)
        b.record()
        torch.cuda.synchronize()
        windows.append(a.elapsed_time(b) / iters * 1e3)
    return statistics.median(windows), min(windows), max(windows), statistics.median(host)


def parameters(dev):
    """Parameters of the two networks' shapes with a gradient each, and the gradients."""
    depth = kb.modules.KBNetModel.from_config(kb.kitti_config(), dev, trainable=True)
    pose = kb.posenet_resnet.ResNetPoseNetModel(n_layer=18, device=dev, trainable=True)
    shapes = [tuple(p.shape) for m in (depth, pose) for p in m.parameters()]
    del depth, pose
    gen = torch.Generator(device=dev).manual_seed(3)
    params = [torch.nn.Parameter(0.1 * torch.randn(s, device=dev, generator=gen)) for s in shapes]
    grads = [torch.randn(s, device=dev, generator=gen) for s in shapes]
    return params, grads


def fmt(label, r):
    return f"{label:52s} {r[0]:9.1f} [{r[1]:.1f}, {r[2]:.1f}]   host {r[3]:8.1f}"


def measure(dev, rank, world, iters):
    """This rank's lines; with world > 1 inside an initialised process group."""
    import torch.distributed as dist
    params, grads = parameters(dev)
    averager = kb.dist.GradientAverager(params, rank, world)

    def bind():
        for p, g in zip(params, grads):
            p.grad = g

    def pack():
        kb.ops.multi_tensor_scale_copy(grads, averager.views, 0.5)

    def average():
        bind()
        averager.average(8, 8 * world)

    elements = sum(p.numel() for p in params)
    lines = [f"# {len(params)} tensors, {elements} elements, buffer {averager.total} elements ({4 * averager.total / 1e6:.1f} MB), "
             f"{8 * elements / 1e6:.1f} MB a pack at 8 B an element; rank {rank} of {world}",
             f"# median [min, max] of 5 windows of {iters} calls, device events, us; host = wall time of the loop per call"]
    lines.append(fmt("pack launches (multi_tensor_scale_copy)", timed(pack, iters)))
    if world > 1:
        lines.append(fmt(f"all_reduce(SUM) of the buffer alone, {world} ranks", timed(lambda: dist.all_reduce(averager.buffer), iters)))
    lines.append(fmt("average()" + (" (no collective)" if world == 1 else f", {world} ranks"), timed(average, iters)))
    pack()
    kb.ops.PROFILE = []
    try:
        pack()
        torch.cuda.synchronize()
        records = [(r[4], r[5].elapsed_time(r[6])) for r in kb.ops.PROFILE if r[0] == "multi_tensor_scale_copy"]
    finally:
        kb.ops.PROFILE = None
    total_b, total_ms = sum(r[0] for r in records), sum(r[1] for r in records)
    lines.append(f"# {len(records)} launches a pack (table capacity {kb.ops.MULTI_COPY_TABLE_CAPACITY}); between their own events: " +
                 ", ".join(f"{b / 1e6:.1f} MB in {ms * 1e3:.1f} us = {b / ms / 1e9:.2f} TB/s" for b, ms in records))
    lines.append(f"# all launches: {total_b / 1e6:.1f} MB in {total_ms * 1e3:.1f} us = {total_b / total_ms / 1e9:.2f} TB/s, "
                 f"{total_b / total_ms / 1e9 / HBM_TBS * 100:.0f} % of the {HBM_TBS} TB/s a float4 copy reaches")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="fewer iterations (a check that the script runs)")
    ap.add_argument("--ranks", type=int, default=1, help="processes, one per device, over RCCL (needs that many visible devices)")
    ap.add_argument("--rank", type=int, default=None, help=argparse.SUPPRESS)      # a child of --ranks N
    ap.add_argument("--port", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("grad_average_bench: needs the GPU (no CPU timing stands in for it)")
    iters = 3 if a.quick else 30
    have = torch.cuda.device_count()
    if a.rank is not None:      # one rank of a group: rank 0 prints the lines of the slowest figures' owner, itself
        import torch.distributed as dist
        torch.cuda.set_device(a.rank)
        dist.init_process_group(backend="nccl", init_method=f"tcp://127.0.0.1:{a.port}", rank=a.rank, world_size=a.ranks)
        try:
            lines = measure(torch.device("cuda", a.rank), a.rank, a.ranks, iters)
            every = [None] * a.ranks
            dist.all_gather_object(every, lines)
            if a.rank == 0:
                print("\n".join(line for rank_lines in every for line in rank_lines), flush=True)
        finally:
            dist.destroy_process_group()
        return
    lines = [f"# tools/grad_average_bench.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}, {have} visible device(s)"]
    lines += measure(torch.device("cuda:0"), 0, 1, iters)
    print("\n".join(lines), flush=True)
    if a.ranks > 1 and have < a.ranks:
        lines.append(f"# --ranks {a.ranks}: not measured, {have} visible device(s)")
        print(lines[-1], flush=True)
    elif a.ranks > 1:
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        env = dict(os.environ)
        for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
            env.pop(k, None)
        cmd = [sys.executable, os.path.abspath(__file__), "--ranks", str(a.ranks), "--port", str(port)] + (["--quick"] if a.quick else [])
        children = [subprocess.Popen(cmd + ["--rank", str(r)], stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL, text=True, env=env)
                    for r in range(a.ranks)]
        out = children[0].communicate(timeout=900)[0]
        for child in children[1:]:
            child.wait(timeout=60)
        lines += [f"# --ranks {a.ranks} over RCCL, every rank's lines in rank order"] + out.splitlines()
        print("\n".join(out.splitlines()), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
