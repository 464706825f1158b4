#!/usr/bin/env python3
"""Times one training step (forward, backward) of ResNetPoseNetModel(18) at full widths in 'batch' mode on 8 x 320 x 768 frames,
in one session on one card:

  * sync_batch_norm off: every layer on the statistics of this process's frames (ops.batch_norm_stats / batch_norm_act);
  * sync_batch_norm(BatchNormGroup(0, 1, reduce_single=True)) on a one-rank RCCL group: the synchronised path with its two
    collectives a layer (ops.batch_norm_act_sync), nothing to wait for but the collectives' own launches;
  * with --ranks N (N >= 2 visible devices, one process each, 8 frames a rank): the same step on an N-rank group, every rank's
    figure.

    python tools/bn_sync_bench.py [--out FILE] [--quick] [--ranks N]

Method: tools/kbnet_train_bench.py's -- device events around a loop after a warm-up, median [min, max] of 5 windows of 30 steps;
host = wall time of the same loop per step.  The launch and collective counts come from one step under ops.PROFILE."""
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
import torch.distributed as dist  # noqa: E402

import kbnet_amd as kb  # noqa: E402

FRAMES, HEIGHT, WIDTH = 8, 320, 768


def timed(step, iters):
    """(median, min, max) over 5 windows of the mean device-event time of one step [ms], and the host's wall time per step [ms]."""
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    windows, host = [], []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        t0 = time.perf_counter()
        for _ in range(iters):
            step()
        host.append((time.perf_counter() - t0) / iters * 1e3)
        b.record()
        torch.cuda.synchronize()
        windows.append(a.elapsed_time(b) / iters)
    return statistics.median(windows), min(windows), max(windows), statistics.median(host)


def fmt(label, r):
    return f"{label:64s} {r[0]:8.3f} [{r[1]:.3f}, {r[2]:.3f}] ms   host {r[3]:8.3f} ms"


def make_step(dev, group):
    pose = kb.posenet_resnet.ResNetPoseNetModel(n_layer=18, device=dev, trainable=True)
    pose.load_state_dicts(*kb.synthetic.make_resnet_pose_weights(18, list(kb.posenet_resnet.RESNET_FILTERS),
                                                                 list(kb.posenet_resnet.RESNET_DECODER_FILTERS), seed=7))
    pose.requires_grad_(True).set_batch_norm("batch").sync_batch_norm(group)
    image0, image1 = (t.to(dev) for t in kb.synthetic.make_image_pair(FRAMES, HEIGHT, WIDTH, seed=11))
    cot = torch.randn(FRAMES, 4, 4, device=dev, generator=torch.Generator(device=dev).manual_seed(5))

    def step():
        for p in pose.parameters():
            p.grad = None
        (pose.forward(image0, image1) * cot).sum().backward()

    return step


def launches(step):
    """name -> launches of one step."""
    step()
    kb.ops.PROFILE = []
    try:
        step()
        torch.cuda.synchronize()
        names = [r[0] for r in kb.ops.PROFILE]
    finally:
        kb.ops.PROFILE = None
    return {n: names.count(n) for n in sorted(set(names))}


def measure(dev, group, label, iters):
    step = make_step(dev, group)
    counts = launches(step)
    bn = {k: v for k, v in counts.items() if k.startswith("bn_")}
    collectives = (counts.get("bn_moments", 0) + counts.get("bn_act_backward_sums", 0)) if group is not None and group.collective else 0
    return [fmt(label, timed(step, iters)),
            f"#   {sum(counts.values())} launches a step, of BatchNorm: {bn}; {collectives} collectives a step"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="fewer iterations (a check that the script runs)")
    ap.add_argument("--ranks", type=int, default=1, help="also N processes, one per device, over RCCL (needs that many visible devices)")
    ap.add_argument("--rank", type=int, default=None, help=argparse.SUPPRESS)      # a child of --ranks N
    ap.add_argument("--port", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bn_sync_bench: needs the GPU (no CPU timing stands in for it)")
    iters = 3 if a.quick else 30
    have = torch.cuda.device_count()
    if a.rank is not None:      # one rank of a group
        torch.cuda.set_device(a.rank)
        dist.init_process_group(backend="nccl", init_method=f"tcp://127.0.0.1:{a.port}", rank=a.rank, world_size=a.ranks)
        try:
            lines = measure(torch.device("cuda", a.rank), kb.dist.BatchNormGroup(a.rank, a.ranks),
                            f"sync_batch_norm on, rank {a.rank} of {a.ranks} over RCCL, {FRAMES} frames a rank", iters)
            every = [None] * a.ranks
            dist.all_gather_object(every, lines)
            if a.rank == 0:
                print("\n".join(line for rank_lines in every for line in rank_lines), flush=True)
        finally:
            dist.destroy_process_group()
        return
    dev = torch.device("cuda:0")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    lines = [f"# tools/bn_sync_bench.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}, {have} visible device(s)",
             f"# ResNetPoseNetModel(18) full widths, 'batch' mode, one forward + backward on {FRAMES} x {HEIGHT} x {WIDTH}; median [min, max] "
             f"of 5 windows of {iters} steps, device events; host = wall time of the loop per step"]
    lines += measure(dev, None, "sync_batch_norm off", iters)
    print("\n".join(lines), flush=True)
    torch.cuda.set_device(dev)
    dist.init_process_group(backend="nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        group = kb.dist.BatchNormGroup(0, 1, reduce_single=True)
        assert group.collective
        more = measure(dev, group, "sync_batch_norm on, one-rank RCCL group (reduce_single)", iters)
        more += measure(dev, None, "sync_batch_norm off, again", iters)
    finally:
        dist.destroy_process_group()
    lines += more
    print("\n".join(more), flush=True)
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
