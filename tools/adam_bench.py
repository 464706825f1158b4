#!/usr/bin/env python3
"""Times optimizer.step() over the parameters the reference trains -- the KITTI preset KBNetModel plus ResNetPoseNetModel(18) at
full widths, two groups with their own weight decay (reference src/kbnet.py:360-369) -- for kb.optim.Adam (one multi-tensor HIP
kernel, csrc/adam.hip) and torch.optim.Adam with its defaults (the comparator: what INTEGRATION documented before kb.optim.Adam),
with foreach=False and fused=True beside it for information.  The gradients are synthetic (N(0, 1), fixed between steps): the
optimizer's time does not depend on their values.

    python tools/adam_bench.py [--out FILE] [--quick]

Method: device events around a loop of steps after a warm-up; median [min, max] of 5 windows of 30 steps.  A window is as long as
the slower of host and device: the host side of a step (gathering ~ 130 tensors) is part of what a training loop pays, and is
reported on its own as well (wall time of the same loop with the device idle at its start).  Also: the launch count of the HIP step
and its achieved bytes per second from ops.PROFILE records (28 B an element) against the guide's measured HBM rate."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import kbnet_amd as kb  # noqa: E402

HBM_TBS = 6.29     # MI355X, measured float4 copy (8.0 TB/s peak)


def timed(step, iters):
    """(median, min, max) over 5 windows of the mean device-event time of one step [us], and the host's wall time per step [us]."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="fewer iterations (a check that the script runs)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("adam_bench: needs the GPU (no CPU timing stands in for it)")
    dev = torch.device("cuda:0")
    iters = 3 if a.quick else 30
    depth = kb.modules.KBNetModel.from_config(kb.kitti_config(), dev, trainable=True)
    pose = kb.posenet_resnet.ResNetPoseNetModel(n_layer=18, device=dev, trainable=True)
    pose.requires_grad_(True)
    shapes = [[tuple(p.shape) for p in m.parameters()] for m in (depth, pose)]
    gen = torch.Generator(device=dev).manual_seed(3)

    def make(cls, **kw):
        groups = [[torch.nn.Parameter(0.1 * torch.randn(s, device=dev, generator=gen)) for s in grp] for grp in shapes]
        for grp in groups:
            for p in grp:
                p.grad = torch.randn(p.shape, device=dev, generator=gen)
        return cls([{"params": groups[0], "weight_decay": 1e-4}, {"params": groups[1], "weight_decay": 1e-4}], lr=1e-4, **kw)

    elements = sum(int(torch.tensor(s).prod()) for grp in shapes for s in grp)
    tensors = sum(len(grp) for grp in shapes)
    lines = [f"# tools/adam_bench.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}: {tensors} tensors "
             f"({len(shapes[0])} depth + {len(shapes[1])} pose), {elements} elements, {28 * elements / 1e6:.1f} MB a step at 28 B an element",
             f"# optimizer.step(): median [min, max] of 5 windows of {iters} steps, device events, us; host = wall time of the loop per step"]
    print("\n".join(lines), flush=True)
    results = {}
    for label, cls, kw in (("kb.optim.Adam (HIP)", kb.optim.Adam, {}), ("torch.optim.Adam() [comparator]", torch.optim.Adam, {}),
                           ("torch.optim.Adam(foreach=False)", torch.optim.Adam, {"foreach": False}),
                           ("torch.optim.Adam(fused=True)", torch.optim.Adam, {"fused": True})):
        opt = make(cls, **kw)
        results[label] = timed(opt.step, iters)
        med, lo, hi, host = results[label]
        lines.append(f"{label:34s} {med:9.1f} [{lo:.1f}, {hi:.1f}]   host {host:8.1f}")
        print(lines[-1], flush=True)
        del opt
    ours, ref = results["kb.optim.Adam (HIP)"][0], results["torch.optim.Adam() [comparator]"][0]
    lines.append(f"HIP / comparator: {ours / ref:.2f}")
    print(lines[-1], flush=True)
    opt = make(kb.optim.Adam)
    opt.step()
    kb.ops.PROFILE = []
    try:
        opt.step()
        torch.cuda.synchronize()
        records = [(r[4], r[5].elapsed_time(r[6])) for r in kb.ops.PROFILE if r[0] == "adam_step"]
    finally:
        kb.ops.PROFILE = None
    total_b, total_ms = sum(r[0] for r in records), sum(r[1] for r in records)
    lines.append(f"# {len(records)} launches a step (table capacity {kb.ops.ADAM_TABLE_CAPACITY}); between their own events: " +
                 ", ".join(f"{b / 1e6:.1f} MB in {ms * 1e3:.1f} us = {b / ms / 1e9:.2f} TB/s" for b, ms in records))
    lines.append(f"# all launches: {total_b / 1e6:.1f} MB in {total_ms * 1e3:.1f} us = {total_b / total_ms / 1e9:.2f} TB/s, "
                 f"{total_b / total_ms / 1e9 / HBM_TBS * 100:.0f} % of the {HBM_TBS} TB/s a float4 copy reaches")
    print("\n".join(lines[-2:]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
