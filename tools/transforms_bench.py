#!/usr/bin/env python3
"""Times the training augmentation on the GPU: (a) kb.transforms.Transforms.transform (csrc/augment.hip: a selection launch and an
apply launch) against (b) the reference's algorithm written out in torch on the same device -- per-sample Python loops, and for the
removal nonzero(), randperm() and int() of a device scalar for every flagged frame, as src/transforms.py does it.

    python tools/transforms_bench.py [--out FILE] [--quick] [--probe]

Shape: the training bench's batch, 8 x 3 x 320 x 768: three images, the sparse depth (about 5 % positive, as KITTI's), the filtered
sparse depth and its validity map -- the six tensors of the reference's call.  Rows: the KITTI script's options (remove
[0.6, 0.7], p = 1, so about half the frames are flagged), and the same with both flips and uniform noise on.

Method: after a warm-up of the same shapes, 5 windows of `iters` calls each between two device events; reported per call: the
median window with the smallest and largest.  Host time: a host clock around the same loop WITHOUT a trailing synchronise -- what
a training loop pays to enqueue the call ((b) synchronises inside, so its host time is its whole time).  Device time of the two
launches: ops.PROFILE's event pairs, one call a pair, in a pass of their own.  The inputs of one call are 94 MB and its outputs
as much, inside the 256 MiB last-level cache, so the calls rotate through 8 input sets (755 MB between two uses of one set).
Bytes per second of the apply launch: 8 B an element (read once, written once) over its device time.

--probe appends where the selection launch's time goes: ops.augment on ONE range map 8 x 1 x 320 x 768 (24 rotating inputs, the
median of 40 ops.PROFILE event pairs) with 0 %, 5 %, 20 % and 100 % of it positive, 1, 4 or 8 frames flagged, at density 0 (k = 0
ends the kernel after the read of the frame and the candidate list) and at density 0.65 (everything)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import kbnet_amd as kb  # noqa: E402

N, H, W = 8, 320, 768
SETS = 8
ROWS = [
    ("kitti: remove [0.6, 0.7]", dict(normalized_image_range=[0, 1], random_flip_type=["none"], random_remove_points=[0.60, 0.70],
                                      random_noise_type="none", random_noise_spread=-1)),
    ("+ flips + uniform noise", dict(normalized_image_range=[0, 1], random_flip_type=["horizontal", "vertical"], random_remove_points=[0.60, 0.70],
                                     random_noise_type="uniform", random_noise_spread=0.5)),
]


def make_inputs(dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g, device=dev)
    images = [torch.floor(256.0 * rnd(N, 3, H, W)) for _ in range(3)]
    sparse = torch.where(rnd(N, 1, H, W) < 0.05, 1.0 + 79.0 * rnd(N, 1, H, W), torch.zeros((), device=dev))
    _, validity, filtered = kb.ops.preprocess(None, sparse)
    return images, [sparse], [filtered, validity]


class TorchTransforms:
    """The reference's algorithm (src/transforms.py:61-359), restated for this tool: the same decisions, the same per-sample loops
    and the same torch calls, but without writing into the caller's tensors (the range maps are cloned once a call)."""

    def __init__(self, ours):
        self.t = ours

    def transform(self, images_arr, range_maps_arr, validity_maps_arr, p):
        t = self.t
        n = images_arr[0].shape[0]
        device = images_arr[0].device
        do = np.random.rand(n) <= p
        lo, hi = [float(v) for v in t.normalized_image_range]
        if (lo, hi) == (0.0, 1.0):
            images_arr = [x / 255.0 for x in images_arr]
        elif (lo, hi) == (-1.0, 1.0):
            images_arr = [2.0 * (x / 255.0) - 1.0 for x in images_arr]
        else:
            images_arr = [x.clone() for x in images_arr]
        range_maps_arr = [x.clone() for x in range_maps_arr]
        validity_maps_arr = [x.clone() for x in validity_maps_arr]
        for enabled, dims in ((t.do_random_horizontal_flip, [-1]), (t.do_random_vertical_flip, [-2])):
            if enabled:
                flip = np.logical_and(do, np.random.rand(n) <= 0.5)
                for arr in (images_arr, range_maps_arr, validity_maps_arr):
                    for x in arr:
                        for b in range(n):
                            if flip[b]:
                                x[b, ...] = torch.flip(x[b], dims=dims)
        if t.do_random_remove_points:
            remove = np.logical_and(do, np.random.rand(n) <= 0.5)
            a, c = t.remove_points_range
            densities = (c - a) * torch.rand(n, device=device) + a
            for x in range_maps_arr:
                for b in range(n):
                    if remove[b]:
                        frame = x[b]
                        indices = (frame > 0).nonzero(as_tuple=True)
                        subset = torch.randperm(indices[0].shape[0], device=device)
                        subset = subset[0:int(densities[b] * subset.shape[0])]
                        frame[tuple(i[subset] for i in indices)] = 0.0
        if t.do_random_noise:
            noise = np.logical_and(do, np.random.rand(n) <= 0.5)
            for x in range_maps_arr:
                for b in range(n):
                    if noise[b]:
                        frame = x[b]
                        mask = torch.where(frame > 0, torch.ones_like(frame), torch.zeros_like(frame))
                        if t.random_noise_type == "gaussian":
                            frame = frame + t.random_noise_spread * torch.randn(*frame.shape, device=device)
                        else:
                            frame = frame + t.random_noise_spread * (torch.rand(*frame.shape, device=device) - 0.5)
                        x[b, ...] = frame * mask
        return images_arr, range_maps_arr, validity_maps_arr


def windows(fn, sets, iters, count=5):
    """([device ms a call] per window, [host ms a call] per window)."""
    for i in range(len(sets)):
        fn(sets[i])
    torch.cuda.synchronize()
    device, host = [], []
    for _ in range(count):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        for i in range(iters):
            fn(sets[i % len(sets)])
        b.record()
        host.append((time.perf_counter() - t0) * 1e3 / iters)
        torch.cuda.synchronize()
        device.append(a.elapsed_time(b) / iters)
    return device, host


def spread(values, unit="us", scale=1e3):
    return f"{statistics.median(values) * scale:9.1f} {unit} (min {min(values) * scale:.1f}, max {max(values) * scale:.1f})"


def stages(fn, sets, iters):
    """Device time of the two launches, from ops.PROFILE: {name: [ms a call]}."""
    kb.ops.PROFILE = []
    try:
        for i in range(iters):
            fn(sets[i % len(sets)])
        torch.cuda.synchronize()
        out = {}
        for name, _, _, _, nbytes, start, end in kb.ops.PROFILE:
            out.setdefault(name, []).append(start.elapsed_time(end))
        return out
    finally:
        kb.ops.PROFILE = None


def probe(dev):
    g = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda: torch.rand(N, 1, H, W, generator=g, device=dev)
    lines = ["selection probe: one range map, us a launch, median (min) of 40 calls",
             "  positive  flagged   density 0: read + list      density 0.65: everything"]
    for fraction in (0.0, 0.05, 0.2, 1.0):
        sets = [torch.where(rnd() < fraction, 1.0 + 79.0 * rnd(), torch.zeros((), device=dev)) for _ in range(24)]
        for flagged in (1, 4, 8):
            flags = [kb.ops.AUGMENT_REMOVE] * flagged + [0] * (N - flagged)
            cells = []
            for density in (0.0, 0.65):
                densities = torch.full((N,), density, device=dev)
                times = stages(lambda s: kb.ops.augment([], [s], [], flags, densities, seed=1, call=0), sets, 40)["augment_select"]
                cells.append(f"{statistics.median(times) * 1e3:7.1f} ({min(times) * 1e3:.1f})")
            lines.append(f"  {fraction:8.2f}  {flagged:7d}   {cells[0]:>24s}      {cells[1]:>24s}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--probe", action="store_true", help="also split the selection launch's time (see the module docstring)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("transforms_bench needs a GPU: a time measured anywhere else says nothing")
    dev = torch.device("cuda:0")
    kb._lib.load()
    sets = [make_inputs(dev, 100 + i) for i in range(2 if args.quick else SETS)]
    elements = sum(t.numel() for lst in sets[0] for t in lst)
    lines = [f"transforms_bench on {torch.cuda.get_device_name(0)}: {N} x 3 x {H} x {W}, six tensors, {elements * 4 / 1e6:.0f} MB in and as much out; "
             f"{float((sets[0][1][0] > 0).float().mean()) * 100:.1f} % of the depth positive; p = 1"]
    iters_a, iters_b = (10, 2) if args.quick else (200, 10)
    for label, options in ROWS:
        ours = kb.transforms.Transforms(seed=1, **options)
        theirs = TorchTransforms(ours)
        np.random.seed(0)
        torch.manual_seed(0)
        dev_a, host_a = windows(lambda s: ours.transform(s[0], s[1], s[2], 1.0), sets, iters_a)
        np.random.seed(0)
        torch.manual_seed(0)
        parts = stages(lambda s: ours.transform(s[0], s[1], s[2], 1.0), sets, 50 if not args.quick else 4)
        np.random.seed(0)
        torch.manual_seed(0)
        dev_b, host_b = windows(lambda s: theirs.transform(s[0], s[1], s[2], 1.0), sets, iters_b)
        apply_ms = statistics.median(parts["augment_apply"])
        lines += [f"[{label}]",
                  f"  (a) Transforms.transform   device {spread(dev_a)}   host, no trailing synchronise {spread(host_a)}",
                  f"      selection launch       device {spread(parts.get('augment_select', [0.0]))}   ({len(parts.get('augment_select', []))} calls with a flagged frame)",
                  f"      apply launch           device {spread(parts['augment_apply'])}   {8.0 * elements / (apply_ms * 1e-3) / 1e12:.2f} TB/s at 8 B an element",
                  f"  (b) the reference in torch device {spread(dev_b)}   host {spread(host_b)}",
                  f"  (a) / (b) = {statistics.median(dev_a) / statistics.median(dev_b):.4f}   ((b) / (a) = {statistics.median(dev_b) / statistics.median(dev_a):.0f} x)"]
    if args.probe:
        lines += probe(dev)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
