#!/usr/bin/env python3
"""Times the forward value of the objective on the GPU: (a) ops.photometric_loss (one HIP kernel) against (b) the same arithmetic
as a torch composition (tests/loss_oracle.py on cuda tensors, fp32: what a user of the reference gets on this GPU), with and
without the warped-image outputs, plus the read rate torch.sum reaches over the same inputs.

    python tools/loss_bench.py [--out FILE] [--quick]

Method: device events around a loop of calls after a warm-up of the same shapes; the median of 5 such windows.  (a)'s bytes per
second count the bytes that MUST move: 12 fp32 planes per pixel = 48 B (72 B with the two 3-channel image outputs).  The inputs
of one call are 48 B per pixel: 32 x 352 x 1216 is 657 MB and 32 x 480 x 640 is 472 MB, beyond the 256 MiB last-level cache;
8 x 352 x 1216 (164 MB) and 1 x 352 x 1216 (21 MB) fit in it, so those sizes rotate through enough input sets to exceed 768 MB
between two uses of the same set."""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import kbnet_amd as kb  # noqa: E402
import loss_oracle as lo  # noqa: E402

SIZES = [(32, 352, 1216), (8, 352, 1216), (32, 480, 640), (1, 352, 1216)]
ROTATE_BYTES = 768e6


def make_inputs(n, h, w, dev, seed):
    """Device-side inputs: uniform images, a smooth depth of 2-20 m with 5 % valid sparse points, poses of ~0.02 rad / ~0.5 m."""
    g = torch.Generator(device=dev).manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g, device=dev)
    images = [rnd(n, 3, h, w) for _ in range(3)]
    depth = 2.0 + 18.0 * torch.nn.functional.interpolate(rnd(n, 1, h // 16 + 2, w // 16 + 2), size=(h, w), mode="bilinear", align_corners=True)
    validity = (rnd(n, 1, h, w) < 0.05).float()
    sparse = depth * validity
    k = torch.zeros(n, 3, 3, device=dev)
    k[:, 0, 0] = k[:, 1, 1] = 0.6 * w
    k[:, 0, 2], k[:, 1, 2], k[:, 2, 2] = 0.5 * (w - 1), 0.5 * (h - 1), 1.0
    scale = torch.tensor([0.04, 0.04, 0.04, 1.0, 1.0, 1.0], device=dev)
    poses = [kb.ops.pose_matrix((rnd(n, 6) - 0.5) * scale) for _ in range(2)]
    return images + [depth.contiguous(), sparse, validity, k] + poses


def timed(fn, sets, iters):
    """Median over 5 windows of the mean time of one call [ms]; call i uses input set i mod len(sets)."""
    for i in range(max(2, len(sets))):
        fn(sets[i % len(sets)])
    torch.cuda.synchronize()
    windows = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(iters):
            fn(sets[i % len(sets)])
        b.record()
        torch.cuda.synchronize()
        windows.append(a.elapsed_time(b) / iters)
    return statistics.median(windows), min(windows), max(windows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="fewer iterations (a check that the script runs)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("loss_bench: needs the GPU (no CPU timing stands in for it)")
    dev = torch.device("cuda:0")
    lines = [f"# tools/loss_bench.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             "# (a) ops.photometric_loss   (b) torch composition (tests/loss_oracle.py, fp32, cuda)   median [min, max] of 5 windows",
             "# size            images  (a) ms                  (a) GB/s  (b) ms                     (b)/(a)   inputs   input sets"]
    for n, h, w in SIZES:
        pixels = n * h * w
        in_bytes = 48 * pixels
        copies = 1 if in_bytes > 256 * 2 ** 20 else math.ceil(ROTATE_BYTES / in_bytes)
        sets = [make_inputs(n, h, w, dev, seed=s) for s in range(copies)]
        iters_a = (4 if a.quick else max(20, int(2e9 / in_bytes)))
        iters_b = (2 if a.quick else max(5, int(2e8 / in_bytes)))
        for images in (False, True):
            fa = lambda s: kb.ops.photometric_loss(*s, return_images=images)
            ta = timed(fa, sets, iters_a)
            fb = lambda s: lo.compute_loss(*s)
            tb = timed(fb, sets, iters_b) if not images else tb   # the composition always forms the images: one timing serves both rows
            moved = (72 if images else 48) * pixels
            lines.append(f"{n:2d} x {h} x {w:<5d}  {'yes' if images else 'no ':3s}   {ta[0]:7.3f} [{ta[1]:.3f}, {ta[2]:.3f}]  {moved / ta[0] / 1e6:8.0f}  "
                         f"{tb[0]:8.3f} [{tb[1]:.3f}, {tb[2]:.3f}]  {tb[0] / ta[0]:7.1f}   {in_bytes / 1e6:5.0f} MB  {copies}"
                         + ("" if copies == 1 else "  (fits in the last-level cache: rotated)"))
            print(lines[-1], flush=True)
        if (n, h, w) == SIZES[0]:
            flat = [t for t in sets[0][:6]]
            ts = timed(lambda s: [t.sum() for t in flat], sets, 4 if a.quick else 20)
            lines.append(f"# torch.sum over the same {in_bytes / 1e6:.0f} MB of inputs (6 launches): {ts[0]:.3f} ms = {in_bytes / ts[0] / 1e6:.0f} GB/s read")
            print(lines[-1], flush=True)
        # same inputs, same answer: the timed paths agree (loose: the composition runs in fp32 throughout)
        sums = kb.ops.photometric_loss(*sets[0])
        got = kb.ops.loss_terms(sums, h, w).mean(0)
        want = lo.compute_loss(*sets[0])["per_frame"].double().mean(0)
        err = (got - want).abs()          # make_inputs' sparse depth IS the depth at the valid points: that term is exactly 0 in both
        rel = float(torch.where(want != 0, err / want.abs(), err).max())
        lines.append(f"#   terms of (a) vs (b) on set 0: max relative difference {rel:.1e}")
        print(lines[-1], flush=True)
        assert rel < 1e-3, rel
        del sets
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
