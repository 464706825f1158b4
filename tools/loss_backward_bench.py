#!/usr/bin/env python3
"""Times forward + backward of the objective on the GPU: (a) KBNetModel.compute_loss(...)[0].backward() (two HIP kernels and a few
scalar torch ops) against (b) the same arithmetic as a torch composition under autograd (tests/loss_oracle.py on cuda tensors,
fp32: what a user of the reference gets on this GPU), with the peak of allocated memory of each and the rate the backward kernel
alone reaches on the bytes it must move.

    python tools/loss_backward_bench.py [--out FILE] [--quick]

Method (that of tools/loss_bench.py): device events around a loop of calls after a warm-up of the same shapes; the median of 5
such windows; sizes whose inputs fit in the 256 MiB last-level cache rotate through enough input sets to exceed 768 MB between
two uses of the same set.  The backward kernel must move 52 B per pixel: 12 fp32 planes in, 1 out.  Peak memory is
torch.cuda.max_memory_allocated over one forward + backward, less what was allocated before it (the inputs)."""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import kbnet_amd as kb  # noqa: E402
import loss_oracle as lo  # noqa: E402
from loss_bench import ROTATE_BYTES, SIZES, make_inputs, timed  # noqa: E402


def leaves(s):
    """The input set with fresh leaves for the depth and the two poses."""
    s = list(s)
    for i in (3, 7, 8):
        s[i] = s[i].detach().requires_grad_(True)
    return s


def peak_of(fn, s):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn(s)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="fewer iterations (a check that the script runs)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("loss_backward_bench: needs the GPU (no CPU timing stands in for it)")
    dev = torch.device("cuda:0")
    model = kb.modules.KBNetModel.from_config(kb.kitti_config().narrow(), dev)

    def ours(s):
        s = leaves(s)
        model.compute_loss(*s)[0].backward()
        return s[3].grad

    def composition(s):
        s = leaves(s)
        lo.compute_loss(*s)["loss"].backward()
        return s[3].grad

    lines = [f"# tools/loss_backward_bench.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             "# forward + backward: (a) KBNetModel.compute_loss   (b) torch composition under autograd (tests/loss_oracle.py, fp32, cuda)",
             "# median [min, max] of 5 windows; peak = allocated beyond the inputs during one forward + backward",
             "# size            (a) ms                  (b) ms                     (b)/(a)  (a) peak   (b) peak   backward kernel ms  GB/s of 52 B/px  input sets"]
    for n, h, w in SIZES:
        pixels = n * h * w
        in_bytes = 48 * pixels
        copies = 1 if in_bytes > 256 * 2 ** 20 else math.ceil(ROTATE_BYTES / in_bytes)
        sets = [make_inputs(n, h, w, dev, seed=s) for s in range(copies)]
        iters_a = 4 if a.quick else max(20, int(1e9 / in_bytes))
        iters_b = 2 if a.quick else max(5, int(1e8 / in_bytes))
        ta = timed(ours, sets, iters_a)
        tb = timed(composition, sets, iters_b)
        gs = torch.rand(n, 8, device=dev, dtype=torch.float64) + 0.5
        out = (torch.empty(n, 1, h, w, device=dev), torch.empty(n, 2, 12, device=dev, dtype=torch.float64))
        tk = timed(lambda s: kb.ops.photometric_loss_backward(*s, gs, out=out), sets, iters_a)
        pa, pb = peak_of(ours, sets[0]), peak_of(composition, sets[0])
        lines.append(f"{n:2d} x {h} x {w:<5d}  {ta[0]:7.3f} [{ta[1]:.3f}, {ta[2]:.3f}]  {tb[0]:8.3f} [{tb[1]:.3f}, {tb[2]:.3f}]  {tb[0] / ta[0]:7.1f}  "
                     f"{pa / 1e6:7.1f} MB {pb / 1e6:8.1f} MB  {tk[0]:7.3f} [{tk[1]:.3f}, {tk[2]:.3f}]  {52 * pixels / tk[0] / 1e6:8.0f}  {copies}"
                     + ("" if copies == 1 else "  (fits in the last-level cache: rotated)"))
        print(lines[-1], flush=True)
        # same inputs, same answer: the timed paths agree.  Loose, because these images are white noise: a sample position that two
        # fp32 evaluations put on either side of an integer (about one in 10^4 per axis and pair at these widths) reads other taps,
        # and on white noise that changes the pixel's gradient by its own size, so two correct evaluations sit about sqrt(4e-4) =
        # 2e-2 apart in relative L2; a wrong pair, sign or weight is O(1).  The tests gate the gradient on band-limited images.
        ga, gb = ours(sets[0]).double(), composition(sets[0]).double()
        rel = float((ga - gb).norm() / gb.norm())
        lines.append(f"#   depth gradient of (a) vs (b) on set 0: relative L2 {rel:.1e}; image-sized tensors (4 B/px planes) beyond the inputs at the "
                     f"peak: (a) {pa / (4.0 * pixels):.1f}  (b) {pb / (4.0 * pixels):.1f}")
        print(lines[-1], flush=True)
        assert rel < 1e-1, rel
        del sets, out
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
