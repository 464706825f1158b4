#!/usr/bin/env python3
"""Times one training step of the pose network on the GPU -- forward with autograd recorded, then backward of
L = sum(pose * cotangent) -- for (a) PoseNetModel (csrc/posenet.hip + csrc/posenet_backward.hip) and (b) the same network as
torch.nn modules on the device (Conv2d stride 2 without bias, BatchNorm2d, LeakyReLU(0.2); 1 x 1 conv, mean, x 0.01,
ops.pose_matrix), in both BatchNorm modes, beside (a)'s fused eval-mode forward.

    python tools/posenet_train_bench.py [--out FILE] [--quick] [--size N H W]

Method: device events around a loop of steps after a warm-up of the same shapes; the median of 5 windows.  Then one more step of
(a) with ops.PROFILE on: the time of every launch between its own pair of events (this brackets enqueue gaps too; a kernel trace
is the tool for kernel times), summed by kernel name.  Both sides start from the same weights and images; their parameter
gradients are compared before anything is timed."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import kbnet_amd as kb  # noqa: E402

KERNELS = kb.posenet.POSENET_KERNELS
FILTERS = kb.posenet.POSENET_FILTERS


class TorchPoseNet(torch.nn.Module):
    def __init__(self, enc, dec):
        super().__init__()
        self.convs, self.norms = torch.nn.ModuleList(), torch.nn.ModuleList()
        cin = 6
        for i, (f, k) in enumerate(zip(FILTERS, KERNELS), 1):
            conv = torch.nn.Conv2d(cin, f, k, stride=2, padding=k // 2, bias=False)
            norm = torch.nn.BatchNorm2d(f)
            conv.weight.data.copy_(enc[f"conv{i}.conv.weight"])
            norm.load_state_dict({key: enc[f"conv{i}.batch_norm.{key}"] for key in norm.state_dict()})
            self.convs.append(conv)
            self.norms.append(norm)
            cin = f
        self.head = torch.nn.Conv2d(cin, 6, 1, bias=False)
        self.head.weight.data.copy_(dec["conv.conv.weight"])

    def forward(self, image0, image1):
        x = torch.cat([image0, image1], dim=1)
        for conv, norm in zip(self.convs, self.norms):
            x = torch.nn.functional.leaky_relu(norm(conv(x)), 0.2)
        return kb.ops.pose_matrix(0.01 * self.head(x).mean(dim=(2, 3)))


def timed(step, iters):
    """Median, min, max over 5 windows of the mean time of one step [ms]."""
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    windows = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            step()
        b.record()
        torch.cuda.synchronize()
        windows.append(a.elapsed_time(b) / iters)
    return statistics.median(windows), min(windows), max(windows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="fewer iterations (a check that the script runs)")
    ap.add_argument("--size", type=int, nargs=3, default=(8, 352, 1216), metavar=("N", "H", "W"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("posenet_train_bench: needs the GPU (no CPU timing stands in for it)")
    dev = torch.device("cuda:0")
    n, h, w = a.size
    iters = 3 if a.quick else 30
    enc, dec = kb.synthetic.make_posenet_weights(seed=5)
    image0, image1 = (t.to(dev) for t in kb.synthetic.make_image_pair(n, h, w, seed=6))
    cot = torch.randn(n, 4, 4, device=dev, generator=torch.Generator(device=dev).manual_seed(7))
    lines = [f"# tools/posenet_train_bench.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}: {n} x 3 x {h} x {w}, "
             f"filters {list(FILTERS)}",
             "# one step = forward (autograd recorded) + backward of sum(pose * cotangent); median [min, max] of 5 windows of "
             f"{iters} steps, ms"]
    for mode in ("running", "batch"):
        ours = kb.modules.PoseNetModel(device=dev)
        ours.load_state_dicts(enc, dec)
        ours.requires_grad_(True).set_batch_norm(mode)
        theirs = TorchPoseNet(enc, dec).to(dev)
        theirs.train(mode == "batch")

        def step_ours():
            for p in ours.parameters():
                p.grad = None
            (ours.forward(image0, image1) * cot).sum().backward()

        def step_theirs():
            for p in theirs.parameters():
                p.grad = None
            (theirs(image0, image1) * cot).sum().backward()

        step_ours()
        step_theirs()
        worst = 0.0
        for i in range(1, 8):
            ga, gb = getattr(ours.encoder, f"conv{i}").conv.weight.grad, theirs.convs[i - 1].weight.grad
            worst = max(worst, float(((ga - gb).abs() / (gb.abs() + gb.pow(2).mean().sqrt())).max()))
        lines.append(f"# BatchNorm on {mode} statistics: conv weight gradients of (a) and (b) differ by at most {worst:.1e} of |b| + rms(b)")
        print(lines[-1], flush=True)
        ta, tb = timed(step_ours, iters), timed(step_theirs, iters)
        lines.append(f"{mode:8s} (a) HIP {ta[0]:8.3f} [{ta[1]:.3f}, {ta[2]:.3f}]   (b) torch.nn {tb[0]:8.3f} [{tb[1]:.3f}, {tb[2]:.3f}]   (a)/(b) {ta[0] / tb[0]:.2f}")
        print(lines[-1], flush=True)
        kb.ops.PROFILE = []
        try:
            step_ours()
            torch.cuda.synchronize()
            by_name = {}
            for name, work, executed, _, _, start, end in kb.ops.PROFILE:
                t, wk, ex, cnt = by_name.get(name, (0.0, 0.0, 0.0, 0))
                by_name[name] = (t + start.elapsed_time(end), wk + work, ex + (executed or 0.0), cnt + 1)
        finally:
            kb.ops.PROFILE = None
        for name, (t, wk, ex, cnt) in sorted(by_name.items(), key=lambda kv: -kv[1][0]):
            extra = f"  {wk / t / 1e9:8.2f} TFLOP/s algorithmic, executed / useful {ex / wk:.2f}" if wk else ""
            lines.append(f"#   {name:28s} x {cnt:2d}  {t:8.3f} ms{extra}")
            print(lines[-1], flush=True)
    with torch.no_grad():
        ours.set_batch_norm("running")
        tf = timed(lambda: ours.forward(image0, image1), iters)
    lines.append(f"fused eval-mode forward of (a), nothing recorded: {tf[0]:.3f} [{tf[1]:.3f}, {tf[2]:.3f}] ms")
    print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
