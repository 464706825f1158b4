#!/usr/bin/env python3
"""Times one training step of the pose network on the GPU -- forward with autograd recorded, then backward of
L = sum(pose * cotangent) -- for (a) PoseNetModel (csrc/posenet.hip + csrc/posenet_backward.hip) and (b) the same network as
torch.nn modules on the device (Conv2d stride 2 without bias, BatchNorm2d, LeakyReLU(0.2); 1 x 1 conv, mean, x 0.01,
ops.pose_matrix), in both BatchNorm modes, beside (a)'s fused eval-mode forward.

    python tools/posenet_train_bench.py [--out FILE] [--quick] [--size N H W] [--encoder posenet|resnet18|resnet34]

--encoder resnet18 / resnet34: ResNetPoseNetModel(trainable=True) (csrc/conv_affine.hip, csrc/conv_affine_backward.hip and the
BatchNorm and stride-2 kernels of csrc/posenet_backward.hip) beside the reference's block structure as torch.nn modules
(src/net_utils.py:572-667: the activation twice on the main path, a bias-free 1 x 1 projection where the shape changes).

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


class _ConvBN(torch.nn.Module):
    def __init__(self, cin, f, k, stride, norm=True):
        super().__init__()
        self.conv = torch.nn.Conv2d(cin, f, k, stride=stride, padding=k // 2, bias=False)
        if norm:
            self.batch_norm = torch.nn.BatchNorm2d(f)

    def forward(self, x):
        x = self.conv(x)
        return torch.nn.functional.leaky_relu(self.batch_norm(x), 0.2) if hasattr(self, "batch_norm") else x


class _Block(torch.nn.Module):
    def __init__(self, cin, f, stride):
        super().__init__()
        self.conv1, self.conv2 = _ConvBN(cin, f, 3, stride), _ConvBN(f, f, 3, 1)
        self.projection = _ConvBN(cin, f, 1, stride, norm=False)

    def forward(self, x):
        a = self.conv2(self.conv1(x))
        skip = self.projection(x) if a.shape != x.shape else x
        return torch.nn.functional.leaky_relu(a + skip, 0.2)


class TorchResNetPose(torch.nn.Module):
    """The modules carry the reference's keys, so the synthetic state dicts load with strict=True."""

    def __init__(self, n_layer, enc, dec):
        super().__init__()
        filters, hidden = kb.posenet_resnet.RESNET_FILTERS, kb.posenet_resnet.RESNET_DECODER_FILTERS
        self.encoder, self.decoder = torch.nn.Module(), torch.nn.Module()
        self.encoder.conv1 = _ConvBN(6, filters[0], 7, 2)
        cin = filters[0]
        for stage, (count, f) in enumerate(zip(kb.posenet_resnet.RESNET_BLOCKS[n_layer], filters[1:]), 2):
            blocks = []
            for b in range(count):
                blocks.append(_Block(cin, f, 2 if (b == 0 and stage > 2) else 1))
                cin = f
            setattr(self.encoder, f"blocks{stage}", torch.nn.Sequential(*blocks))
        layers = []
        for f in hidden:
            layers.append(_ConvBN(cin, f, 3, 2))
            cin = f
        layers.append(_ConvBN(cin, 6, 1, 1, norm=False))
        self.decoder.conv = torch.nn.Sequential(*layers)
        self.encoder.load_state_dict(enc, strict=True)
        self.decoder.load_state_dict(dec, strict=True)

    def forward(self, image0, image1):
        x = self.encoder.conv1(torch.cat([image0, image1], dim=1))
        x = torch.nn.functional.max_pool2d(x, 3, stride=2, padding=1)
        for stage in range(2, 6):
            x = getattr(self.encoder, f"blocks{stage}")(x)
        return kb.ops.pose_matrix(0.01 * self.decoder.conv(x).mean(dim=(2, 3)))


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
    ap.add_argument("--encoder", choices=("posenet", "resnet18", "resnet34"), default="posenet")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("posenet_train_bench: needs the GPU (no CPU timing stands in for it)")
    dev = torch.device("cuda:0")
    n, h, w = a.size
    iters = 3 if a.quick else 30
    resnet = int(a.encoder[6:]) if a.encoder != "posenet" else 0
    enc, dec = kb.synthetic.make_resnet_pose_weights(resnet, seed=5) if resnet else kb.synthetic.make_posenet_weights(seed=5)
    image0, image1 = (t.to(dev) for t in kb.synthetic.make_image_pair(n, h, w, seed=6))
    cot = torch.randn(n, 4, 4, device=dev, generator=torch.Generator(device=dev).manual_seed(7))
    lines = [f"# tools/posenet_train_bench.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}: {n} x 3 x {h} x {w}, "
             f"{a.encoder}, filters {list(kb.posenet_resnet.RESNET_FILTERS if resnet else FILTERS)}",
             "# one step = forward (autograd recorded) + backward of sum(pose * cotangent); median [min, max] of 5 windows of "
             f"{iters} steps, ms"]
    for mode in ("running", "batch"):
        ours = kb.posenet_resnet.ResNetPoseNetModel(resnet, device=dev, trainable=True) if resnet else kb.modules.PoseNetModel(device=dev)
        ours.load_state_dicts(enc, dec)
        ours.requires_grad_(True).set_batch_norm(mode)
        theirs = (TorchResNetPose(resnet, enc, dec) if resnet else TorchPoseNet(enc, dec)).to(dev)
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
        if resnet:
            named = dict(theirs.encoder.named_parameters())
            pairs = [(p.grad, named[k].grad) for k, p in ours.encoder.named_parameters() if k.endswith("conv.weight") and p.grad is not None]
        else:
            pairs = [(getattr(ours.encoder, f"conv{i}").conv.weight.grad, theirs.convs[i - 1].weight.grad) for i in range(1, 8)]
        for ga, gb in pairs:
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
            lines.append(f"#   {name:36s} x {cnt:2d}  {t:8.3f} ms{extra}")
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
