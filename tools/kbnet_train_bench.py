#!/usr/bin/env python3
"""Times one training step of the depth network on the GPU -- forward with autograd recorded, then backward of
L = sum(depth * cotangent) -- for (a) KBNetModel(trainable=True) (kbnet_train.py: the fp32 conv kernels, csrc/posenet_backward.hip,
csrc/conv_affine_backward.hip, csrc/kbnet_backward.hip) and (b) the same network in torch.nn.functional operations on the device
(conv2d without bias, leaky_relu(0.2), interpolate(mode='nearest'), cat, sigmoid), beside (a)'s fused forward.

    python tools/kbnet_train_bench.py [--out FILE] [--quick] [--size N H W] [--narrow] [--averager]

Method: device events around a loop of steps after a warm-up of the same shapes; the median of 5 windows.  Then one more step of (a)
with ops.PROFILE on: the time of every launch between its own pair of events (this brackets enqueue gaps too; a kernel trace is the
tool for kernel times), summed by kernel name.  Both sides start from the same weights and frames; their parameter gradients are
compared before anything is timed."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import kbnet_amd as kb  # noqa: E402


class TorchKBNet(torch.nn.Module):
    """KBNetModel.forward of the reference (src/kbnet_model.py:163-184 and what it calls) for the shipped presets: KB levels 0-3,
    level 4 plain.  The parameters are the three state dicts' tensors under their own keys."""

    def __init__(self, cfg, sds):
        super().__init__()
        self.cfg = cfg
        self.names = [f"{grp}::{k}" for grp, sd in zip(("s2d", "enc", "dec"), sds) for k in sd]
        self.weights = torch.nn.ParameterList([torch.nn.Parameter(v.clone()) for sd in sds for v in sd.values()])

    def forward(self, image, sparse_depth, validity_map_depth, intrinsics):
        cfg = self.cfg
        w = dict(zip(self.names, self.weights))

        def conv(x, key, stride=1, act=True):
            y = F.conv2d(x, w[key], None, stride=stride, padding=w[key].shape[-1] // 2)
            return F.leaky_relu(y, 0.2) if act else y

        x = torch.cat([sparse_depth, validity_map_depth], dim=1)
        y = kb.ops.s2d_pyramid(x, cfg.min_pools, cfg.max_pools)      # data on both sides
        for i in range(cfg.n_convolution_sparse_to_dense_pool):
            y = conv(y, f"s2d::pool_convs.{i}.conv.weight")
        depth = conv(torch.cat([y, x], dim=1), "s2d::conv.conv.weight")
        n, _, h0, w0 = image.shape
        kinv0 = kb.ops.intrinsics_inverse(intrinsics, 1.0, 1.0)
        kinv1 = kb.ops.intrinsics_inverse(intrinsics, ((w0 + 1) // 2) / w0, ((h0 + 1) // 2) / h0)
        conv_image, conv_depth, fused = conv(image, "enc::conv0_image.conv.weight"), conv(depth, "enc::conv0_depth.conv.weight"), None
        skips = []
        for level in range(4):
            p = f"enc::calibrated_backprojection{level + 1}."
            coords = kb.ops.camera_coordinates(kinv0 if level == 0 else kinv1, *conv_image.shape[2:])
            xyz = coords * conv(conv_depth, p + "proj_depth.conv.weight")
            new_fused = conv(torch.cat([conv_image, xyz] + ([] if fused is None else [fused]), dim=1), p + "conv_fused.conv.weight", 2)
            new_depth = conv(torch.cat([conv_depth, coords], dim=1), p + "conv_depth.conv_block.0.conv.weight", 2)
            conv_image = conv(conv_image, p + "conv_image.conv_block.0.conv.weight", 2)
            conv_depth, fused = new_depth, new_fused
            skips.append(torch.cat([fused, conv_depth], dim=1))
        y = torch.cat([conv(fused, "enc::conv5_image.conv_block.0.conv.weight", 2),
                       conv(conv_depth, "enc::conv5_depth.conv_block.0.conv.weight", 2)], dim=1)
        for i in (4, 3, 2, 1, 0):
            size = skips[i - 1].shape[2:] if i else (h0, w0)
            y = conv(F.interpolate(y, size=tuple(size), mode="nearest"), f"dec::deconv{i}.deconv.conv.conv.weight")
            y = conv(torch.cat([y, skips[i - 1]], dim=1) if i else y, f"dec::deconv{i}.conv.conv.weight")
        logits = conv(y, "dec::output0.conv.weight", act=False)
        return cfg.min_predict_depth / (torch.sigmoid(logits) + cfg.min_predict_depth / cfg.max_predict_depth)


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
    ap.add_argument("--size", type=int, nargs=3, default=(8, 320, 768), metavar=("N", "H", "W"))
    ap.add_argument("--narrow", action="store_true", help="KBNetConfig.narrow() widths")
    ap.add_argument("--averager", action="store_true", help="also time (a) with a world-1 kb.dist.GradientAverager.average() after the backward pass")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("kbnet_train_bench: needs the GPU (no CPU timing stands in for it)")
    dev = torch.device("cuda:0")
    n, h, w = a.size
    iters = 3 if a.quick else 30
    cfg = kb.kitti_config().narrow() if a.narrow else kb.kitti_config()
    sds = kb.synthetic.make_state_dicts(cfg, seed=5)
    frames = [t.to(dev) for t in kb.synthetic.make_frames(n, h, w, "kitti", seed=6)]
    cot = torch.randn(n, 1, h, w, device=dev, generator=torch.Generator(device=dev).manual_seed(7))
    lines = [f"# tools/kbnet_train_bench.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}: {n} x 3 x {h} x {w}, "
             f"encoder widths {list(cfg.n_filters_encoder_image)} / {list(cfg.n_filters_encoder_depth)}, decoder {list(cfg.n_filters_decoder)}",
             "# one step = forward (autograd recorded) + backward of sum(depth * cotangent); median [min, max] of 5 windows of "
             f"{iters} steps, ms"]
    ours = kb.modules.KBNetModel.from_config(cfg, dev, trainable=True)
    ours.load_state_dicts(*sds)
    theirs = TorchKBNet(cfg, sds).to(dev)

    def step_ours():
        for p in ours.parameters():
            p.grad = None
        (ours.forward(*frames) * cot).sum().backward()

    def step_theirs():
        for p in theirs.parameters():
            p.grad = None
        (theirs(*frames) * cot).sum().backward()

    step_ours()
    step_theirs()
    named = {f"{grp}::{k}": p for grp, mod in zip(("s2d", "enc", "dec"), ours.modules()) for k, p in mod.named_parameters()}
    worst = 0.0
    for key, p in zip(theirs.names, theirs.weights):
        ga, gb = named[key].grad, p.grad
        assert (ga is None) == (gb is None), key
        if gb is not None:
            worst = max(worst, float(((ga - gb).abs() / (gb.abs() + gb.pow(2).mean().sqrt())).max()))
    lines.append(f"# parameter gradients of (a) and (b) differ by at most {worst:.1e} of |b| + rms(b)")
    print(lines[-1], flush=True)
    ta, tb = timed(step_ours, iters), timed(step_theirs, iters)
    lines.append(f"step  (a) HIP {ta[0]:8.3f} [{ta[1]:.3f}, {ta[2]:.3f}]   (b) torch {tb[0]:8.3f} [{tb[1]:.3f}, {tb[2]:.3f}]   (a)/(b) {ta[0] / tb[0]:.2f}")
    print(lines[-1], flush=True)
    if a.averager:      # the data-parallel step's cost on one rank: the pack of every gradient into the one buffer, no collective
        averager = kb.dist.GradientAverager(ours.parameters(), 0, 1)

        def step_averaged():
            step_ours()
            averager.average(n, n)

        tw, again = timed(step_averaged, iters), timed(step_ours, iters)
        lines.append(f"step  (a) + GradientAverager(world 1).average {tw[0]:8.3f} [{tw[1]:.3f}, {tw[2]:.3f}]   (a) alone, timed again "
                     f"{again[0]:8.3f} [{again[1]:.3f}, {again[2]:.3f}]   difference {1e3 * (tw[0] - again[0]):+.0f} us "
                     f"({averager.total} buffer elements)")
        print(lines[-1], flush=True)
        for p in ours.parameters():
            p.grad = None
    kb.ops.PROFILE = []
    try:
        step_ours()
        torch.cuda.synchronize()
        by_name, launches = {}, len(kb.ops.PROFILE)
        for name, work, executed, _, _, start, end in kb.ops.PROFILE:
            t, wk, ex, cnt = by_name.get(name, (0.0, 0.0, 0.0, 0))
            by_name[name] = (t + start.elapsed_time(end), wk + work, ex + (executed or 0.0), cnt + 1)
    finally:
        kb.ops.PROFILE = None
    lines.append(f"# {launches} recorded launches in one step of (a), by kernel:")
    print(lines[-1], flush=True)
    for name, (t, wk, ex, cnt) in sorted(by_name.items(), key=lambda kv: -kv[1][0]):
        extra = f"  {wk / t / 1e9:8.2f} TFLOP/s algorithmic, executed / useful {ex / wk:.2f}" if wk and t else ""
        lines.append(f"#   {name:44s} x {cnt:2d}  {t:8.3f} ms{extra}")
        print(lines[-1], flush=True)
    with torch.no_grad():
        tf = timed(lambda: ours.forward(*frames), iters)
    lines.append(f"fused forward of (a), nothing recorded: {tf[0]:.3f} [{tf[1]:.3f}, {tf[2]:.3f}] ms")
    print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
