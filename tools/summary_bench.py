#!/usr/bin/env python3
"""Times the two image panels of KBNetModel.log_summary on the GPU: (a) ops.summary_image_panel and ops.summary_depth_panel
(csrc/summary.hip, one launch each) against (b) the reference's algorithm on the same GPU and host -- slice on the device, the
error expressions in torch on the device, .cpu() of every tensor, matplotlib's colormap frame by frame, torch.cat on the CPU, and
torchvision's make_grid restated (src/kbnet_model.py:466-650, src/log_utils.py:48-75).

    python tools/summary_bench.py [--out FILE] [--quick]

Shape: the training bench's batch, 8 x 3 x 320 x 768, every row of both panels (the training call has no ground truth and the
validation call no warped images; here both panels are full, 3 and 4 rows), n_display = 8: panels of 3 x 964 x 12306 and
3 x 1284 x 12306 floats.

Method: after a warm-up, 5 windows of `iters` calls between two device events; per call the median window with the smallest and
the largest.  Host time of (a): a host clock around the same loop without a trailing synchronise -- what the training loop loses
to enqueue the two launches.  (b) waits for the device in every .cpu(), so its wall time is what the training loop loses.  The
inputs rotate through 4 sets.  Bytes per second of (a): the panel written once plus every cell's sources read once."""
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
MAX_DEPTH = 100.0
EPSILON = 1e-8
SETS = 4


def make_inputs(dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g, device=dev)
    image0 = rnd(N, 3, H, W)
    image01 = (image0 + 0.1 * (rnd(N, 3, H, W) - 0.5)).clamp(0, 1)
    image02 = (image0 + 0.2 * (rnd(N, 3, H, W) - 0.5)).clamp(0, 1)
    output = 1.5 + 98.5 * rnd(N, 1, H, W)
    validity = (rnd(N, 1, H, W) < 0.05).float()
    sparse = output * (0.9 + 0.2 * rnd(N, 1, H, W)) * validity
    gt_validity = (rnd(N, 1, H, W) < 0.3).float()
    gt = torch.cat([output * (0.95 + 0.1 * rnd(N, 1, H, W)) * gt_validity, gt_validity], dim=1)
    return dict(image0=image0, image01=image01, image02=image02, output_depth0=output, sparse_depth0=sparse, validity_map0=validity, ground_truth0=gt)


def ours(s):
    image = kb.ops.summary_image_panel(s["image0"], s["image01"], s["image02"], n_display=N)
    depth = kb.ops.summary_depth_panel(s["output_depth0"], MAX_DEPTH, s["image0"], s["sparse_depth0"], s["validity_map0"], s["ground_truth0"], n_display=N)
    return image, depth


def colorize(T, colormap):
    """log_utils.colorize: to the host, matplotlib frame by frame, back to a tensor."""
    from matplotlib import colormaps
    cm = colormaps[colormap]
    T = np.squeeze(np.transpose(T.cpu().numpy(), (0, 2, 3, 1)), axis=-1)
    color = np.concatenate([np.expand_dims(cm(T[n, ...])[..., 0:3], 0) for n in range(T.shape[0])], axis=0)
    return torch.from_numpy(np.transpose(color, (0, 3, 1, 2)).astype(np.float32))


def make_grid(tensor, nrow, padding=2):
    """torchvision.utils.make_grid for a B x 3 x h x w CPU tensor, from its documented behaviour."""
    if tensor.shape[0] == 1:
        return tensor[0]
    nmaps = tensor.shape[0]
    xmaps = min(nrow, nmaps)
    ymaps = -(-nmaps // xmaps)
    height, width = tensor.shape[2] + padding, tensor.shape[3] + padding
    grid = tensor.new_full((3, height * ymaps + padding, width * xmaps + padding), 0.0)
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= nmaps:
                break
            grid.narrow(1, y * height + padding, height - padding).narrow(2, x * width + padding, width - padding).copy_(tensor[k])
            k += 1
    return grid


def theirs(s):
    """The reference's statements for the two panels (histograms and scalars left out), on device tensors as its training loop has them."""
    n_display = N
    image0_summary = s["image0"][0:n_display, ...]
    display_image = [torch.cat([image0_summary.cpu(), torch.zeros_like(image0_summary, device=torch.device("cpu"))], dim=-1)]
    display_depth = [display_image[-1]]
    for key in ("image01", "image02"):
        warped = s[key][0:n_display, ...]
        error = torch.mean(torch.abs(image0_summary - warped), dim=1, keepdim=True)
        display_image.append(torch.cat([warped.cpu(), colorize((error / 0.10).cpu(), "inferno")], dim=3))
    output = s["output_depth0"][0:n_display, ...]
    n_batch, _, n_height, n_width = output.shape
    display_depth.append(torch.cat([colorize((output / MAX_DEPTH).cpu(), "viridis"), torch.zeros(n_batch, 3, n_height, n_width)], dim=3))
    gt = s["ground_truth0"]
    for ref, validity in ((s["sparse_depth0"][0:n_display], s["validity_map0"][0:n_display]),
                          (torch.unsqueeze(gt[:, 0, :, :], dim=1)[0:n_display], torch.unsqueeze(gt[:, 1, :, :], dim=1)[0:n_display])):
        error = torch.abs(output - ref)
        error = torch.where(validity == 1.0, (error + EPSILON) / (ref + EPSILON), validity)
        display_depth.append(torch.cat([colorize((ref / MAX_DEPTH).cpu(), "viridis"), colorize((error / 0.05).cpu(), "inferno")], dim=3))
    return make_grid(torch.cat(display_image, dim=2), n_display), make_grid(torch.cat(display_depth, dim=2), n_display)


def windows(fn, sets, iters, count=5):
    """([device ms a call] per window, [host ms a call, no trailing synchronise] per window)."""
    for s in sets:
        fn(s)
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
    return f"{statistics.median(values) * scale:10.1f} {unit} (min {min(values) * scale:.1f}, max {max(values) * scale:.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("summary_bench needs a GPU: a time measured anywhere else says nothing")
    dev = torch.device("cuda:0")
    kb._lib.load()
    sets = [make_inputs(dev, 100 + i) for i in range(2 if args.quick else SETS)]
    image, depth = ours(sets[0])
    ref_image, ref_depth = theirs(sets[0])
    same = [float((a.cpu() == b).float().mean()) for a, b in ((image, ref_image), (depth, ref_depth))]
    nbytes = 4.0 * (image.numel() + depth.numel()) + 4.0 * N * H * W * (21 + 12)   # the panels + the planes each cell reads (3 + 9 + 9; 3 + 1 + 4 + 4)
    lines = [f"summary_bench on {torch.cuda.get_device_name(0)}: {N} x 3 x {H} x {W}, n_display {N}; panels {tuple(image.shape)} and {tuple(depth.shape)}, "
             f"{nbytes / 1e6:.0f} MB moved a call",
             f"  elements equal to the reference's run on this GPU (its scalar divisions run on the device there): image panel "
             f"{100 * same[0]:.4f} %, depth panel {100 * same[1]:.4f} %"]
    dev_a, host_a = windows(ours, sets, 5 if args.quick else 100)
    dev_image, _ = windows(lambda s: kb.ops.summary_image_panel(s["image0"], s["image01"], s["image02"], n_display=N), sets, 5 if args.quick else 100)
    dev_b, host_b = windows(theirs, sets, 1 if args.quick else 3, count=3 if args.quick else 5)
    a_ms = statistics.median(dev_a)
    lines += [f"  (a) both panels, two launches      device {spread(dev_a)}   {nbytes / (a_ms * 1e-3) / 1e12:.2f} TB/s   host, no trailing synchronise {spread(host_a)}",
              f"      the image panel alone          device {spread(dev_image)}",
              f"  (b) the reference's algorithm      wall   {spread(host_b, 'ms', 1.0)}   (device events around it {spread(dev_b, 'ms', 1.0)})",
              f"  host time lost a log_summary call: (b) {statistics.median(host_b):.1f} ms, (a) {statistics.median(host_a) * 1e3:.1f} us; "
              f"(b) / (a) device = {statistics.median(host_b) / a_ms:.0f} x"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
