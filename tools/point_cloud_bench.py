#!/usr/bin/env python3
"""ops.point_cloud alone: the three launches of kbn_point_cloud_forward on 8 x 352 x 1216 (KITTI) and 8 x 480 x 640
(VOID), with colour, for a dense depth and for its 5 % sparse samples -- and beside them the same records formed in torch on the same
GPU (mask, gather, stack, byte views; the camera coordinates are made once, outside the timed window).

    python tools/point_cloud_bench.py [--calls 200]                                   # device events around windows of calls
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o p -- python tools/point_cloud_bench.py --calls 50 --no-torch

Under rocprofv3 the kernel statistics split a call into its three launches (point_count_kernel, point_scan_kernel,
point_emit_kernel).  Prints one JSON line; `bytes_per_call` is what the algorithm moves: the depth read twice, the image's three
planes read where a quad holds a kept pixel (counted as the whole image for the dense case and as 12 bytes a kept pixel for the sparse
one), a record written per kept pixel."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import kbnet_amd as kb  # noqa: E402

SHAPES = ((8, 352, 1216), (8, 480, 640))
DENSITIES = ("dense", "sparse5")


def make(n, h, w, density, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    image = torch.rand((n, 3, h, w), generator=g, device=dev)
    depth = 1.5 + 98.5 * torch.nn.functional.avg_pool2d(torch.rand((n, 1, h, w), generator=g, device=dev), 31, stride=1, padding=15)
    if density == "sparse5":
        depth = depth * (torch.rand((n, 1, h, w), generator=g, device=dev) < 0.05)
    k = torch.tensor([[0.58 * w, 0.0, 0.5 * w], [0.0, 1.92 * h, 0.5 * h], [0.0, 0.0, 1.0]], device=dev).repeat(n, 1, 1)
    return image, depth.contiguous(), kb.ops.intrinsics_inverse(k)


def torch_records(depth, coordinates, image):
    """The same bytes, frame by frame, with torch's own kernels: a list of M_i x 15 uint8 tensors."""
    n, _, h, w = depth.shape
    out = []
    for i in range(n):
        d = depth[i].reshape(1, -1)
        keep = (torch.isfinite(d) & (d > 0)).reshape(-1)
        xyz = (coordinates[i].reshape(3, -1) * d)[:, keep].t().contiguous()
        rgb = (image[i].reshape(3, -1)[:, keep] * 255.0).clamp(0.0, 255.0).to(torch.uint8).t()
        out.append(torch.cat([xyz.view(torch.uint8), rgb], dim=1))
    return out


def windows(fn, calls, count):
    times = []
    for _ in range(count):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for i in range(calls):
            fn(i)
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end) * 1e3 / calls)
    return [min(times), statistics.median(times), max(times)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200, help="calls a window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true", help="leave the torch formulation out (for a kernel trace of the operator alone)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "point_cloud_bench.py measures on the GPU: no device, no number"
    dev = torch.device("cuda")
    result = {"device": torch.cuda.get_device_name(0), "calls_per_window": args.calls, "windows": args.windows}
    for n, h, w in SHAPES:
        out = torch.empty((n, kb.ops.point_cloud_stride(h, w, True)), dtype=torch.uint8, device=dev)
        points = torch.empty(n, dtype=torch.int64, device=dev)
        work = torch.empty(kb.ops.point_cloud_workspace_bytes(n, h, w), dtype=torch.uint8, device=dev)
        for density in DENSITIES:
            sets = [make(n, h, w, density, dev, seed) for seed in range(4)]      # rotating inputs, as in pack_frames_bench.py

            def call(i):
                image, depth, kinv = sets[i % 4]
                kb.ops.point_cloud(depth, kinv, image, out=out, out_points=points, workspace=work)

            for i in range(8):
                call(i)
            torch.cuda.synchronize()
            entry = {"us_per_call": windows(call, args.calls, args.windows)}
            kept = float(points.double().sum())
            pixels = n * h * w
            entry["points_per_call"] = kept
            entry["bytes_per_call"] = 8.0 * pixels + (12.0 * pixels if density == "dense" else 12.0 * kept) + 15.0 * kept
            entry["gbytes_per_s"] = entry["bytes_per_call"] / entry["us_per_call"][1] * 1e-3
            if not args.no_torch:
                coordinates = kb.ops.camera_coordinates(sets[0][2], h, w)
                image, depth, _ = sets[(args.calls - 1) % 4]      # the set the last timed call used: `out` holds its records
                made = torch_records(depth, coordinates, image)
                for i, records in enumerate(made):
                    assert int(points[i]) == records.shape[0] and torch.equal(out[i, :records.numel()], records.reshape(-1)), (h, w, density, i)

                def torch_call(i):
                    image, depth, _ = sets[i % 4]
                    torch_records(depth, coordinates, image)

                torch_calls = max(1, args.calls // 10)
                torch_call(0)
                torch.cuda.synchronize()
                entry["torch_us_per_call"] = windows(torch_call, torch_calls, args.windows)
            result[f"{n}x{h}x{w}_{density}"] = entry
    print(json.dumps(result))


if __name__ == "__main__":
    main()
