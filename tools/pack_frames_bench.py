#!/usr/bin/env python3
"""The device encoder of packed frames alone: ops.pack_frames on 8 x 352 x 1216 x 3 of 8 bits and on 16 planes of
352 x 1216 of 16 bits, for three contents -- `output` (what export_pack makes of a smoothed picture, a smooth dense depth and its
5 % sparse samples), `constant` (every b = 0: the emit pass writes header bytes and the left rows' first samples only) and `noise`
(every b = bits: the most fields and the most bytes).

    python tools/pack_frames_bench.py [--calls 200]                                   # device events around windows of calls
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o p -- python tools/pack_frames_bench.py --calls 50 --content output

Under rocprofv3 the kernel statistics split a call into its three launches (pack_sizes_kernel, pack_table_kernel,
pack_emit_kernel); --content keeps one content in the trace."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import kbnet_amd as kb  # noqa: E402

H, W, BATCH = 352, 1216, 8


def make(content, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    if content == "constant":
        return torch.full((BATCH, H, W, 3), 77, dtype=torch.uint8, device=dev), torch.full((2 * BATCH, H, W), 1234, dtype=torch.int16, device=dev)
    if content == "noise":
        return (torch.randint(0, 256, (BATCH, H, W, 3), generator=g, device=dev, dtype=torch.uint8),
                torch.randint(-32768, 32768, (2 * BATCH, H, W), generator=g, device=dev, dtype=torch.int16))
    image = torch.nn.functional.avg_pool2d(torch.rand((BATCH, 3, H, W), generator=g, device=dev), 9, stride=1, padding=4)
    depth_a = 1.5 + 98.5 * torch.nn.functional.avg_pool2d(torch.rand((BATCH, 1, H, W), generator=g, device=dev), 31, stride=1, padding=15)
    depth_b = depth_a * (torch.rand((BATCH, 1, H, W), generator=g, device=dev) < 0.05)
    planes = torch.empty((2 * BATCH, H, W), dtype=torch.int16, device=dev)
    rgb, _, _ = kb.ops.export_pack(image, depth_a, depth_b, out=(None, planes[:BATCH], planes[BATCH:]))
    return rgb, planes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200, help="calls a window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--content", default=None, choices=("output", "constant", "noise"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "pack_frames_bench.py measures on the GPU: no device, no number"
    dev = torch.device("cuda")
    work = torch.empty(max(kb.ops.pack_frames_workspace_bytes(BATCH, H, W, 3, 8), kb.ops.pack_frames_workspace_bytes(2 * BATCH, H, W, 1, 16)),
                       dtype=torch.uint8, device=dev)
    result = {"shape": [BATCH, H, W], "device": torch.cuda.get_device_name(0), "calls_per_window": args.calls, "windows": args.windows}
    for content in ((args.content,) if args.content else ("output", "constant", "noise")):
        sets = [make(content, dev, seed) for seed in range(4)]      # rotating, as in run_export_bench.py
        outs = (torch.empty((BATCH, kb.ops.pack_frames_stride(H, W, 3, 8)), dtype=torch.uint8, device=dev),
                torch.empty((2 * BATCH, kb.ops.pack_frames_stride(H, W, 1, 16)), dtype=torch.uint8, device=dev))
        sizes = (torch.empty(BATCH, dtype=torch.int64, device=dev), torch.empty(2 * BATCH, dtype=torch.int64, device=dev))
        for which in (0, 1):
            for i in range(8):
                kb.ops.pack_frames(sets[i % 4][which], out=outs[which], out_bytes=sizes[which], workspace=work)
            torch.cuda.synchronize()
            times = []
            for _ in range(args.windows):
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                for i in range(args.calls):
                    kb.ops.pack_frames(sets[i % 4][which], out=outs[which], out_bytes=sizes[which], workspace=work)
                end.record()
                end.synchronize()
                times.append(start.elapsed_time(end) * 1e3 / args.calls)
            result[f"{content}_{'rgb8' if which == 0 else 'planes16'}"] = {
                "us_per_call": [min(times), statistics.median(times), max(times)], "encoded_bytes_per_frame": float(sizes[which].double().mean()),
                "sample_bytes_per_frame": H * W * (3 if which == 0 else 2)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
