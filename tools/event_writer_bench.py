#!/usr/bin/env python3
"""Times a histogram of the training loop's monitoring on the GPU: (a) ops.histogram_tensorflow (csrc/histogram.hip, two launches
behind a memset) and EventWriter.add_histogram around it, against (b) what TensorBoard's writer does with the same device tensor on
the same box -- .cpu() (a wait for the device), astype(float), np.histogram over the 1549 'tensorflow' edges, min, max, sum, dot.

    python tools/event_writer_bench.py [--out FILE] [--quick]

Shape: the training bench's output depth, 8 x 1 x 320 x 768 (7.9 MB), dense values in [1.5, 100), and the sparse depth of the same
shape (5 % of the pixels set, runs of zeros between them).

Method (tools/summary_bench.py's): after a warm-up, 5 windows of `iters` calls between two device events; per call the median
window with the smallest and the largest.  Host time of (a): a host clock around the same loop without a trailing synchronise --
what the training loop loses to the call.  (b) waits for the device in .cpu(), so its wall time is what the training loop loses.
The inputs rotate through 4 sets."""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import kbnet_amd as kb  # noqa: E402

N, H, W = 8, 320, 768
SETS = 4


def make_inputs(dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    output = 1.5 + 98.5 * torch.rand(N, 1, H, W, generator=g, device=dev)
    sparse = output * (torch.rand(N, 1, H, W, generator=g, device=dev) < 0.05).float()
    return {"output": output, "sparse": sparse}


def theirs(t, edges):
    """make_np, astype(float) and make_histogram's NumPy calls."""
    values = t.detach().cpu().numpy().astype(float).reshape(-1)
    counts, _ = np.histogram(values, bins=edges)
    return counts, values.min(), values.max(), values.sum(), values.dot(values)


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
        raise SystemExit("event_writer_bench needs a GPU: a time measured anywhere else says nothing")
    dev = torch.device("cuda:0")
    kb._lib.load()
    edges = np.asarray(kb.ops.histogram_edges())
    sets = [make_inputs(dev, 100 + i) for i in range(2 if args.quick else SETS)]
    lines = [f"event_writer_bench on {torch.cuda.get_device_name(0)}: {N} x 1 x {H} x {W} float32, {4 * N * H * W / 1e6:.1f} MB a tensor"]
    iters = 5 if args.quick else 100
    with tempfile.TemporaryDirectory() as tmp, kb.summary.EventWriter(tmp) as writer:
        for key in ("output", "sparse"):
            counts, _ = kb.ops.histogram_tensorflow(sets[0][key])
            want = theirs(sets[0][key], edges)
            packed = counts._base.cpu().numpy()
            same = np.array_equal(packed[:1548], want[0]) and tuple(packed[1548:].view(np.float64)[:2]) == (want[1], want[2])
            dev_k, host_k = windows(lambda s: kb.ops.histogram_tensorflow(s[key]), sets, iters)
            dev_w, host_w = windows(lambda s: writer.add_histogram("bench_" + key, s[key], 1), sets, iters)
            writer.flush()
            dev_b, host_b = windows(lambda s: theirs(s[key], edges), sets, 1 if args.quick else 3, count=3 if args.quick else 5)
            k_ms = statistics.median(dev_k)
            lines += [f"  {key} depth: counts, min and max equal to NumPy's: {same}",
                      f"    (a) ops.histogram_tensorflow        device {spread(dev_k)}   {4.0 * N * H * W / (k_ms * 1e-3) / 1e12:.2f} TB/s   "
                      f"host, no trailing synchronise {spread(host_k)}",
                      f"        EventWriter.add_histogram       device {spread(dev_w)}   host, no trailing synchronise {spread(host_w)}",
                      f"    (b) .cpu() + np.histogram + sums    wall   {spread(host_b, 'ms', 1.0)}",
                      f"    host time lost a call: (b) {statistics.median(host_b):.1f} ms, (a) {statistics.median(host_w) * 1e3:.1f} us"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
