#!/usr/bin/env python3
"""Times PoseNetModel.forward (HIP: csrc/posenet.hip) against the same network as torch-ROCm ops on the device (F.conv2d, the
eval-mode affine, leaky_relu, the 1 x 1 conv, mean, ops.pose_matrix), in one process, alternating the two, for KITTI pairs
(352 x 1216).  Device events around every repetition, warm-up first, medians reported; one JSON line per batch size.

    python tools/posenet_bench.py [--encoder posenet|resnet18|resnet34] [--batches 32 1] [--reps 30] [--warmup 5] [--layers]

--encoder resnet18 / resnet34: ResNetPoseNetModel.forward (csrc/conv_affine.hip) against the F.conv2d / F.max_pool2d chain of the
same network; --layers then times conv1, the pool, each block's conv1, conv2 (with the add and the second activation) and
projection, the decoder's convs and the head.
--layers: also the median of every layer alone (both sides), which says where a difference comes from.  ALGORITHMIC FLOPs are
counted from the shapes (2 N OH OW C k k F per conv); the rate is a whole-forward figure, not a kernel's share of peak.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kbnet_amd as kb  # noqa: E402

KERNELS = (7, 5, 3, 3, 3, 3, 3)


def torch_layer(x, w, scale, shift, k):
    return F.leaky_relu(F.conv2d(x, w, None, stride=2, padding=k // 2) * scale + shift, 0.20)


def torch_forward(image0, image1, weights, affines, w_dec):
    x = torch.cat([image0, image1], dim=1)
    for w, (scale, shift), k in zip(weights, affines, KERNELS):
        x = torch_layer(x, w, scale, shift, k)
    return kb.ops.pose_matrix(0.01 * F.conv2d(x, w_dec).mean(dim=(2, 3)))


def timed(fns, reps, warmup):
    """Median milliseconds of each callable, the callables alternating inside every repetition."""
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            times[i].append(a.elapsed_time(b))
    return [statistics.median(t) for t in times], [(min(t), max(t)) for t in times]


def flops(n, h, w, filters):
    total, cin = 0.0, 6
    for f, k in zip(filters, KERNELS):
        h, w = (h + 1) // 2, (w + 1) // 2
        total += 2.0 * n * h * w * cin * k * k * f
        cin = f
    return total + 2.0 * n * h * w * cin * 6


# ---- the ResNet pose networks: every conv as (name, module, stride, what it reads, what it adds) ---------------------------
def torch_affine_conv(x, layer, residual=None):
    """One ResNetConv2d as torch ops: conv, the eval-mode affine, the activation, and with `residual` the add and the second one."""
    y = F.conv2d(x, layer.conv.weight, None, stride=layer.stride, padding=layer.kernel_size // 2)
    if hasattr(layer, "batch_norm"):
        scale, shift = layer.affine()
        y = y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    if layer.slope is not None:
        y = F.leaky_relu(y, layer.slope)
    if residual is not None:
        y = y + residual
        if layer.slope is not None:
            y = F.leaky_relu(y, layer.slope)
    return y


def torch_resnet_forward(model, image0, image1):
    x = torch_affine_conv(torch.cat([image0, image1], dim=1), model.encoder.conv1)
    x = F.max_pool2d(x, 3, stride=2, padding=1)
    for block in model.encoder.blocks():
        h = torch_affine_conv(x, block.conv1)
        skip = torch_affine_conv(x, block.projection) if block.projects(x) else x
        x = torch_affine_conv(h, block.conv2, residual=skip)
    for layer in model.decoder.hidden():
        x = torch_affine_conv(x, layer)
    return kb.ops.pose_matrix(0.01 * F.conv2d(x, model.decoder.conv[-1].conv.weight).mean(dim=(2, 3)))


def resnet_flops(model, n, h, w):
    def conv(layer, h, w):
        oh, ow = -(-h // layer.stride), -(-w // layer.stride)
        return 2.0 * n * oh * ow * layer.in_channels * layer.kernel_size ** 2 * layer.out_channels, oh, ow
    total, h, w = conv(model.encoder.conv1, h, w)
    h, w = (h + 1) // 2, (w + 1) // 2
    for block in model.encoder.blocks():
        if block.stride != 1 or block.in_channels != block.out_channels:
            total += conv(block.projection, h, w)[0]
        f, h, w = conv(block.conv1, h, w)
        total += f + conv(block.conv2, h, w)[0]
    for layer in model.decoder.hidden():
        f, h, w = conv(layer, h, w)
        total += f
    return total + 2.0 * n * h * w * model.decoder.conv[-1].conv.weight.shape[1] * 6


def resnet_layers(model, i0, i1, reps, warmup):
    """Median milliseconds of every launch alone, HIP and torch alternating, on the tensors a forward hands it."""
    per = []

    def one(name, hip, ref):
        (a, b), _ = timed([hip, ref], reps, warmup)
        per.append({"layer": name, "hip_ms": round(a, 4), "torch_ms": round(b, 4)})

    cat = torch.cat([i0, i1], dim=1)
    enc, dec = model.encoder, model.decoder
    x = enc.conv1.run([i0, i1])
    one("conv1 7x7 s2", lambda: enc.conv1.run([i0, i1]), lambda: torch_affine_conv(cat, enc.conv1))
    one("pool", lambda: kb.ops.maxpool3x3s2(x), lambda: F.max_pool2d(x, 3, stride=2, padding=1))
    x = kb.ops.maxpool3x3s2(x)
    for name, block in [(f"{s}.{b}", blk) for s in enc.stages for b, blk in enumerate(getattr(enc, s))]:
        shape = f"{block.in_channels}->{block.out_channels} @{x.shape[2]}x{x.shape[3]}"
        h = block.conv1.run([x])
        one(f"{name}.conv1 3x3 s{block.stride} {shape}", lambda: block.conv1.run([x]), lambda: torch_affine_conv(x, block.conv1))
        skip = x
        if block.projects(x):
            skip = block.projection.run([x])
            one(f"{name}.projection 1x1 s{block.stride}", lambda: block.projection.run([x]), lambda: torch_affine_conv(x, block.projection))
        one(f"{name}.conv2 3x3 s1 +skip", lambda: block.conv2.run([h], residual=skip), lambda: torch_affine_conv(h, block.conv2, residual=skip))
        x = block.conv2.run([h], residual=skip)
    for i, layer in enumerate(dec.hidden()):
        one(f"decoder.{i} 3x3 s2", lambda: layer.run([x]), lambda: torch_affine_conv(x, layer))
        x = layer.run([x])
    w_dec = dec.conv[-1].conv.weight
    one("head", lambda: kb.ops.pose_head(x, w_dec), lambda: kb.ops.pose_matrix(0.01 * F.conv2d(x, w_dec).mean(dim=(2, 3))))
    return per


def main_resnet(args, dev):
    n_layer = int(args.encoder[6:])
    enc, dec = kb.synthetic.make_resnet_pose_weights(n_layer, seed=5)
    model = kb.modules.ResNetPoseNetModel(n_layer, device=dev)
    model.load_state_dicts(enc, dec)
    with torch.no_grad():
        for n in args.batches:
            i0, i1 = [t.to(dev) for t in kb.synthetic.make_image_pair(1, args.height, args.width, seed=7)]
            i0, i1 = i0.repeat(n, 1, 1, 1).contiguous(), i1.repeat(n, 1, 1, 1).contiguous()
            hip = lambda: model.forward(i0, i1)
            ref = lambda: torch_resnet_forward(model, i0, i1)
            diff = float((hip() - ref()).abs().max())
            (t_hip, t_ref), spread = timed([hip, ref], args.reps, args.warmup)
            gflop = resnet_flops(model, n, args.height, args.width) / 1e9
            out = {"encoder": args.encoder, "batch": n, "height": args.height, "width": args.width, "hip_ms": round(t_hip, 4),
                   "torch_ms": round(t_ref, 4), "hip_over_torch": round(t_hip / t_ref, 3),
                   "hip_min_max_ms": [round(v, 4) for v in spread[0]], "torch_min_max_ms": [round(v, 4) for v in spread[1]],
                   "algorithmic_gflop": round(gflop, 3), "hip_tflops": round(gflop / t_hip, 2), "max_abs_pose_difference": diff,
                   "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
            if args.layers:
                out["layers"] = resnet_layers(model, i0, i1, args.reps, args.warmup)
            print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--encoder", choices=["posenet", "resnet18", "resnet34"], default="posenet")
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 1])
    ap.add_argument("--height", type=int, default=352)
    ap.add_argument("--width", type=int, default=1216)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--layers", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("posenet_bench needs a GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    torch.backends.cudnn.benchmark = True          # let MIOpen pick its fastest convs: the fair torch side
    if args.encoder != "posenet":
        return main_resnet(args, dev)
    enc, dec = kb.synthetic.make_posenet_weights(seed=5)
    model = kb.modules.PoseNetModel(device=dev)
    model.load_state_dicts(enc, dec)
    layers = model.encoder.layers()
    weights = [l.conv.weight.detach() for l in layers]
    affines = [tuple(t.view(1, -1, 1, 1) for t in l.affine()) for l in layers]
    w_dec = model.decoder.conv.conv.weight.detach()
    filters = [w.shape[0] for w in weights]
    with torch.no_grad():
        for n in args.batches:
            i0, i1 = [t.to(dev) for t in kb.synthetic.make_image_pair(1, args.height, args.width, seed=7)]
            i0, i1 = i0.repeat(n, 1, 1, 1).contiguous(), i1.repeat(n, 1, 1, 1).contiguous()
            hip = lambda: model.forward(i0, i1)
            ref = lambda: torch_forward(i0, i1, weights, affines, w_dec)
            diff = float((hip() - ref()).abs().max())
            (t_hip, t_ref), spread = timed([hip, ref], args.reps, args.warmup)
            out = {"batch": n, "height": args.height, "width": args.width, "hip_ms": round(t_hip, 4), "torch_ms": round(t_ref, 4),
                   "hip_over_torch": round(t_hip / t_ref, 3), "hip_min_max_ms": [round(v, 4) for v in spread[0]],
                   "torch_min_max_ms": [round(v, 4) for v in spread[1]], "algorithmic_gflop": round(flops(n, args.height, args.width, filters) / 1e9, 3),
                   "hip_tflops": round(flops(n, args.height, args.width, filters) / t_hip / 1e9, 2), "max_abs_pose_difference": diff,
                   "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
            if args.layers:
                acts = model.encoder.encode([i0, i1], return_layers=True)
                xs = [[i0, i1]] + [[a] for a in acts[:-1]]
                cat = torch.cat([i0, i1], dim=1)
                per = []
                for j, layer in enumerate(layers):
                    tx = cat if j == 0 else acts[j - 1]
                    (a, b), _ = timed([lambda: layer.run(xs[j]), lambda: torch_layer(tx, weights[j], *affines[j], KERNELS[j])],
                                      args.reps, args.warmup)
                    per.append({"layer": j + 1, "hip_ms": round(a, 4), "torch_ms": round(b, 4)})
                (a, b), _ = timed([lambda: model.decoder(acts[-1]),
                                   lambda: kb.ops.pose_matrix(0.01 * F.conv2d(acts[-1], w_dec).mean(dim=(2, 3)))], args.reps, args.warmup)
                per.append({"layer": "head", "hip_ms": round(a, 4), "torch_ms": round(b, 4)})
                out["layers"] = per
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
