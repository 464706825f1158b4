#!/usr/bin/env python3
"""The training input pipeline on the GPU box: does a loader keep the training step fed?

    python tools/train_loader_bench.py [--out FILE] [--quick]

Writes 64 KITTI-sized samples into a temporary directory with PIL -- RGB triplets of 3726 x 375 mixed with 3672 x 370 (a smooth
scene plus sensor noise: compresses like a photograph), 16-bit sparse depth with about 5 % positive points, intrinsics -- and
reports, for batches of 8 cropped to 320 x 768 with the KITTI script's crop type (horizontal vertical anchored bottom):

1. Loader throughput, triplets/s: (a) kb.loader.TrainingFrameLoader(workers=8) against (b) the reference's algorithm restated
   here (PIL decode -> float32 -> split -> NumPy crop in `datasets.KBNetTrainingDataset`'s order, under
   torch.utils.data.DataLoader(num_workers=8, batch_size=8, shuffle=True), then `.to(device)` of the five tensors, reference
   src/kbnet.py:134-144, 392-397).  Both on the same host CPUs.  A host clock around whole epochs that end in a device
   synchronise, after a warm epoch (page cache, pinned staging, worker start-up); the median epoch with the smallest and largest.
   The (b) workers are separate processes started BEFORE this process touches the GPU, and they never touch it.
2. Kernel time: the device time of kbn_unpack_train_frames_forward alone on one batch's bytes (outputs preallocated, the entry
   point called directly, `iters` launches between two device events, the median of 5 windows after a warm-up) against the same
   four tensors computed by torch from the same device bytes (slice, permute, .float(), / 256; the same windows).  The calls rotate
   through 8 output sets (94 MB each) and 4 input sets, more than the 256 MiB last-level cache holds.  Bytes per output pixel:
   3 C + 2 read, 40 written.  The two results are compared bit for bit first.
3. Bytes that cross PCIe per batch for both loaders, from the shapes.

With --packed the files are first converted to packed frames (kb.loader.pack_frames) and both total sizes are printed;
the run then compares, in this one process and on this one GPU, TrainingFrameLoader over the packed files with the same loader
over the PNG files at 2 and at 8 workers (part 1, the reference-style DataLoader is left out), kbn_unpack_packed_frames_forward
with kbn_unpack_train_frames_forward on the same batch (part 2, results compared bit for bit first), and the host time of
kbn_frame_check with the inflate it stands in for (one thread, per triplet with its depth map).  The files are synthetic.

With --sequences two synthetic sequences, one of each raw size, are written frame by frame -- every frame once -- and,
from the same frames, the triplet files np.concatenate([previous, current, next], axis=1) of every sample (window 1), both as PNG and
as packed frames.  In this one process and on this one GPU the run reports the bytes on disk both ways, TrainingFrameLoader over the
triplet files beside the same loader over sequence entries (PNG and packed, 2 and 8 workers: three opens a sample against one, but a
third of the bytes), and the four launches -- kbn_unpack_train_frames_forward, kbn_unpack_sequence_frames_forward,
kbn_unpack_packed_frames_forward, kbn_unpack_packed_sequence_frames_forward -- on one batch, results compared bit for bit first.

One GPU process; nothing is retried."""
import argparse
import os
import shutil
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

import kbnet_amd as kb  # noqa: E402

N_FILES, BATCH, SHAPE, WORKERS = 64, 8, (320, 768), 8
CROP_TYPE = ["horizontal", "vertical", "anchored", "bottom"]     # bash/kitti/train_kbnet_kitti.sh
RAW_SIZES = [(375, 1242), (370, 1224)]
STEP_MS = 42.7                                                    # the training step at 8 x 320 x 768, DESIGN.md section 8i


def write_sample(args):
    d, i = args
    h, w = RAW_SIZES[i % 2]
    g = np.random.Generator(np.random.Philox(100 + i))
    yy, xx = np.mgrid[0:h, 0:3 * w]
    base = 128 + 60 * np.sin(xx / 90.0 + i) * np.cos(yy / 40.0) + 30 * np.sin((xx + yy) / 17.0)
    rgb = np.stack([base + g.normal(0, 6, base.shape) + 20 * c for c in range(3)], axis=-1).clip(0, 255).astype(np.uint8)
    Image.fromarray(rgb).save(os.path.join(d, f"im{i}.png"), compress_level=6)
    z = (g.random((h, w)) < 0.05) * (g.random((h, w)) * 79 + 1) * 256
    Image.fromarray(z.astype(np.uint16)).save(os.path.join(d, f"sd{i}.png"))
    np.save(os.path.join(d, f"k{i}.npy"), np.array([[721.5, 0, 609.6], [0, 721.5, 172.9], [0, 0, 1]]))


class ReferenceStyleDataset(torch.utils.data.Dataset):
    """The reference's KBNetTrainingDataset.__getitem__ (src/datasets.py:199-225) restated: PIL, float32, split, NumPy crop."""

    def __init__(self, images, depths, ks, shape, crop_type):
        self.images, self.depths, self.ks, self.shape, self.crop_type = images, depths, ks, shape, crop_type

    def __len__(self):
        return len(self.images)

    def __getitem__(self, i):
        triplet = np.transpose(np.asarray(Image.open(self.images[i]).convert("RGB"), np.float32), (2, 0, 1))
        image1, image0, image2 = np.split(triplet, indices_or_sections=3, axis=-1)
        z = np.array(Image.open(self.depths[i]), dtype=np.float32) / 256.0
        z[z <= 0] = 0.0
        z = np.expand_dims(z, axis=0)
        k = np.load(self.ks[i]).astype(np.float32)
        [image0, image1, image2, z], k = kb.loader.random_crop([image0, image1, image2, z], self.shape, intrinsics=k, crop_type=self.crop_type)
        return [T.astype(np.float32) for T in (image0, image1, image2, z, k)]


class _Done(Exception):
    """--packed or --sequences has written its lines: the default parts are not run."""


def epochs(run_epoch, count):
    """Triplets/s of `count` epochs, each timed on its own, after one warm epoch."""
    run_epoch()
    rates = []
    for _ in range(count):
        t = time.perf_counter()
        n = run_epoch()
        rates.append(n / (time.perf_counter() - t))
    return rates


def spread(values, fmt="{:.1f}"):
    return f"{fmt.format(statistics.median(values))} (min {fmt.format(min(values))}, max {fmt.format(max(values))})"


def windows(fn, iters, count=5):
    """Device ms a call: `count` windows of `iters` calls between two device events, after a warm-up of 16 calls."""
    for i in range(16):
        fn(i)
    torch.cuda.synchronize()
    out = []
    for _ in range(count):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(iters):
            fn(i)
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return out


def kernel_part(dev, images, depths, quick):
    """One batch's decoded bytes on the device: the unpack launch alone against torch ops."""
    lib = kb._lib.load()
    files = [open(p, "rb").read() for p in images[:BATCH] + depths[:BATCH]]
    raw = [kb.loader.decode_png(f) for f in files]
    frames, img_at, dep_at = [], 0, 0
    np.random.seed(0)
    for im, z in zip(raw[:BATCH], raw[BATCH:]):
        y, x = kb.loader.draw_crop(z.shape[0], z.shape[1], SHAPE, CROP_TYPE)
        frames.append((img_at, dep_at, z.shape[0], z.shape[1], y, x))
        img_at, dep_at = (img_at + im.nbytes + 15) & ~15, (dep_at + z.nbytes + 15) & ~15
    img_host, dep_host = np.zeros(img_at, np.uint8), np.zeros(dep_at, np.uint8)
    for f, im, z in zip(frames, raw[:BATCH], raw[BATCH:]):
        img_host[f[0]:f[0] + im.nbytes] = im.reshape(-1)
        dep_host[f[1]:f[1] + z.nbytes] = z.reshape(-1).view(np.uint8)
    n_in, n_out = (2, 2) if quick else (4, 8)
    ins = [(torch.from_numpy(img_host).to(dev), torch.from_numpy(dep_host).to(dev)) for _ in range(n_in)]
    h, w = SHAPE
    outs = [[torch.empty((BATCH, c, h, w), device=dev) for c in (3, 3, 3, 1)] for _ in range(n_out)]
    table = (kb._lib.TrainFrame * BATCH)()
    for slot, (io, do, H, W, y, x) in zip(table, frames):
        slot.image_offset, slot.depth_offset, slot.height, slot.raw_width, slot.y_start, slot.x_start = io, do, H, 3 * W, y, x
    stream = torch.cuda.current_stream().cuda_stream

    def ours(i):
        (im, z), o = ins[i % n_in], outs[i % n_out]
        rc = lib.kbn_unpack_train_frames_forward(im.data_ptr(), im.numel(), z.data_ptr(), z.numel(), table, BATCH, h, w, 3, 16,
                                                 o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), stream)
        assert rc == 0, rc

    def torch_ops(i):
        (im, z), o = ins[i % n_in], outs[i % n_out]
        for n, (io, do, H, W, y, x) in enumerate(frames):
            triplet = im[io:io + H * 3 * W * 3].view(H, 3 * W, 3)
            for out, third in zip(o[:3], (1, 0, 2)):
                out[n] = triplet[y:y + h, third * W + x:third * W + x + w].permute(2, 0, 1).float()
            o[3][n, 0] = z[do:do + H * W * 2].view(torch.int16).view(H, W)[y:y + h, x:x + w].float() / 256.0      # (the samples are below 2^15)

    ours(0)
    mine = [t.clone() for t in outs[0]]
    torch_ops(0)
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(mine, outs[0])), "the two computations differ"
    t_ours = windows(ours, 20 if quick else 400)
    t_torch = windows(torch_ops, 5 if quick else 50)
    pixels = BATCH * h * w
    moved = pixels * (3 * 3 + 2 + 40)
    us = statistics.median(t_ours) * 1e3
    return [f"2. kernel: one batch, {BATCH} frames of {RAW_SIZES[0][0]} x {RAW_SIZES[0][1]} / {RAW_SIZES[1][0]} x {RAW_SIZES[1][1]} -> {h} x {w}; results equal bit for bit",
            f"   kbn_unpack_train_frames_forward   device {spread([t * 1e3 for t in t_ours])} us a launch; 11 B read + 40 B written a pixel = "
            f"{moved / 1e6:.1f} MB -> {moved / (us * 1e-6) / 1e12:.2f} TB/s",
            f"   torch ops on the same bytes       device {spread([t * 1e3 for t in t_torch])} us a batch ({4 * BATCH} slice-permute-convert copies and "
            f"{BATCH} divisions; event window, launch gaps included)",
            f"   torch / kernel = {statistics.median(t_torch) / statistics.median(t_ours):.1f} x"], frames


def packed_kernel_part(dev, images, depths, packed_images, packed_depths, frames, quick):
    """The packed decoder on one batch's files against the raw-byte kernel on the same batch's decoded bytes: same crops, same
    event windows, the same rotation through output sets."""
    lib = kb._lib.load()
    h, w = SHAPE
    raw = [kb.loader.decode_png(open(p, "rb").read()) for p in images[:BATCH] + depths[:BATCH]]
    img_host, dep_host = np.zeros(frames[-1][0] + raw[BATCH - 1].nbytes, np.uint8), np.zeros(frames[-1][1] + raw[-1].nbytes, np.uint8)
    for f, im, z in zip(frames, raw[:BATCH], raw[BATCH:]):
        img_host[f[0]:f[0] + im.nbytes] = im.reshape(-1)
        dep_host[f[1]:f[1] + z.nbytes] = z.reshape(-1).view(np.uint8)
    files = [open(p, "rb").read() for p in packed_images[:BATCH] + packed_depths[:BATCH]]
    for data in files:
        kb.loader.check_frame(data)
    at, total = [], [0, 0]
    for j, data in enumerate(files):
        which = 0 if j < BATCH else 1
        at.append(total[which])
        total[which] = (total[which] + len(data) + 15) & ~15
    hosts = [np.zeros(total[0], np.uint8), np.zeros(total[1], np.uint8)]
    for j, data in enumerate(files):
        hosts[0 if j < BATCH else 1][at[j]:at[j] + len(data)] = np.frombuffer(data, np.uint8)
    n_in, n_out = (2, 2) if quick else (4, 8)
    raw_ins = [(torch.from_numpy(img_host).to(dev), torch.from_numpy(dep_host).to(dev)) for _ in range(n_in)]
    ins = [(torch.from_numpy(hosts[0]).to(dev), torch.from_numpy(hosts[1]).to(dev)) for _ in range(n_in)]
    outs = [[torch.empty((BATCH, c, h, w), device=dev) for c in (3, 3, 3, 1)] for _ in range(n_out)]
    table, raw_table = (kb._lib.PackedFrame * BATCH)(), (kb._lib.TrainFrame * BATCH)()
    for j, (slot, raw_slot, (io, do, H, W, y, x)) in enumerate(zip(table, raw_table, frames)):
        slot.image_offset, slot.depth_offset, slot.image_bytes, slot.depth_bytes = at[j], at[BATCH + j], len(files[j]), len(files[BATCH + j])
        slot.height, slot.raw_width, slot.y_start, slot.x_start = H, 3 * W, y, x
        raw_slot.image_offset, raw_slot.depth_offset, raw_slot.height, raw_slot.raw_width, raw_slot.y_start, raw_slot.x_start = io, do, H, 3 * W, y, x
    stream = torch.cuda.current_stream().cuda_stream

    def packed(i):
        (im, z), o = ins[i % n_in], outs[i % n_out]
        rc = lib.kbn_unpack_packed_frames_forward(im.data_ptr(), im.numel(), z.data_ptr(), z.numel(), table, BATCH, h, w, 3, 16,
                                                  o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), stream)
        assert rc == 0, rc

    def plain(i):
        (im, z), o = raw_ins[i % n_in], outs[i % n_out]
        rc = lib.kbn_unpack_train_frames_forward(im.data_ptr(), im.numel(), z.data_ptr(), z.numel(), raw_table, BATCH, h, w, 3, 16,
                                                 o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), stream)
        assert rc == 0, rc

    packed(0)
    mine = [t.clone() for t in outs[0]]
    plain(0)
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(mine, outs[0])), "the two kernels differ"
    iters = 20 if quick else 400
    t_plain = windows(plain, iters)
    t_packed = windows(packed, iters)
    t_plain_again = windows(plain, iters)
    us = lambda t: spread([v * 1e3 for v in t])
    ratio = statistics.median(t_packed) / statistics.median(t_plain + t_plain_again)
    step_share = statistics.median(t_packed) / STEP_MS * 100
    return [f"2. kernels: one batch, {BATCH} frames -> {h} x {w}; results equal bit for bit; packed input {(total[0] + total[1]) / 1e6:.1f} MB, raw input "
            f"{(img_host.nbytes + dep_host.nbytes) / 1e6:.1f} MB, output {BATCH * h * w * 40 / 1e6:.1f} MB",
            f"   kbn_unpack_train_frames_forward    device {us(t_plain)} us a launch (before), {us(t_plain_again)} us (after)",
            f"   kbn_unpack_packed_frames_forward   device {us(t_packed)} us a launch",
            f"   packed / raw-byte = {ratio:.2f} x; the packed launch is {step_share:.3f} % of the {STEP_MS} ms step"]


def host_check_part(images, depths, packed_images, packed_depths):
    """One thread: kbn_frame_check of a packed triplet and its depth map against the inflate (kbn_png_decode) of the PNG pair."""
    lib = kb._lib.load()
    n = min(16, len(images))
    packed = [open(p, "rb").read() for p in packed_images[:n] + packed_depths[:n]]
    pngs = [open(p, "rb").read() for p in images[:n] + depths[:n]]
    outs = [np.empty_like(kb.loader.decode_png(f)) for f in pngs]
    check_ms, inflate_ms = [], []
    for _ in range(5):
        t = time.perf_counter()
        for data in packed:
            assert lib.kbn_frame_check(data, len(data)) == 0
        check_ms.append((time.perf_counter() - t) / n * 1e3)
        t = time.perf_counter()
        for data, out in zip(pngs, outs):
            kb.loader.decode_png(data, out)
        inflate_ms.append((time.perf_counter() - t) / n * 1e3)
    return [f"4. host, one thread, per triplet with its depth map: kbn_frame_check {spread(check_ms, '{:.3f}')} ms; kbn_png_decode (inflate + filters) "
            f"{spread(inflate_ms, '{:.2f}')} ms; inflate / check = {statistics.median(inflate_ms) / statistics.median(check_ms):.0f} x"]


def packed_run(args, d, images, depths, ks, lines):
    """--packed: sizes, loader rates packed against PNG at 2 and 8 workers, the two kernels, the host check."""
    packed_images = [os.path.join(d, "packed", f"im{i}.kbf") for i in range(len(images))]
    packed_depths = [os.path.join(d, "packed", f"sd{i}.kbf") for i in range(len(images))]
    png_bytes, packed_bytes = kb.loader.pack_frames(images + depths, packed_images + packed_depths, workers=WORKERS)
    raw_bytes = sum(RAW_SIZES[i % 2][0] * RAW_SIZES[i % 2][1] * (9 + 2) for i in range(len(images)))
    lines.append(f"0. sizes of the {len(images)} SYNTHETIC samples (no real KITTI frame has been measured): PNG {png_bytes / 1e6:.1f} MB, packed {packed_bytes / 1e6:.1f} MB, "
                 f"raw {raw_bytes / 1e6:.1f} MB; packed / PNG = {packed_bytes / png_bytes:.3f}, packed / raw = {packed_bytes / raw_bytes:.3f}, "
                 f"PNG / raw = {png_bytes / raw_bytes:.3f}")
    if not torch.cuda.is_available():
        raise SystemExit("train_loader_bench needs a GPU: a time measured anywhere else says nothing")
    dev = torch.device("cuda:0")
    kb._lib.load()
    lines[0] += f"; {torch.cuda.get_device_name(0)}"
    need = BATCH / (STEP_MS * 1e-3)
    lines.append(f"1. TrainingFrameLoader, triplets/s, median (min, max) of the epoch windows (the {STEP_MS} ms step takes {need:.0f} a GPU):")
    medians = {}
    for workers in (2, 8):
        for name, im, de in (("PNG", images, depths), ("packed", packed_images, packed_depths)):
            loader = kb.loader.TrainingFrameLoader(im, de, ks, shape=SHAPE, random_crop_type=CROP_TYPE, batch_size=BATCH, shuffle=True, device=dev,
                                                   workers=workers, prefetch=4)

            def epoch():
                n = 0
                for _ in range(4):
                    for inputs in loader:
                        n += inputs[0].shape[0]
                torch.cuda.synchronize()
                return n

            rates = epochs(epoch, 2 if args.quick else 8)
            medians[(name, workers)] = statistics.median(rates)
            lines.append(f"   {name:6} workers={workers}   {spread(rates)}")
    lines.append(f"   packed / PNG at 8 workers = {medians[('packed', 8)] / medians[('PNG', 8)]:.2f}; at 2 workers = {medians[('packed', 2)] / medians[('PNG', 2)]:.2f}; "
                 f"packed at 2 workers / PNG at 8 workers = {medians[('packed', 2)] / medians[('PNG', 8)]:.2f}")
    np.random.seed(0)
    frames, img_at, dep_at = [], 0, 0
    for i in range(BATCH):
        H, W = RAW_SIZES[i % 2]
        y, x = kb.loader.draw_crop(H, W, SHAPE, CROP_TYPE)
        frames.append((img_at, dep_at, H, W, y, x))
        img_at, dep_at = (img_at + H * 3 * W * 3 + 15) & ~15, (dep_at + H * W * 2 + 15) & ~15
    lines += packed_kernel_part(dev, images, depths, packed_images, packed_depths, frames, args.quick)
    packed_batch = sum(os.path.getsize(p) for p in packed_images[:BATCH] + packed_depths[:BATCH])
    raw_batch = sum(H * 3 * W * 3 + H * W * 2 for _, _, H, W, _, _ in frames)
    lines.append(f"3. PCIe bytes a batch: packed {packed_batch / 1e6:.1f} MB, raw bytes {raw_batch / 1e6:.1f} MB; packed / raw = {packed_batch / raw_batch:.2f}")
    lines += host_check_part(images, depths, packed_images, packed_depths)
    lines.append("5. multi-GPU effect: not measured (one GPU, one process).")


def _scene(h, w, s, t):
    """Frame t of sequence s: the default mode's smooth scene, drifting 7 columns a frame, plus sensor noise."""
    g = np.random.Generator(np.random.Philox(1000 * (s + 1) + t))
    yy, xx = np.mgrid[0:h, 0:w]
    base = 128 + 60 * np.sin((xx + 7 * t) / 90.0 + s) * np.cos(yy / 40.0) + 30 * np.sin((xx + yy + 3 * t) / 17.0)
    return np.stack([base + g.normal(0, 6, base.shape) + 20 * c for c in range(3)], axis=-1).clip(0, 255).astype(np.uint8)


def write_frame(args):
    d, s, t = args
    h, w = RAW_SIZES[s]
    os.makedirs(os.path.join(d, f"seq{s}"), exist_ok=True)
    Image.fromarray(_scene(h, w, s, t)).save(os.path.join(d, f"seq{s}", f"f{t:04d}.png"), compress_level=6)


def write_triplet_sample(args):
    """Sample (s, t): the triplet file of frames t, t + 1, t + 2 of sequence s, its sparse depth and its intrinsics."""
    d, s, t, fields = args
    h, w = RAW_SIZES[s]
    frames = [kb.loader.decode_png(open(path, "rb").read()) for path in fields]
    Image.fromarray(np.concatenate(frames, axis=1)).save(os.path.join(d, f"tr{s}_{t}.png"), compress_level=6)
    g = np.random.Generator(np.random.Philox(5000 * (s + 1) + t))
    z = (g.random((h, w)) < 0.05) * (g.random((h, w)) * 79 + 1) * 256
    Image.fromarray(z.astype(np.uint16)).save(os.path.join(d, f"sd{s}_{t}.png"))
    np.save(os.path.join(d, f"k{s}_{t}.npy"), np.array([[721.5, 0, 609.6], [0, 721.5, 172.9], [0, 0, 1]]))


def _to_packed(path):
    return os.path.splitext(path)[0] + ".kbf"


def sequence_batch(entries, triplets, depths, packed):
    """The first BATCH samples laid out for the four launches (host side, no GPU): {name: (image bytes, depth bytes, record
    table)} for "train", "sequence" (decoded bytes) and "packed", "packed_sequence" (files as they are on disk), under one set of
    crops.  Every distinct frame lies once in the sequence buffers."""
    h, w = SHAPE
    read = lambda path: open(path, "rb").read()
    load = (lambda path: read(_to_packed(path))) if packed else (lambda path: kb.loader.decode_png(read(path)).tobytes())

    def lay(blobs):
        at, total = [], 0
        for data in blobs:
            at.append(total)
            total = (total + len(data) + 15) & ~15
        host = np.zeros(total, np.uint8)
        for a, data in zip(at, blobs):
            host[a:a + len(data)] = np.frombuffer(data, np.uint8)
        return host, at

    fields = [kb.loader.split_sample(entry) for entry in entries[:BATCH]]
    distinct = list(dict.fromkeys(path for f in fields for path in f))
    frame_blobs, triplet_blobs, depth_blobs = [load(p) for p in distinct], [load(p) for p in triplets[:BATCH]], [load(p) for p in depths[:BATCH]]
    (frame_host, frame_at), (triplet_host, triplet_at), (depth_host, depth_at) = lay(frame_blobs), lay(triplet_blobs), lay(depth_blobs)
    where = {path: (a, len(data)) for path, a, data in zip(distinct, frame_at, frame_blobs)}
    np.random.seed(0)
    sizes = [kb.loader.png_info(read(f[1])[:33])[1::-1] for f in fields]      # (height, width) of `current`
    starts = [kb.loader.draw_crop(H, W, SHAPE, CROP_TYPE) for H, W in sizes]
    if packed:
        triplet_table, sequence_table = (kb._lib.PackedFrame * BATCH)(), (kb._lib.PackedSequenceFrame * BATCH)()
    else:
        triplet_table, sequence_table = (kb._lib.TrainFrame * BATCH)(), (kb._lib.SequenceFrame * BATCH)()
    for j, ((H, W), (y, x), f) in enumerate(zip(sizes, starts, fields)):
        a, b = triplet_table[j], sequence_table[j]
        a.image_offset, a.depth_offset, a.height, a.raw_width, a.y_start, a.x_start = triplet_at[j], depth_at[j], H, 3 * W, y, x
        b.depth_offset, b.height, b.width, b.y_start, b.x_start = depth_at[j], H, W, y, x
        for k, path in enumerate(f):
            b.image_offset[k] = where[path][0]
            if packed:
                b.image_bytes[k] = where[path][1]
        if packed:
            a.image_bytes, a.depth_bytes, b.depth_bytes = len(triplet_blobs[j]), len(depth_blobs[j]), len(depth_blobs[j])
    names = ("packed", "packed_sequence") if packed else ("train", "sequence")
    return {names[0]: (triplet_host, depth_host, triplet_table), names[1]: (frame_host, depth_host, sequence_table)}


def sequence_kernel_part(dev, entries, triplets, depths, quick):
    """The two new launches beside the two existing ones on one batch: the same crops, event windows and rotation through output
    sets; the four results are compared bit for bit first."""
    lib = kb._lib.load()
    h, w = SHAPE
    batches = {**sequence_batch(entries, triplets, depths, False), **sequence_batch(entries, triplets, depths, True)}
    n_in, n_out = (2, 2) if quick else (4, 8)
    outs = [[torch.empty((BATCH, c, h, w), device=dev) for c in (3, 3, 3, 1)] for _ in range(n_out)]
    stream = torch.cuda.current_stream().cuda_stream
    entry = {"train": lib.kbn_unpack_train_frames_forward, "sequence": lib.kbn_unpack_sequence_frames_forward,
             "packed": lib.kbn_unpack_packed_frames_forward, "packed_sequence": lib.kbn_unpack_packed_sequence_frames_forward}
    calls, nbytes = {}, {}
    for name, (image_host, depth_host, table) in batches.items():
        ins = [(torch.from_numpy(image_host).to(dev), torch.from_numpy(depth_host).to(dev)) for _ in range(n_in)]
        nbytes[name] = image_host.nbytes + depth_host.nbytes

        def call(i, ins=ins, table=table, fn=entry[name]):
            (im, z), o = ins[i % n_in], outs[i % n_out]
            rc = fn(im.data_ptr(), im.numel(), z.data_ptr(), z.numel(), table, BATCH, h, w, 3, 16, o[0].data_ptr(), o[1].data_ptr(),
                    o[2].data_ptr(), o[3].data_ptr(), stream)
            assert rc == 0, rc

        calls[name] = call
    results = {}
    for name, call in calls.items():
        for t in outs[0]:
            t.fill_(-1.0)
        call(0)
        torch.cuda.synchronize()
        results[name] = [t.clone() for t in outs[0]]
    for name in ("sequence", "packed", "packed_sequence"):
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(results["train"], results[name])), f"{name} differs"
    iters = 20 if quick else 400
    order = ("train", "sequence", "packed", "packed_sequence")
    first = {name: windows(calls[name], iters) for name in order}
    again = {name: windows(calls[name], iters) for name in order}
    us = lambda t: spread([v * 1e3 for v in t])
    lines = [f"2. kernels: one batch, {BATCH} samples -> {h} x {w}; the four results equal bit for bit; output {BATCH * h * w * 40 / 1e6:.1f} MB; "
             "two rounds of windows, each launch after the other three"]
    for name in order:
        lines.append(f"   kbn_unpack_{name}_frames_forward".ljust(48) + f"input {nbytes[name] / 1e6:5.1f} MB   device {us(first[name])} us a launch, "
                     f"{us(again[name])} us in the second round")
    med = lambda name: statistics.median(first[name] + again[name])
    lines.append(f"   sequence / train = {med('sequence') / med('train'):.2f} x; packed_sequence / packed = {med('packed_sequence') / med('packed'):.2f} x")
    return lines


def sequences_run(args, d, lines):
    """--sequences: bytes on disk, loader rates of the triplet path beside the sequence path, the four launches."""
    per = 8 if args.quick else N_FILES // 2      # samples a sequence
    frames = [[os.path.join(d, f"seq{s}", f"f{t:04d}.png") for t in range(per + 2)] for s in range(2)]
    samples = [(s, t) for t in range(per) for s in range(2)]      # the two sizes alternate, as in the default mode
    by_sequence = [kb.loader.sequence_lines(f, window=1, ends="drop") for f in frames]
    with ThreadPoolExecutor(max_workers=WORKERS) as ex:
        list(ex.map(write_frame, [(d, s, t) for s in range(2) for t in range(per + 2)]))
        list(ex.map(write_triplet_sample, [(d, s, t, kb.loader.split_sample(by_sequence[s][t])) for s, t in samples]))
    lists = {"PNG": {"sequence": [by_sequence[s][t] for s, t in samples], "triplet": [os.path.join(d, f"tr{s}_{t}.png") for s, t in samples],
                     "depth": [os.path.join(d, f"sd{s}_{t}.png") for s, t in samples]}}
    ks = [os.path.join(d, f"k{s}_{t}.npy") for s, t in samples]
    lists["packed"] = {name: [kb.loader.map_sample(entry, _to_packed) for entry in entries] for name, entries in lists["PNG"].items()}
    for name in ("sequence", "triplet", "depth"):      # sequence entries go through pack_frames as they are: every frame once
        kb.loader.pack_frames(lists["PNG"][name], lists["packed"][name], workers=WORKERS)
    size = lambda entries: sum(os.path.getsize(p) for p in dict.fromkeys(path for e in entries for path in (kb.loader.split_sample(e) or (e,))))
    disk = {(kind, form): size(lists[kind][form]) for kind in lists for form in ("sequence", "triplet")}
    lines[0] = (f"train_loader_bench --sequences: {len(samples)} SYNTHETIC samples (no real KITTI frame has been measured) of two sequences of {per + 2} frames, "
                f"batch {BATCH}, crop {SHAPE[0]} x {SHAPE[1]} {' '.join(CROP_TYPE)}")
    lines.append("0. image bytes on disk, triplet files | one file a frame: " + "; ".join(
        f"{kind} {disk[(kind, 'triplet')] / 1e6:.1f} MB | {disk[(kind, 'sequence')] / 1e6:.1f} MB ({disk[(kind, 'sequence')] / disk[(kind, 'triplet')]:.3f})"
        for kind in lists) + f"; {3 * len(samples)} frame slots in the triplets, {2 * (per + 2)} frames")
    if not torch.cuda.is_available():
        raise SystemExit("train_loader_bench needs a GPU: a time measured anywhere else says nothing")
    dev = torch.device("cuda:0")
    kb._lib.load()
    lines[0] += f"; {torch.cuda.get_device_name(0)}"
    need = BATCH / (STEP_MS * 1e-3)
    lines.append(f"1. TrainingFrameLoader, triplets/s, median (min, max) of the epoch windows (the {STEP_MS} ms step takes {need:.0f} a GPU):")
    medians = {}
    for workers in (2, 8):
        for kind in ("PNG", "packed"):
            for form in ("triplet", "sequence"):
                loader = kb.loader.TrainingFrameLoader(lists[kind][form], lists[kind]["depth"], ks, shape=SHAPE, random_crop_type=CROP_TYPE,
                                                       batch_size=BATCH, shuffle=True, device=dev, workers=workers, prefetch=4)

                def epoch():
                    n = 0
                    for _ in range(4):
                        for inputs in loader:
                            n += inputs[0].shape[0]
                    torch.cuda.synchronize()
                    return n

                rates = epochs(epoch, 2 if args.quick else 8)
                medians[(kind, form, workers)] = statistics.median(rates)
                lines.append(f"   {kind:6} {form:8} workers={workers}   {spread(rates)}")
    lines.append("   sequence / triplet: " + "; ".join(
        f"{kind} at {workers} workers {medians[(kind, 'sequence', workers)] / medians[(kind, 'triplet', workers)]:.2f}"
        for kind in ("PNG", "packed") for workers in (2, 8)))
    lines += sequence_kernel_part(dev, lists["PNG"]["sequence"], lists["PNG"]["triplet"], lists["PNG"]["depth"], args.quick)
    lines.append("3. multi-GPU effect: not measured (one GPU, one process).")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--packed", action="store_true", help="convert the files to packed frames and compare the packed path with the PNG path")
    ap.add_argument("--sequences", action="store_true", help="compare sequence entries (one file a frame) with the triplet files of the same frames")
    ap.add_argument("--quick", action="store_true", help="16 files, short windows: a rehearsal, not a measurement")
    args = ap.parse_args()
    n_files = 16 if args.quick else N_FILES
    d = tempfile.mkdtemp(prefix="kbn_train_loader_")
    try:
        if args.sequences:
            lines = [""]
            sequences_run(args, d, lines)
            raise _Done
        with ThreadPoolExecutor(max_workers=WORKERS) as ex:
            list(ex.map(write_sample, [(d, i) for i in range(n_files)]))
        images = [os.path.join(d, f"im{i}.png") for i in range(n_files)]
        depths = [os.path.join(d, f"sd{i}.png") for i in range(n_files)]
        ks = [os.path.join(d, f"k{i}.npy") for i in range(n_files)]
        mb = sum(os.path.getsize(p) for p in images + depths) / 1e6
        lines = [f"train_loader_bench: {n_files} samples, {mb / n_files:.2f} MB of PNG a sample, batch {BATCH}, crop {SHAPE[0]} x {SHAPE[1]} "
                 f"{' '.join(CROP_TYPE)}, {WORKERS} workers"]
        if args.packed:
            packed_run(args, d, images, depths, ks, lines)
            raise _Done
        # (b) first: its worker processes start, and run a whole epoch, before this process touches the GPU
        reference = torch.utils.data.DataLoader(ReferenceStyleDataset(images, depths, ks, SHAPE, CROP_TYPE), batch_size=BATCH, shuffle=True,
                                                num_workers=WORKERS, drop_last=False, persistent_workers=True, multiprocessing_context="spawn")
        for _ in reference:
            pass
        if not torch.cuda.is_available():
            raise SystemExit("train_loader_bench needs a GPU: a time measured anywhere else says nothing")
        dev = torch.device("cuda:0")
        kb._lib.load()
        lines[0] += f"; {torch.cuda.get_device_name(0)}"

        def reference_epoch():
            n = 0
            for inputs in reference:
                inputs = [in_.to(dev) for in_ in inputs]
                n += inputs[0].shape[0]
            torch.cuda.synchronize()
            return n

        rate_b = epochs(reference_epoch, 2 if args.quick else 4)
        del reference
        ours = kb.loader.TrainingFrameLoader(images, depths, ks, shape=SHAPE, random_crop_type=CROP_TYPE, batch_size=BATCH, shuffle=True,
                                             device=dev, workers=WORKERS, prefetch=4)

        def our_epoch():      # four epochs a window: one alone lasts some tens of milliseconds
            n = 0
            for _ in range(4):
                for inputs in ours:
                    n += inputs[0].shape[0]
            torch.cuda.synchronize()
            return n

        rate_a = epochs(our_epoch, 2 if args.quick else 8)
        need = BATCH / (STEP_MS * 1e-3)
        verdict = lambda r: "keeps up" if statistics.median(r) >= need else "STARVES the step"
        lines += [f"1. loader throughput, triplets/s (the {STEP_MS} ms step takes {need:.0f}):",
                  f"   (a) TrainingFrameLoader              {spread(rate_a)}   {verdict(rate_a)}",
                  f"   (b) PIL + NumPy under DataLoader     {spread(rate_b)}   {verdict(rate_b)}",
                  f"   (a) / (b) = {statistics.median(rate_a) / statistics.median(rate_b):.2f}"]
        part, frames = kernel_part(dev, images, depths, args.quick)
        lines += part
        ours_bytes = sum(H * 3 * W * 3 + H * W * 2 for _, _, H, W, _, _ in frames) + BATCH * 36
        ref_bytes = BATCH * (10 * SHAPE[0] * SHAPE[1] * 4 + 36)
        lines += [f"3. PCIe bytes a batch: (a) {ours_bytes / 1e6:.1f} MB (the raw uint8 triplets and uint16 depth, whole frames, + intrinsics)   "
                  f"(b) {ref_bytes / 1e6:.1f} MB (ten float32 planes of the crop a frame + intrinsics)   (a) / (b) = {ours_bytes / ref_bytes:.2f}"]
    except _Done:
        pass
    finally:
        shutil.rmtree(d, ignore_errors=True)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
