#!/usr/bin/env python3
"""Times kb.inference.run and its export on the GPU, at KITTI size (352 x 1216, batch 8):

  (a) frames/s of run() with save_outputs off and on (wall clock around the call: it ends with every file written);
  (b) the comparator for the export, written here: the reference's own algorithm over the same loader, preprocess and forward --
      per frame .cpu().numpy() of the normalised image, the output depth and the filtered sparse depth, kept in lists as float32,
      every ground truth loaded before the loop, then PIL after the loop (src/kbnet.py:754-761, 924-930, 986-1026).  Without PIL
      (b) is "not measured";
  (c) the pack launch alone (kbn_export_pack_forward on 8 x 352 x 1216, all three sources) through device events, with its
      algorithmic bytes (20 in + 7 out a pixel) over its time.

  (d) with --packed: the packed export (output_format="packed") as a fourth kind in the same alternating rounds, the
      bytes it writes beside the PNG export's, and the two ops.pack_frames calls of a batch (8 x 352 x 1216 x 3 of 8 bits, then
      16 planes of 16 bits: six launches) through device events as in (c), on the pixels export_pack makes of smoothed sources;
      the same two run() kinds over PACKED copies of every input file (images, sparse depth, ground truth: no inflate left on the
      host), and loader.OutputWriter ALONE on resident tensors -- PNG and packed, with and without ground truth -- which says
      what the writer can take when nothing else wants the host's cores.

    python tools/run_export_bench.py [--out FILE] [--quick] [--packed]

Inputs: 8 seeded synthetic frames (kb.synthetic.make_triplet: band-limited images, a smooth dense depth whose sparse samples
are the sparse depth and whose 30 % samples are the ground truth) written ONCE as PNG files into a temporary directory, and listed
cyclically up to the run's length; the checkpoint holds seeded weights of the full KITTI network.  Method: one warm-up run of each
kind, then (a)-off, (a)-on and (b) ALTERNATE for `--rounds` rounds in this one process; every timed run lasts at least about a
second; per kind the median with the smallest and the largest.  (c): after a warm-up, windows of back-to-back launches between two
device events, the sources rotating through 4 sets (370 MB: more than the last-level cache holds), a second of device time in all."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import kbnet_amd as kb  # noqa: E402

H, W, BATCH = 352, 1216, 8
DISTINCT = 8


def write_dataset(directory, cfg, dev):
    """8 frames as files + the four path lists of `length` cyclic entries are written by `lists`; -> the per-frame file names."""
    image0, image1, image2, depth, sparse, _, intrinsics, _, _ = kb.synthetic.make_triplet(DISTINCT, H, W, "kitti", seed=11)
    rng = np.random.default_rng(12)
    files = []
    for i in range(DISTINCT):
        triplet = torch.cat([image1[i], image0[i], image2[i]], dim=-1)      # t-1, t, t+1 side by side
        px = (triplet * 255.0).round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous().numpy()
        truth = (depth[i, 0].numpy() * (rng.uniform(size=(H, W)) < 0.3)).astype(np.float32)
        names = [os.path.join(directory, f"{kind}_{i}.{ext}") for kind, ext in (("image", "png"), ("sparse", "png"), ("k", "npy"), ("truth", "png"))]
        with open(names[0], "wb") as f:
            f.write(kb.loader.encode_image_png(px, level=1))
        kb.loader.save_depth(sparse[i, 0].numpy(), names[1])
        np.save(names[2], intrinsics[i].numpy())
        kb.loader.save_depth(truth, names[3])
        files.append(names)
    model = kb.modules.KBNetModel.from_config(cfg, dev)
    model.load_state_dicts(*kb.synthetic.make_state_dicts(cfg, seed=0, gain=1.3))
    checkpoint = os.path.join(directory, "model.pth")
    model.save_model(checkpoint, step=1)
    return files, checkpoint


def lists(directory, files, length, tag):
    paths = []
    for column, name in enumerate(("image", "sparse_depth", "intrinsics", "ground_truth")):
        path = os.path.join(directory, f"{tag}_{name}.txt")
        kb.loader.write_paths(path, [files[i % DISTINCT][column] for i in range(length)])
        paths.append(path)
    return paths


def settings(cfg):
    return dict(min_pool_sizes_sparse_to_dense_pool=list(cfg.min_pool_sizes_sparse_to_dense_pool),
                max_pool_sizes_sparse_to_dense_pool=list(cfg.max_pool_sizes_sparse_to_dense_pool),
                n_filters_encoder_image=list(cfg.n_filters_encoder_image), n_filters_encoder_depth=list(cfg.n_filters_encoder_depth),
                n_filters_decoder=list(cfg.n_filters_decoder), min_predict_depth=cfg.min_predict_depth, max_predict_depth=cfg.max_predict_depth)


def ours(paths, checkpoint, out, cfg, save_outputs, workers, output_format="png"):
    shutil.rmtree(out, ignore_errors=True)
    start = time.perf_counter()
    result = kb.inference.run_with_format(*paths, checkpoint_path=out, depth_model_restore_path=checkpoint, save_outputs=save_outputs,
                              batch_size=BATCH, workers=workers, return_results=False, output_format=output_format, **settings(cfg))
    torch.cuda.synchronize()
    assert result is None
    return time.perf_counter() - start


def reference_export(paths, checkpoint, out, cfg, workers):
    """The reference's export over the same device path: everything to host lists as float32, the files after the loop through PIL."""
    from PIL import Image
    shutil.rmtree(out, ignore_errors=True)
    dev = torch.device("cuda")
    start = time.perf_counter()
    image_paths, sparse_paths, k_paths, truth_paths = (kb.loader.read_paths(p) for p in paths)
    ground_truths = []
    for path in truth_paths:
        z = np.array(Image.open(path), dtype=np.float32) / 256.0
        z[z <= 0] = 0.0
        v = z.astype(np.float32)
        v[z > 0] = 1.0
        ground_truths.append(np.stack([z, v], axis=-1))
    model = kb.modules.KBNetModel.from_config(cfg, dev)
    model.restore_model(checkpoint)
    images, output_depths, sparse_depths = [], [], []
    frames = kb.loader.InferenceFrameLoader(image_paths, sparse_paths, k_paths, use_image_triplet=True, batch_size=BATCH, device=dev, workers=workers)
    with torch.no_grad():
        for image, sparse_depth, intrinsics in frames:
            image, validity, filtered = kb.ops.preprocess(image, sparse_depth)
            output_depth = model.forward(image=image, sparse_depth=sparse_depth, validity_map_depth=validity, intrinsics=intrinsics)
            for i in range(image.shape[0]):
                output = np.squeeze(output_depth[i:i + 1].detach().cpu().numpy())
                images.append(np.transpose(np.squeeze(image[i:i + 1].cpu().numpy()), (1, 2, 0)))
                sparse_depths.append(np.squeeze(filtered[i:i + 1].cpu().numpy()))
                output_depths.append(output)
    dirpaths = [os.path.join(out, "outputs", d) for d in kb.loader.OUTPUT_DIRECTORIES]
    for d in dirpaths:
        os.makedirs(d)

    def save_depth(z, path):
        Image.fromarray(np.uint32(z * 256.0), mode="I").save(path)

    for idx, (image, output_depth, sparse_depth, ground_truth) in enumerate(zip(images, output_depths, sparse_depths, ground_truths)):
        filename = "{:010d}.png".format(idx)
        Image.fromarray((255 * image).astype(np.uint8)).save(os.path.join(dirpaths[0], filename))
        save_depth(output_depth, os.path.join(dirpaths[1], filename))
        save_depth(sparse_depth, os.path.join(dirpaths[2], filename))
        save_depth(ground_truth[..., 0], os.path.join(dirpaths[3], filename))
    return time.perf_counter() - start


def pack_alone(dev, windows, per_window):
    lib = kb._lib.load()
    n, px = BATCH, BATCH * H * W
    g = torch.Generator(device=dev).manual_seed(5)
    sets = []
    for _ in range(4):
        image = torch.rand((n, 3, H, W), generator=g, device=dev)
        depth_a = 1.5 + 98.5 * torch.rand((n, 1, H, W), generator=g, device=dev)
        depth_b = depth_a * (torch.rand((n, 1, H, W), generator=g, device=dev) < 0.05)
        outs = (torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev), torch.empty((n, H, W), dtype=torch.int16, device=dev),
                torch.empty((n, H, W), dtype=torch.int16, device=dev))
        sets.append((image, depth_a, depth_b) + outs)
    stream = torch.cuda.current_stream().cuda_stream

    def launch(s):
        rc = lib.kbn_export_pack_forward(s[0].data_ptr(), 255.0, 0.0, s[1].data_ptr(), s[2].data_ptr(), s[3].data_ptr(), s[4].data_ptr(),
                                         s[5].data_ptr(), n, H, W, stream)
        assert rc == 0, rc

    for i in range(64):
        launch(sets[i % 4])
    torch.cuda.synchronize()
    times = []
    for _ in range(windows):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for i in range(per_window):
            launch(sets[i % 4])
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end) * 1e3 / per_window)      # us a launch
    nbytes = 27.0 * px
    med = statistics.median(times)
    return {"us_per_launch": [min(times), med, max(times)], "bytes_per_launch": nbytes, "read_bytes": 20.0 * px, "written_bytes": 7.0 * px,
            "TB_per_s": [nbytes / (t * 1e-6) / 1e12 for t in (max(times), med, min(times))], "windows": windows, "launches_per_window": per_window,
            "device_seconds": sum(times) * per_window * 1e-6}


def pack_frames_alone(dev, windows, per_window):
    """The two ops.pack_frames calls OutputWriter(file_format="packed") makes for a batch, between device events."""
    n = BATCH
    g = torch.Generator(device=dev).manual_seed(5)
    sets = []
    for _ in range(4):
        image = torch.rand((n, 3, H, W), generator=g, device=dev)
        image = torch.nn.functional.avg_pool2d(image, 9, stride=1, padding=4)      # a picture has neighbours that resemble each other
        depth_a = 1.5 + 98.5 * torch.nn.functional.avg_pool2d(torch.rand((n, 1, H, W), generator=g, device=dev), 31, stride=1, padding=15)
        depth_b = depth_a * (torch.rand((n, 1, H, W), generator=g, device=dev) < 0.05)
        planes = torch.empty((2 * n, H, W), dtype=torch.int16, device=dev)
        rgb, _, _ = kb.ops.export_pack(image, depth_a, depth_b, out=(None, planes[:n], planes[n:]))
        out_rgb = torch.empty((n, kb.ops.pack_frames_stride(H, W, 3, 8)), dtype=torch.uint8, device=dev)
        out_planes = torch.empty((2 * n, kb.ops.pack_frames_stride(H, W, 1, 16)), dtype=torch.uint8, device=dev)
        sets.append((rgb, planes, out_rgb, out_planes, torch.empty(n, dtype=torch.int64, device=dev), torch.empty(2 * n, dtype=torch.int64, device=dev)))
    work = torch.empty(max(kb.ops.pack_frames_workspace_bytes(n, H, W, 3, 8), kb.ops.pack_frames_workspace_bytes(2 * n, H, W, 1, 16)),
                       dtype=torch.uint8, device=dev)

    def launch(s, which):
        if which != "planes":
            kb.ops.pack_frames(s[0], out=s[2], out_bytes=s[4], workspace=work)
        if which != "rgb":
            kb.ops.pack_frames(s[1], out=s[3], out_bytes=s[5], workspace=work)

    result = {"windows": windows, "calls_per_window": per_window}
    for which in ("rgb", "planes", "both"):
        for i in range(16):
            launch(sets[i % 4], which)
        torch.cuda.synchronize()
        times = []
        for _ in range(windows):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for i in range(per_window):
                launch(sets[i % 4], which)
            end.record()
            end.synchronize()
            times.append(start.elapsed_time(end) * 1e3 / per_window)
        result[f"us_{which}"] = spread(times)
    result["encoded_bytes_rgb_frame"] = float(sets[0][4].double().mean())
    result["encoded_bytes_plane"] = float(sets[0][5].double().mean())
    result["sample_bytes_batch"] = 7.0 * n * H * W
    return result


def writer_alone(dev, tmp, workers, batches):
    """frames/s of OutputWriter fed the same resident batch `batches[format]` times: wall clock from the first submit to close()."""
    g = torch.Generator(device=dev).manual_seed(6)
    image = torch.nn.functional.avg_pool2d(torch.rand((BATCH, 3, H, W), generator=g, device=dev), 9, stride=1, padding=4)
    depth_a = 1.5 + 98.5 * torch.nn.functional.avg_pool2d(torch.rand((BATCH, 1, H, W), generator=g, device=dev), 31, stride=1, padding=15)
    depth_b = depth_a * (torch.rand((BATCH, 1, H, W), generator=g, device=dev) < 0.05)
    truth = kb.loader.depth_samples(depth_a * (torch.rand((BATCH, 1, H, W), generator=g, device=dev) < 0.3)).reshape(BATCH, H, W)
    result = {}
    for fmt in kb.loader.OUTPUT_FORMATS:
        for with_truth in (True, False):
            times = []
            for r in range(3):      # the first is the warm-up
                out = os.path.join(tmp, f"writer_{fmt}_{int(with_truth)}")
                shutil.rmtree(out, ignore_errors=True)
                torch.cuda.synchronize()
                start = time.perf_counter()
                with kb.loader.OutputWriter(out, threads=workers, file_format=fmt) as writer:
                    for b in range(batches[fmt]):
                        writer.submit([f"{b}_{i}.png" for i in range(BATCH)], image, depth_a, depth_b, ground_truth_samples=truth if with_truth else None)
                times.append(time.perf_counter() - start)
            result[f"{fmt}_{'with' if with_truth else 'without'}_truth_frames_per_s"] = sorted(batches[fmt] * BATCH / t for t in times[1:])
    return result


def spread(values):
    return [min(values), statistics.median(values), max(values)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="short runs (a rehearsal, not a measurement)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--packed", action="store_true", help="also measure the packed export and the pack_frames launches")
    ap.add_argument("--no_reference", action="store_true", help="leave (b), the reference's export through PIL, out")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "run_export_bench.py measures on the GPU: no device, no number"
    dev = torch.device("cuda")
    cfg = kb.kitti_config()
    frames_off, frames_on = (64, 16) if args.quick else (1024, 160)
    try:
        import PIL  # noqa: F401
        have_pil = True
    except ImportError:
        have_pil = False
    have_pil = have_pil and not args.no_reference
    result = {"shape": [BATCH, H, W], "device": torch.cuda.get_device_name(0), "workers": args.workers, "rounds": args.rounds,
              "frames": {"off": frames_off, "on": frames_on, "reference_export": frames_on}, "pil": have_pil}
    with tempfile.TemporaryDirectory() as tmp:
        files, checkpoint = write_dataset(tmp, cfg, dev)
        off, on = lists(tmp, files, frames_off, "off"), lists(tmp, files, frames_on, "on")
        warm = lists(tmp, files, 2 * BATCH, "warm")
        ours(warm, checkpoint, os.path.join(tmp, "w0"), cfg, False, args.workers)
        ours(warm, checkpoint, os.path.join(tmp, "w1"), cfg, True, args.workers)
        if have_pil:
            reference_export(warm, checkpoint, os.path.join(tmp, "w2"), cfg, args.workers)
        if args.packed:
            frames_packed = 4 * frames_on      # a run of about a second, as the others
            packed_files = [[os.path.splitext(name)[0] + ".kbf" if column != 2 else name for column, name in enumerate(names)] for names in files]
            kb.loader.pack_frames([n for names in files for c, n in enumerate(names) if c != 2],
                                  [n for names in packed_files for c, n in enumerate(names) if c != 2], workers=args.workers)
            on_packed, off_in, on_all = (lists(tmp, files, frames_packed, "onp"), lists(tmp, packed_files, frames_off, "offin"),
                                         lists(tmp, packed_files, frames_packed, "onall"))
            ours(warm, checkpoint, os.path.join(tmp, "w3"), cfg, True, args.workers, "packed")
            ours(lists(tmp, packed_files, 2 * BATCH, "warmp"), checkpoint, os.path.join(tmp, "w4"), cfg, True, args.workers, "packed")
            result["frames"].update(on_packed=frames_packed, off_packed_inputs=frames_off, on_packed_inputs_and_outputs=frames_packed)
        seconds = {"off": [], "on": [], "on_packed": [], "off_packed_inputs": [], "on_packed_inputs_and_outputs": [], "reference_export": []}
        for r in range(args.rounds):
            seconds["off"].append(ours(off, checkpoint, os.path.join(tmp, "a0"), cfg, False, args.workers))
            seconds["on"].append(ours(on, checkpoint, os.path.join(tmp, "a1"), cfg, True, args.workers))
            if args.packed:
                seconds["on_packed"].append(ours(on_packed, checkpoint, os.path.join(tmp, "a2"), cfg, True, args.workers, "packed"))
                seconds["off_packed_inputs"].append(ours(off_in, checkpoint, os.path.join(tmp, "a3"), cfg, False, args.workers))
                seconds["on_packed_inputs_and_outputs"].append(ours(on_all, checkpoint, os.path.join(tmp, "a4"), cfg, True, args.workers, "packed"))
            if have_pil:
                seconds["reference_export"].append(reference_export(on, checkpoint, os.path.join(tmp, "b"), cfg, args.workers))
            print(f"round {r}: " + "  ".join(f"{k} {v[-1]:.3f} s" for k, v in seconds.items() if v), flush=True)
        # the device's share of an export-on run: the time line of its results.txt
        with open(os.path.join(tmp, "a1", "results.txt")) as f:
            result["device_ms_per_frame_on"] = float(f.read().split("Average time per sample: ")[1].split(" ms")[0])
        written = sum(os.path.getsize(os.path.join(tmp, "a1", "outputs", d, n)) for d in kb.loader.OUTPUT_DIRECTORIES
                      for n in os.listdir(os.path.join(tmp, "a1", "outputs", d)))
        result["written_MB_per_frame"] = written / frames_on / 1e6
        if args.packed:
            with open(os.path.join(tmp, "a2", "results.txt")) as f:
                result["device_ms_per_frame_on_packed"] = float(f.read().split("Average time per sample: ")[1].split(" ms")[0])
            for name, run_dir, count in (("png", "a1", frames_on), ("packed", "a2", frames_packed)):
                result[f"written_MB_per_frame_by_directory_{name}"] = {
                    d: sum(os.path.getsize(os.path.join(tmp, run_dir, "outputs", d, n)) for n in os.listdir(os.path.join(tmp, run_dir, "outputs", d)))
                    / count / 1e6 for d in kb.loader.OUTPUT_DIRECTORIES}
            result["writer_alone"] = writer_alone(dev, tmp, args.workers, {"png": 2 if args.quick else 10, "packed": 4 if args.quick else 60})
    result["seconds"] = {k: spread(v) if v else "not measured" for k, v in seconds.items()}
    result["frames_per_s"] = {k: [result["frames"][k] / t for t in reversed(spread(v))] if v else "not measured" for k, v in seconds.items()}
    if args.packed:
        result["pack_frames"] = pack_frames_alone(dev, 3 if args.quick else 12, 20 if args.quick else 100)
    result["pack"] = pack_alone(dev, 4 if args.quick else 24, 200 if args.quick else 2000)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
