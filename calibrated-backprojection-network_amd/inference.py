"""The inference entry point: the reference's run() (src/kbnet.py:676-1026, what run_kbnet.py calls) on this package's device path
-- score a checkpoint on a list of frames, write results.txt and, with save_outputs, the four directories of PNG files (or, through
run_with_format(..., output_format="packed"), of packed frames encoded on the device: DESIGN 8u); run_with_point_clouds also writes
every frame's metric point clouds as binary PLY files, backprojected on the device.

    reference, per frame (batch 1)                          here, per batch of any size
    DataLoader(KBNetInferenceDataset), .to(device)          loader.InferenceFrameLoader: decoded on host threads, raw bytes over PCIe
    every ground truth loaded through PIL before the loop   the batch's files read and decoded on host threads one batch ahead
                                                            (native reader), uploaded as 2 bytes a pixel, ops.unpack_frames
    validity map, outlier removal, transforms.transform     ops.preprocess: one launch
    depth_model.forward                                     the fused forward under no_grad, on the UNFILTERED sparse depth and
                                                            the filtered validity map, as the reference
    .cpu().numpy(), mask, four NumPy metrics                ops.eval_metrics: the rows stay on the device until the loop is over
    image, output, filtered sparse depth kept in host       loader.OutputWriter: one pack launch a batch, 7 bytes a pixel to a
    lists as float32, all files written after the loop      pinned slot, the files encoded and written by host threads meanwhile
    time.time() around transform + forward, no synchronise  device events around preprocess + forward, read after the loop

The loop never waits for the device or for the files; the first wait is the copy of the N x 4 metric rows after it.  One process,
one GPU: sharding a run over ranks is dist.ShardedRunner's business."""

from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import loader, ops
from ._lib import KbnError
from .modules import KBNetModel
from .summary import log, log_evaluation_settings, log_input_settings, log_network_settings, log_system_settings


class _GroundTruthReader:
    """The ground-truth files of batch b + 1 -- PNGs or packed frames (told apart by the magic; a batch is all one or all the other)
    -- read and decoded (native readers, host threads) into a pinned slot while batch b runs.  get(b) -> (host uint16 view nb x H x W, device int16 nb x H x W): the upload is one asynchronous copy of 2 bytes a pixel
    on the current stream.  A slot is decoded into again only after the copy that last read it has finished."""

    SLOTS = 3

    def __init__(self, paths, batch_size: int, device, workers: int):
        self.paths, self.batch_size, self.device, self.workers = list(paths), int(batch_size), device, max(1, int(workers))
        self.pool = ThreadPoolExecutor(max_workers=min(16, self.workers))     # file reads
        self.driver = ThreadPoolExecutor(max_workers=1)
        self.slots = [{"host": None, "copied": None} for _ in range(self.SLOTS)]
        self.n_batch = (len(self.paths) + self.batch_size - 1) // self.batch_size
        self.pending = {}
        self._ahead(0)

    def _ahead(self, b: int):
        if b < self.n_batch and b not in self.pending:
            self.pending[b] = self.driver.submit(self._decode, b)

    def _decode(self, b: int):
        paths = self.paths[b * self.batch_size:(b + 1) * self.batch_size]
        files = list(self.pool.map(loader._read, paths))
        packed = loader._one_kind(paths, [loader.is_packed_frame(data) for data in files], "run: ground truth")
        info = (lambda data: loader.frame_info(data[:loader.FRAME_HEADER_BYTES])) if packed else loader.png_info
        w, h, c, bits = info(files[0])
        for path, data in zip(paths, files):
            if info(data) != (w, h, 1, 16):
                raise KbnError(f"run: ground truth {path} is not a 16-bit single-channel {'packed frame' if packed else 'PNG'} of "
                               f"{h} x {w} like the first of its batch")
        slot = self.slots[b % self.SLOTS]
        if slot["copied"] is not None:
            slot["copied"].synchronize()
        if slot["host"] is None or tuple(slot["host"].shape[1:]) != (h, w):
            slot["host"] = torch.empty((self.batch_size, h, w), dtype=torch.int16).pin_memory()
        view = slot["host"].numpy().view(np.uint16)
        if packed:      # kbn_frame_decode runs kbn_frame_check first; ctypes drops the interpreter lock around it
            list(self.pool.map(lambda j: loader.decode_frame(files[j], out=view[j]), range(len(files))))
        else:
            loader.decode_png_batch(files, [view[j] for j in range(len(files))], threads=self.workers)
        return slot, len(files)

    def get(self, b: int):
        self._ahead(b)
        slot, nb = self.pending.pop(b).result()
        self._ahead(b + 1)
        raw = slot["host"][:nb].to(self.device, non_blocking=True)
        slot["copied"] = torch.cuda.Event()
        slot["copied"].record(torch.cuda.current_stream(self.device))
        return slot["host"][:nb].numpy().view(np.uint16), raw

    def close(self):
        for f in self.pending.values():
            f.exception()
        self.driver.shutdown(wait=True)
        self.pool.shutdown(wait=True)


def run(image_path,
        sparse_depth_path,
        intrinsics_path,
        ground_truth_path=None,
        # Input settings
        input_channels_image=3,
        input_channels_depth=2,
        normalized_image_range=[0, 1],
        outlier_removal_kernel_size=7,
        outlier_removal_threshold=1.5,
        # Sparse to dense pool settings
        min_pool_sizes_sparse_to_dense_pool=[5, 7, 9, 11, 13],
        max_pool_sizes_sparse_to_dense_pool=[15, 17],
        n_convolution_sparse_to_dense_pool=3,
        n_filter_sparse_to_dense_pool=8,
        # Depth network settings
        n_filters_encoder_image=[48, 96, 192, 384, 384],
        n_filters_encoder_depth=[16, 32, 64, 128, 128],
        resolutions_backprojection=[0, 1, 2, 3],
        n_filters_decoder=[256, 128, 128, 64, 12],
        deconv_type="up",
        min_predict_depth=1.5,
        max_predict_depth=100.0,
        # Weight settings
        weight_initializer="xavier_normal",
        activation_func="leaky_relu",
        # Evaluation settings
        min_evaluate_depth=0.0,
        max_evaluate_depth=100.0,
        # Checkpoint settings
        checkpoint_path="trained_kbnet",
        depth_model_restore_path=None,
        # Output settings
        save_outputs=False,
        keep_input_filenames=False,
        # Hardware settings
        device="cuda",
        *,
        batch_size=8,
        workers=8,
        png_level=6,
        return_results=False):
    """run_with_format with output_format "png": the reference's run() under its arguments, names and defaults, then keyword-only
    batch_size, workers, png_level and return_results -- the signature of DESIGN 8n, which stays as it is.  Everything is documented
    at run_with_format."""
    return _run(**locals(), output_format="png", point_clouds=None, point_cloud_depth_range=None)


def run_with_format(image_path,
                    sparse_depth_path,
                    intrinsics_path,
                    ground_truth_path=None,
                    # Input settings
                    input_channels_image=3,
                    input_channels_depth=2,
                    normalized_image_range=[0, 1],
                    outlier_removal_kernel_size=7,
                    outlier_removal_threshold=1.5,
                    # Sparse to dense pool settings
                    min_pool_sizes_sparse_to_dense_pool=[5, 7, 9, 11, 13],
                    max_pool_sizes_sparse_to_dense_pool=[15, 17],
                    n_convolution_sparse_to_dense_pool=3,
                    n_filter_sparse_to_dense_pool=8,
                    # Depth network settings
                    n_filters_encoder_image=[48, 96, 192, 384, 384],
                    n_filters_encoder_depth=[16, 32, 64, 128, 128],
                    resolutions_backprojection=[0, 1, 2, 3],
                    n_filters_decoder=[256, 128, 128, 64, 12],
                    deconv_type="up",
                    min_predict_depth=1.5,
                    max_predict_depth=100.0,
                    # Weight settings
                    weight_initializer="xavier_normal",
                    activation_func="leaky_relu",
                    # Evaluation settings
                    min_evaluate_depth=0.0,
                    max_evaluate_depth=100.0,
                    # Checkpoint settings
                    checkpoint_path="trained_kbnet",
                    depth_model_restore_path=None,
                    # Output settings
                    save_outputs=False,
                    keep_input_filenames=False,
                    # Hardware settings
                    device="cuda",
                    *,
                    output_format="png",
                    batch_size=8,
                    workers=8,
                    png_level=6,
                    return_results=False):
    """The reference's run() (src/kbnet.py:676-1026): its arguments, names and defaults (src/global_constants.py), then keyword-only
    batch_size (frames a forward; the last batch may be short), workers (host threads of the loader, of the ground-truth reader and
    of the writer), png_level (zlib level of the written files), return_results, and output_format: "png" (what run() passes) or
    "packed" for packed frames (`<name>.kbf` in the same four directories, encoded on the device, readable as sparse
    depth and ground truth by this package's loaders; png_level is ignored); any other value raises KbnError before anything else
    happens.  run() is this function without output_format.

    image_path, sparse_depth_path, intrinsics_path, ground_truth_path: newline-delimited files of paths (loader.read_paths);
    ground_truth_path '' or None: no ground truth, no metrics.  As the reference's run() builds KBNetInferenceDataset with its default
    use_image_triplet=True, every image file is a TRIPLET whose middle third is the frame; an image entry may also be a sequence
    entry previous<TAB>current<TAB>next, of which `current` is the frame and the only file read.  Writes checkpoint_path/results.txt --
    the input paths, the four settings blocks, the mean and the standard deviation over the frames of each frame's MAE, RMSE [mm],
    iMAE, iRMSE [1/km], the time -- and with save_outputs checkpoint_path/outputs/{image, output_depth, sparse_depth, ground_truth}/
    <name>.png per frame: the normalised image, the output depth, the FILTERED sparse depth, the ground truth's own samples; <name>
    is '{:010d}.png' of the dataset index, or the image file's base name (`current`'s, of a sequence entry) with keep_input_filenames.

    Returns None, as the reference; with return_results a dict: per_frame (N x 4 fp64 host tensor, None without ground truth), mean
    and std (four floats each, None without ground truth), time_ms, and output_depth, N x 1 x H x W fp32 on the host -- THE WHOLE
    DATASET IN (PINNED) HOST MEMORY, 4 bytes a pixel: meant for tests and small sets.

    Differences from the reference, on purpose: batches instead of batch 1; the time line goes to results.txt too and is device time
    (events around preprocess + forward); device 'cpu' and path lists of different lengths raise KbnError; the image files of the
    [-1, 1] and [0, 255] ranges hold the picture (loader.image_export_affine); files are written while the run proceeds."""
    return _run(**locals(), point_clouds=None, point_cloud_depth_range=None)


def run_with_point_clouds(image_path,
                          sparse_depth_path,
                          intrinsics_path,
                          ground_truth_path=None,
                          # Input settings
                          input_channels_image=3,
                          input_channels_depth=2,
                          normalized_image_range=[0, 1],
                          outlier_removal_kernel_size=7,
                          outlier_removal_threshold=1.5,
                          # Sparse to dense pool settings
                          min_pool_sizes_sparse_to_dense_pool=[5, 7, 9, 11, 13],
                          max_pool_sizes_sparse_to_dense_pool=[15, 17],
                          n_convolution_sparse_to_dense_pool=3,
                          n_filter_sparse_to_dense_pool=8,
                          # Depth network settings
                          n_filters_encoder_image=[48, 96, 192, 384, 384],
                          n_filters_encoder_depth=[16, 32, 64, 128, 128],
                          resolutions_backprojection=[0, 1, 2, 3],
                          n_filters_decoder=[256, 128, 128, 64, 12],
                          deconv_type="up",
                          min_predict_depth=1.5,
                          max_predict_depth=100.0,
                          # Weight settings
                          weight_initializer="xavier_normal",
                          activation_func="leaky_relu",
                          # Evaluation settings
                          min_evaluate_depth=0.0,
                          max_evaluate_depth=100.0,
                          # Checkpoint settings
                          checkpoint_path="trained_kbnet",
                          depth_model_restore_path=None,
                          # Output settings
                          save_outputs=False,
                          keep_input_filenames=False,
                          # Hardware settings
                          device="cuda",
                          *,
                          output_format="png",
                          batch_size=8,
                          workers=8,
                          png_level=6,
                          return_results=False,
                          point_clouds=("output_depth",),
                          point_cloud_depth_range=None):
    """run_with_format (its arguments, name for name; everything is documented there) that also writes metric point clouds
    (DESIGN 8y): per frame checkpoint_path/outputs/point_cloud/<name>.ply for "output_depth" and
    checkpoint_path/outputs/sparse_point_cloud/<name>.ply for "sparse_depth" in `point_clouds`, <name> being the PNG's with the
    extension replaced -- binary little-endian PLY files (loader.ply_header, loader.load_point_cloud) of the pixels whose depth is
    finite, above 0 and inside the closed point_cloud_depth_range (None: no further bound), in row-major order, in the camera frame
    and in metres, coloured with the image file's pixels.  The points are K^-1 [x y 1]^T z of the fp32 output depth and of the
    FILTERED sparse depth under the batch's intrinsics, made on the device (ops.point_cloud) and written by loader.PointCloudWriter
    while the run proceeds, whether or not save_outputs is set.  An unknown cloud name, a repeated one or an empty selection raises
    KbnError before anything touches the disk or the device.  Everything else -- results.txt, the four directories, the returned
    dict -- is run_with_format's, byte for byte."""
    point_clouds = loader.point_cloud_names(point_clouds)      # None is no selection here; _run reads it as "no point clouds"
    return _run(**locals())


def _run(*, image_path, sparse_depth_path, intrinsics_path, ground_truth_path, input_channels_image, input_channels_depth, normalized_image_range,
         outlier_removal_kernel_size, outlier_removal_threshold, min_pool_sizes_sparse_to_dense_pool, max_pool_sizes_sparse_to_dense_pool,
         n_convolution_sparse_to_dense_pool, n_filter_sparse_to_dense_pool, n_filters_encoder_image, n_filters_encoder_depth,
         resolutions_backprojection, n_filters_decoder, deconv_type, min_predict_depth, max_predict_depth, weight_initializer, activation_func,
         min_evaluate_depth, max_evaluate_depth, checkpoint_path, depth_model_restore_path, save_outputs, keep_input_filenames, device,
         output_format, batch_size, workers, png_level, return_results, point_clouds, point_cloud_depth_range):
    """The run behind run, run_with_format and run_with_point_clouds: every argument of theirs, by name, no defaults.  point_clouds
    None: no point clouds."""
    if output_format not in loader.OUTPUT_FORMATS:
        raise KbnError(f"run: output_format {output_format!r}: expected one of {', '.join(repr(f) for f in loader.OUTPUT_FORMATS)}")
    if point_clouds is not None:
        point_clouds = loader.point_cloud_names(point_clouds)
        if point_cloud_depth_range is not None and not float(point_cloud_depth_range[0]) <= float(point_cloud_depth_range[1]):
            raise KbnError(f"run: point_cloud_depth_range {point_cloud_depth_range!r}: expected (min, max) with min <= max, or None")
    if device == "cuda" or device == "gpu":
        device = torch.device("cuda")
    else:
        raise KbnError(f"run: device {device!r}: the HIP path has no CPU fallback (the reference runs on the CPU for anything but 'cuda' / 'gpu')")
    if int(batch_size) < 1:
        raise KbnError(f"run: batch_size {batch_size}")
    batch_size = int(batch_size)

    if not os.path.exists(checkpoint_path):
        os.makedirs(checkpoint_path)
    log_path = os.path.join(checkpoint_path, "results.txt")
    output_path = os.path.join(checkpoint_path, "outputs")

    # ---- input paths ----
    image_paths = loader.read_paths(image_path)
    sparse_depth_paths = loader.read_paths(sparse_depth_path)
    intrinsics_paths = loader.read_paths(intrinsics_path)
    ground_truth_available = ground_truth_path is not None and ground_truth_path != ""
    ground_truth_paths = loader.read_paths(ground_truth_path) if ground_truth_available else None
    n_sample = len(image_paths)
    for name, paths in (("sparse depth", sparse_depth_paths), ("intrinsics", intrinsics_paths), ("ground truth", ground_truth_paths)):
        if paths is not None and len(paths) != n_sample:
            raise KbnError(f"run: {n_sample} image paths, {len(paths)} {name} paths")
    if n_sample < 1:
        raise KbnError(f"run: {image_path} lists no frame")

    # ---- the model ----
    depth_model = KBNetModel(
        input_channels_image=input_channels_image, input_channels_depth=input_channels_depth,
        min_pool_sizes_sparse_to_dense_pool=min_pool_sizes_sparse_to_dense_pool,
        max_pool_sizes_sparse_to_dense_pool=max_pool_sizes_sparse_to_dense_pool,
        n_convolution_sparse_to_dense_pool=n_convolution_sparse_to_dense_pool, n_filter_sparse_to_dense_pool=n_filter_sparse_to_dense_pool,
        n_filters_encoder_image=n_filters_encoder_image, n_filters_encoder_depth=n_filters_encoder_depth,
        resolutions_backprojection=resolutions_backprojection, n_filters_decoder=n_filters_decoder, deconv_type=deconv_type,
        weight_initializer=weight_initializer, activation_func=activation_func, min_predict_depth=min_predict_depth,
        max_predict_depth=max_predict_depth, device=device)
    depth_model.restore_model(depth_model_restore_path)
    depth_model.eval()
    parameters_depth_model = depth_model.parameters()

    # ---- the head of results.txt ----
    log("Input paths:", log_path)
    for path in [image_path, sparse_depth_path, intrinsics_path] + ([ground_truth_path] if ground_truth_available else []):
        log(path, log_path)
    log("", log_path)
    log_input_settings(
        log_path, input_channels_image=input_channels_image, input_channels_depth=input_channels_depth,
        normalized_image_range=normalized_image_range, outlier_removal_kernel_size=outlier_removal_kernel_size,
        outlier_removal_threshold=outlier_removal_threshold)
    log_network_settings(
        log_path, min_pool_sizes_sparse_to_dense_pool=min_pool_sizes_sparse_to_dense_pool,
        max_pool_sizes_sparse_to_dense_pool=max_pool_sizes_sparse_to_dense_pool,
        n_convolution_sparse_to_dense_pool=n_convolution_sparse_to_dense_pool, n_filter_sparse_to_dense_pool=n_filter_sparse_to_dense_pool,
        n_filters_encoder_image=n_filters_encoder_image, n_filters_encoder_depth=n_filters_encoder_depth,
        resolutions_backprojection=resolutions_backprojection, n_filters_decoder=n_filters_decoder, deconv_type=deconv_type,
        min_predict_depth=min_predict_depth, max_predict_depth=max_predict_depth, weight_initializer=weight_initializer,
        activation_func=activation_func, parameters_depth_model=parameters_depth_model)
    log_evaluation_settings(log_path, min_evaluate_depth=min_evaluate_depth, max_evaluate_depth=max_evaluate_depth)
    log_system_settings(log_path, checkpoint_path=checkpoint_path, depth_model_restore_path=depth_model_restore_path, device=device,
                        n_thread=1)

    # ---- the run ----
    frames = loader.InferenceFrameLoader(image_paths, sparse_depth_paths, intrinsics_paths, use_image_triplet=True,
                                         batch_size=batch_size, device=device, workers=workers)
    truths = _GroundTruthReader(ground_truth_paths, batch_size, device, workers) if ground_truth_available else None
    writer = None
    if save_outputs:
        writer = loader.OutputWriter(output_path, threads=workers, level=png_level, normalized_image_range=normalized_image_range,
                                     file_format=output_format)
    clouds = None
    if point_clouds is not None:
        clouds = loader.PointCloudWriter(output_path, clouds=point_clouds, threads=workers, normalized_image_range=normalized_image_range,
                                         depth_range=point_cloud_depth_range)
    rows, timers, kept = [], [], None
    seen = 0
    try:
        with torch.no_grad():
            for b, (image, sparse_depth, intrinsics) in enumerate(frames):
                n = image.shape[0]
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                image, filtered_validity_map_depth, filtered_sparse_depth = ops.preprocess(
                    image, sparse_depth, kernel_size=outlier_removal_kernel_size, threshold=outlier_removal_threshold,
                    normalized_image_range=normalized_image_range)
                output_depth = depth_model.forward(image=image, sparse_depth=sparse_depth,
                                                   validity_map_depth=filtered_validity_map_depth, intrinsics=intrinsics)
                end.record()
                timers.append((start, end))

                samples = None
                if truths is not None:
                    samples, raw = truths.get(b)
                    _, ground_truth = ops.unpack_frames(None, raw)
                    if tuple(ground_truth.shape) != tuple(output_depth.shape):
                        raise KbnError(f"run: ground truth {ground_truth_paths[seen]} is {tuple(ground_truth.shape[-2:])}, "
                                       f"the frame {tuple(output_depth.shape[-2:])}")
                    # the validity map of a ground truth is depth > 0 (data_utils.load_depth_with_validity_map), which is what the
                    # kernel asks of its validity plane: the depth serves as both
                    rows.append(ops.eval_metrics(output_depth, ground_truth, ground_truth, min_evaluate_depth, max_evaluate_depth))
                if writer is not None or clouds is not None:
                    if keep_input_filenames:
                        filenames = [os.path.basename(loader.sample_name(image_paths[seen + i])) for i in range(n)]
                    else:
                        filenames = ["{:010d}.png".format(seen + i) for i in range(n)]
                if writer is not None:
                    writer.submit(filenames, image, output_depth, filtered_sparse_depth, ground_truth_samples=samples)
                if clouds is not None:
                    clouds.submit(filenames, image, output_depth, filtered_sparse_depth, intrinsics)
                if return_results:
                    if kept is None:
                        kept = torch.empty((n_sample,) + tuple(output_depth.shape[1:]), dtype=torch.float32).pin_memory()
                    kept[seen:seen + n].copy_(output_depth, non_blocking=True)
                seen += n

        # ---- after the loop: the first wait for the device ----
        per_frame = mean = std = None
        if ground_truth_available:
            per_frame = torch.cat(rows, dim=0).cpu()      # the one copy of the N x 4 rows
            mae, rmse, imae, irmse = per_frame.numpy().T
            mean = [np.mean(mae), np.mean(rmse), np.mean(imae), np.mean(irmse)]
            std = [np.std(mae), np.std(rmse), np.std(imae), np.std(irmse)]
            log("Evaluation results:", log_path)
            log("{:>8}  {:>8}  {:>8}  {:>8}".format("MAE", "RMSE", "iMAE", "iRMSE"), log_path)
            log("{:8.3f}  {:8.3f}  {:8.3f}  {:8.3f}".format(*mean), log_path)
            log("{:>8}  {:>8}  {:>8}  {:>8}".format("+/-", "+/-", "+/-", "+/-"), log_path)
            log("{:8.3f}  {:8.3f}  {:8.3f}  {:8.3f}".format(*std), log_path)
        timers[-1][1].synchronize()
        time_elapse = float(sum(start.elapsed_time(end) for start, end in timers))      # ms
        log("Total time: {:.2f} ms  Average time per sample: {:.2f} ms".format(time_elapse, time_elapse / float(n_sample)), log_path)
        if save_outputs:
            log("Saving outputs to {}".format(output_path), log_path)
    except BaseException:
        for closing in (writer, clouds, truths):
            if closing is not None:
                try:
                    closing.close()
                except Exception:      # noqa: BLE001  (the run's own exception is the one to see)
                    pass
        raise
    if truths is not None:
        truths.close()
    if writer is not None:
        writer.close()
    if clouds is not None:
        clouds.close()
    if not return_results:
        return None
    torch.cuda.current_stream(device).synchronize()      # the copies into `kept`
    return {"per_frame": per_frame, "mean": mean, "std": std, "time_ms": time_elapse, "output_depth": kept}
