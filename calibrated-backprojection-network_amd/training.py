"""The training entry point: the reference's train() (src/kbnet.py:31-518, what train_kbnet.py calls) over this package's classes --
the loop INTEGRATION.md ("The training iteration") spells out, with the reference's logging, schedules, validation and checkpoints
around it.

    reference                                               here
    DataLoader(KBNetTrainingDataset, shuffle=True)          loader.TrainingFrameLoader(shuffle=True): device batches
    validity map, OutlierRemoval, Transforms.transform      transforms.train_inputs: one preprocess launch, two augment launches
    KBNetModel / PoseNetModel('resnet18') in .train()       KBNetModel(trainable=True).requires_grad_(True); ResNetPoseNetModel(18,
                                                            trainable=True).requires_grad_(True).set_batch_norm('batch')
    torch.optim.Adam over two groups                        optim.Adam: one launch a step
    SummaryWriter(event_path + '-train' / '-val')           summary.EventWriter: histograms on the device, copies behind the stream
    validate() at batch 1 through a DataLoader              validation.validate over loader.InferenceFrameLoader(val_batch_size)
    loss.item() at every checkpoint                         the same: the loop's only wait for the device

One process, one GPU.  The data-parallel loop stays the documented one (kb.dist.GradientAverager)."""

from __future__ import annotations

import os
import time

import numpy as np
import torch

from . import loader, optim, summary, transforms, validation
from ._lib import KbnError
from .modules import KBNetModel, ResNetPoseNetModel


def n_train_steps(n_train_sample: int, n_batch: int, learning_schedule) -> int:
    """reference src/kbnet.py:131-132: the last epoch of the schedule times the batches of an epoch, the last one short or not."""
    return int(learning_schedule[-1] * np.ceil(n_train_sample / n_batch).astype(np.int32))


def scheduled(epoch: int, position: int, schedule, values, frozen: bool = False):
    """reference src/kbnet.py:378-390 for one schedule at the start of `epoch` (1-based) -> (position, value, moved): the position
    moves on by ONE when the epoch lies behind the schedule's entry at the current position, never with `frozen` (the reference's
    `-1 in augmentation_schedule`)."""
    if not frozen and epoch > schedule[position]:
        return position + 1, values[position + 1], True
    return position, values[position], False


def train(train_image_path,
          train_sparse_depth_path,
          train_intrinsics_path,
          val_image_path,
          val_sparse_depth_path,
          val_intrinsics_path,
          val_ground_truth_path,
          # Batch settings
          n_batch=8,
          n_height=320,
          n_width=768,
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
          # Training settings
          learning_rates=[5e-5, 1e-4, 15e-5, 1e-4, 5e-5, 2e-5],
          learning_schedule=[2, 8, 20, 30, 45, 60],
          augmentation_probabilities=[1.00, 0.50, 0.25],
          augmentation_schedule=[50, 55, 60],
          augmentation_random_crop_type=["horizontal", "vertical", "anchored", "bottom"],
          augmentation_random_flip_type=["none"],
          augmentation_random_remove_points=[0.60, 0.70],
          augmentation_random_noise_type="none",
          augmentation_random_noise_spread=-1,
          # Loss function settings
          w_color=0.15,
          w_structure=0.95,
          w_sparse_depth=0.60,
          w_smoothness=0.04,
          w_weight_decay_depth=0.00,
          w_weight_decay_pose=0.00,
          # Evaluation settings
          min_evaluate_depth=0.00,
          max_evaluate_depth=100.0,
          # Checkpoint settings
          checkpoint_path="trained_kbnet",
          n_checkpoint=5000,
          n_summary=5000,
          n_summary_display=4,
          validation_start_step=200000,
          depth_model_restore_path=None,
          pose_model_restore_path=None,
          # Hardware settings
          device="cuda",
          n_thread=8,
          *,
          workers=None,
          val_batch_size=1,
          summary_writer_factory=summary.EventWriter,
          return_results=False):
    """The reference's train() (src/kbnet.py:31-518): its arguments, names, order and defaults (src/global_constants.py), then
    keyword-only workers (host threads of the two loaders; None: n_thread), val_batch_size (frames a validation forward),
    summary_writer_factory (called with event_path + '-train' and event_path + '-val'; any object with add_scalar, add_histogram,
    add_image and close fits) and return_results.

    The four path arguments of each set are newline-delimited files of paths (loader.read_paths); a validation argument that is
    None switches validation off.  Writes checkpoint_path/results.txt (the two path blocks, the six settings blocks, a line every
    n_checkpoint steps, validate()'s lines), checkpoint_path/depth_model-<step>.pth and pose_model-<step>.pth every n_checkpoint
    steps and after the last epoch, and the two event directories checkpoint_path/events-train and events-val.

    Returns None, as the reference; with return_results a tuple: {'train_step', 'best_results'}, the list of (step, loss) logged at
    the checkpoints, and the checkpoint paths written, depth and pose model alternating.

    The loop waits for the device where the reference logs the loss, at a checkpoint (loss.item()), and in validate(); between
    checkpoints nothing does.  Differences from the reference, on purpose: the shuffle order and the augmentation draws
    (loader.TrainingFrameLoader, transforms.Transforms); validation runs val_batch_size frames a forward; device 'cpu' and path
    lists of different lengths raise KbnError; a configuration the backward pass does not serve (deconv_type='transpose') raises
    before anything is written; restore_model's and the writers' errors propagate; neither model's train() / eval() is called
    (KBNetModel has one mode, the pose model's batch statistics are set_batch_norm('batch')).

    One process, one GPU: the multi-GPU loop is the documented one over kb.dist.GradientAverager."""
    if device == "cuda" or device == "gpu":
        device = torch.device("cuda")
    else:
        raise KbnError(f"train: device {device!r}: the HIP path has no CPU fallback (the reference trains on the CPU for anything but 'cuda' / 'gpu')")
    workers = int(n_thread if workers is None else workers)
    if int(val_batch_size) < 1:
        raise KbnError(f"train: val_batch_size {val_batch_size}")

    depth_model_checkpoint_path = os.path.join(checkpoint_path, "depth_model-{}.pth")
    pose_model_checkpoint_path = os.path.join(checkpoint_path, "pose_model-{}.pth")
    log_path = os.path.join(checkpoint_path, "results.txt")
    event_path = os.path.join(checkpoint_path, "events")

    best_results = {"step": -1, "mae": np.inf, "rmse": np.inf, "imae": np.inf, "irmse": np.inf}

    # ---- input paths ----
    train_image_paths = loader.read_paths(train_image_path)
    train_sparse_depth_paths = loader.read_paths(train_sparse_depth_path)
    train_intrinsics_paths = loader.read_paths(train_intrinsics_path)
    n_train_sample = len(train_image_paths)
    for name, paths in (("sparse depth", train_sparse_depth_paths), ("intrinsics", train_intrinsics_paths)):
        if len(paths) != n_train_sample:
            raise KbnError(f"train: {n_train_sample} training image paths, {len(paths)} {name} paths")
    if n_train_sample < 1:
        raise KbnError(f"train: {train_image_path} lists no frame")
    n_train_step = n_train_steps(n_train_sample, n_batch, learning_schedule)

    validation_available = val_image_path is not None and val_sparse_depth_path is not None and \
        val_intrinsics_path is not None and val_ground_truth_path is not None
    if validation_available:
        val_image_paths = loader.read_paths(val_image_path)
        val_sparse_depth_paths = loader.read_paths(val_sparse_depth_path)
        val_intrinsics_paths = loader.read_paths(val_intrinsics_path)
        val_ground_truth_paths = loader.read_paths(val_ground_truth_path)
        n_val_sample = len(val_image_paths)
        for name, paths in (("sparse depth", val_sparse_depth_paths), ("intrinsics", val_intrinsics_paths),
                            ("ground truth", val_ground_truth_paths)):
            if len(paths) != n_val_sample:
                raise KbnError(f"train: {n_val_sample} validation image paths, {len(paths)} {name} paths")

    # ---- the models: what KBNetModel(trainable=True) refuses is refused before anything is written ----
    depth_model = KBNetModel(
        input_channels_image=input_channels_image, input_channels_depth=input_channels_depth,
        min_pool_sizes_sparse_to_dense_pool=min_pool_sizes_sparse_to_dense_pool,
        max_pool_sizes_sparse_to_dense_pool=max_pool_sizes_sparse_to_dense_pool,
        n_convolution_sparse_to_dense_pool=n_convolution_sparse_to_dense_pool, n_filter_sparse_to_dense_pool=n_filter_sparse_to_dense_pool,
        n_filters_encoder_image=n_filters_encoder_image, n_filters_encoder_depth=n_filters_encoder_depth,
        resolutions_backprojection=resolutions_backprojection, n_filters_decoder=n_filters_decoder, deconv_type=deconv_type,
        weight_initializer=weight_initializer, activation_func=activation_func, min_predict_depth=min_predict_depth,
        max_predict_depth=max_predict_depth, device=device, trainable=True)
    depth_model.requires_grad_(True)
    parameters_depth_model = depth_model.parameters()

    pose_model = ResNetPoseNetModel(18, rotation_parameterization="axis", weight_initializer=weight_initializer, activation_func="relu",
                                    device=device, trainable=True)
    pose_model.requires_grad_(True).set_batch_norm("batch")      # the reference's pose_model.train()
    parameters_pose_model = pose_model.parameters()

    if depth_model_restore_path is not None and depth_model_restore_path != "":
        depth_model.restore_model(depth_model_restore_path)
    if pose_model_restore_path is not None and pose_model_restore_path != "":
        pose_model.restore_model(pose_model_restore_path)

    if not os.path.exists(checkpoint_path):
        os.makedirs(checkpoint_path)

    # ---- the loaders ----
    train_loader = loader.TrainingFrameLoader(train_image_paths, train_sparse_depth_paths, train_intrinsics_paths,
                                              shape=(n_height, n_width), random_crop_type=augmentation_random_crop_type,
                                              batch_size=n_batch, shuffle=True, device=device, workers=workers)
    train_transforms = transforms.Transforms(normalized_image_range=normalized_image_range, random_flip_type=augmentation_random_flip_type,
                                             random_remove_points=augmentation_random_remove_points,
                                             random_noise_type=augmentation_random_noise_type,
                                             random_noise_spread=augmentation_random_noise_spread)
    if validation_available:
        ground_truths = []
        for path in val_ground_truth_paths:
            ground_truth, validity_map = loader.load_depth_with_validity_map(path)
            ground_truths.append(np.stack([ground_truth, validity_map], axis=-1))
        val_dataloader = loader.InferenceFrameLoader(val_image_paths, val_sparse_depth_paths, val_intrinsics_paths, use_image_triplet=True,
                                                     batch_size=int(val_batch_size), device=device, workers=workers)

    train_summary_writer = val_summary_writer = None
    logged, checkpoints = [], []
    try:
        train_summary_writer = summary_writer_factory(event_path + "-train")
        val_summary_writer = summary_writer_factory(event_path + "-val")

        # ---- the head of results.txt ----
        log = summary.log
        log("Training input paths:", log_path)
        for path in (train_image_path, train_sparse_depth_path, train_intrinsics_path):
            log(path, log_path)
        log("", log_path)
        log("Validation input paths:", log_path)
        for path in (val_image_path, val_sparse_depth_path, val_intrinsics_path, val_ground_truth_path):
            log(path, log_path)
        log("", log_path)
        summary.log_input_settings(
            log_path, n_batch=n_batch, n_height=n_height, n_width=n_width, input_channels_image=input_channels_image,
            input_channels_depth=input_channels_depth, normalized_image_range=normalized_image_range,
            outlier_removal_kernel_size=outlier_removal_kernel_size, outlier_removal_threshold=outlier_removal_threshold)
        summary.log_network_settings(
            log_path, min_pool_sizes_sparse_to_dense_pool=min_pool_sizes_sparse_to_dense_pool,
            max_pool_sizes_sparse_to_dense_pool=max_pool_sizes_sparse_to_dense_pool,
            n_convolution_sparse_to_dense_pool=n_convolution_sparse_to_dense_pool, n_filter_sparse_to_dense_pool=n_filter_sparse_to_dense_pool,
            n_filters_encoder_image=n_filters_encoder_image, n_filters_encoder_depth=n_filters_encoder_depth,
            resolutions_backprojection=resolutions_backprojection, n_filters_decoder=n_filters_decoder, deconv_type=deconv_type,
            min_predict_depth=min_predict_depth, max_predict_depth=max_predict_depth, weight_initializer=weight_initializer,
            activation_func=activation_func, parameters_depth_model=parameters_depth_model, parameters_pose_model=parameters_pose_model)
        summary.log_training_settings(
            log_path, n_batch=n_batch, n_train_sample=n_train_sample, n_train_step=n_train_step, learning_rates=learning_rates,
            learning_schedule=learning_schedule, augmentation_probabilities=augmentation_probabilities,
            augmentation_schedule=augmentation_schedule, augmentation_random_crop_type=augmentation_random_crop_type,
            augmentation_random_flip_type=augmentation_random_flip_type, augmentation_random_remove_points=augmentation_random_remove_points,
            augmentation_random_noise_type=augmentation_random_noise_type, augmentation_random_noise_spread=augmentation_random_noise_spread)
        summary.log_loss_func_settings(
            log_path, w_color=w_color, w_structure=w_structure, w_sparse_depth=w_sparse_depth, w_smoothness=w_smoothness,
            w_weight_decay_depth=w_weight_decay_depth, w_weight_decay_pose=w_weight_decay_pose)
        summary.log_evaluation_settings(log_path, min_evaluate_depth=min_evaluate_depth, max_evaluate_depth=max_evaluate_depth)
        summary.log_system_settings(
            log_path, checkpoint_path=checkpoint_path, n_checkpoint=n_checkpoint, summary_event_path=event_path, n_summary=n_summary,
            n_summary_display=n_summary_display, validation_start_step=validation_start_step,
            depth_model_restore_path=depth_model_restore_path, pose_model_restore_path=pose_model_restore_path, device=device,
            n_thread=n_thread)

        # ---- the optimizer and the schedules ----
        learning_schedule_pos, learning_rate = 0, learning_rates[0]
        augmentation_schedule_pos, augmentation_probability = 0, augmentation_probabilities[0]
        optimizer = optim.Adam([{"params": parameters_depth_model, "weight_decay": w_weight_decay_depth},
                                {"params": parameters_pose_model, "weight_decay": w_weight_decay_pose}], lr=learning_rate)

        train_step = 0
        time_start = time.time()
        log("Begin training...", log_path)
        for epoch in range(1, learning_schedule[-1] + 1):
            learning_schedule_pos, learning_rate, moved = scheduled(epoch, learning_schedule_pos, learning_schedule, learning_rates)
            if moved:
                for g in optimizer.param_groups:
                    g["lr"] = learning_rate
            augmentation_schedule_pos, augmentation_probability, _ = scheduled(
                epoch, augmentation_schedule_pos, augmentation_schedule, augmentation_probabilities, frozen=-1 in augmentation_schedule)

            for image0, image1, image2, sparse_depth0, intrinsics in train_loader:
                train_step = train_step + 1
                image0, image1, image2, sparse_depth0, filtered_sparse_depth0, filtered_validity_map_depth0 = transforms.train_inputs(
                    train_transforms, image0, image1, image2, sparse_depth0, augmentation_probability,
                    kernel_size=outlier_removal_kernel_size, threshold=outlier_removal_threshold)
                output_depth0 = depth_model.forward(image=image0, sparse_depth=sparse_depth0,
                                                    validity_map_depth=filtered_validity_map_depth0, intrinsics=intrinsics)
                pose01 = pose_model.forward(image0, image1)
                pose02 = pose_model.forward(image0, image2)
                loss, loss_info = depth_model.compute_loss(
                    image0=image0, image1=image1, image2=image2, output_depth0=output_depth0, sparse_depth0=filtered_sparse_depth0,
                    validity_map_depth0=filtered_validity_map_depth0, intrinsics=intrinsics, pose01=pose01, pose02=pose02,
                    w_color=w_color, w_structure=w_structure, w_sparse_depth=w_sparse_depth, w_smoothness=w_smoothness)
                optimizer.zero_grad()
                loss.backward()
                optimizer.step()

                if (train_step % n_summary) == 0:
                    image01, image02 = loss_info.pop("image01"), loss_info.pop("image02")
                    loss_info.pop("per_frame")      # N x 4, this package's addition: a writer's add_scalar wants one number
                    depth_model.log_summary(summary_writer=train_summary_writer, tag="train", step=train_step, image0=image0,
                                            image01=image01, image02=image02, output_depth0=output_depth0.detach(),
                                            sparse_depth0=filtered_sparse_depth0, validity_map0=filtered_validity_map_depth0,
                                            pose01=pose01, pose02=pose02, scalars=loss_info, n_display=min(n_batch, n_summary_display))

                if (train_step % n_checkpoint) == 0:
                    value = loss.item()      # the loop's wait for the device, where the reference logs the loss
                    time_elapse = (time.time() - time_start) / 3600
                    time_remain = (n_train_step - train_step) * time_elapse / train_step
                    log("Step={:6}/{}  Loss={:.5f}  Time Elapsed={:.2f}h  Time Remaining={:.2f}h".format(
                        train_step, n_train_step, value, time_elapse, time_remain), log_path)
                    logged.append((train_step, value))
                    if train_step >= validation_start_step and validation_available:
                        best_results = validation.validate(
                            depth_model=depth_model, dataloader=val_dataloader, ground_truths=ground_truths, step=train_step,
                            best_results=best_results, min_evaluate_depth=min_evaluate_depth, max_evaluate_depth=max_evaluate_depth,
                            device=device, summary_writer=val_summary_writer, n_summary_display=n_summary_display, log_path=log_path,
                            outlier_removal_kernel_size=outlier_removal_kernel_size, outlier_removal_threshold=outlier_removal_threshold,
                            normalized_image_range=normalized_image_range)
                    for model, pattern in ((depth_model, depth_model_checkpoint_path), (pose_model, pose_model_checkpoint_path)):
                        model.save_model(pattern.format(train_step), train_step, optimizer)
                        checkpoints.append(pattern.format(train_step))

        for model, pattern in ((depth_model, depth_model_checkpoint_path), (pose_model, pose_model_checkpoint_path)):
            model.save_model(pattern.format(train_step), train_step, optimizer)
            if pattern.format(train_step) not in checkpoints:
                checkpoints.append(pattern.format(train_step))
    except BaseException:
        for writer in (train_summary_writer, val_summary_writer):
            if writer is not None:
                try:
                    writer.close()
                except Exception:      # noqa: BLE001  (the run's own exception is the one to see)
                    pass
        raise
    try:
        train_summary_writer.close()
    finally:
        val_summary_writer.close()
    if not return_results:
        return None
    return {"train_step": train_step, "best_results": best_results}, logged, checkpoints
