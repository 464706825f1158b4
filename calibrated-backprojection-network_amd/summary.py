"""The training loop's monitoring: what the reference's loop calls between optimizer.step() and save_model besides validate()
(validation.py) -- KBNetModel.log_summary (reference src/kbnet_model.py:417-650) and the two helpers of src/log_utils.py.

    reference                                   here
    log_utils.log(s, filepath, to_console)      log: the same lines into the same file
    log_utils.colorize(T, colormap)             colorize: matplotlib's lookup as a HIP kernel, on T's device
    KBNetModel.log_summary(...)                 log_summary (KBNetModel.log_summary calls it): the same add_histogram / add_scalar /
                                                add_image calls, the two image panels written by one launch each
                                                (ops.summary_image_panel, ops.summary_depth_panel)
    kbnet.log_*_settings (src/kbnet.py:1032-1296)  the six functions of those names: the settings blocks at the head of results.txt
                                                (kb.inference.run) and of the training log

The reference copies every tensor to the host, colourises frame by frame through matplotlib, concatenates on the CPU and calls
torchvision.utils.make_grid.  Here a panel is one kernel launch and stays on the device; the writer -- any object with add_image,
add_histogram and add_scalar, TensorBoard's SummaryWriter among them -- is handed device tensors and decides when they leave it.
Neither tensorboard, matplotlib nor torchvision is imported.

    torch.utils.tensorboard.SummaryWriter       EventWriter (events.py): the same event files written by hand; a histogram is a HIP
                                                kernel over the tensor where it lies (ops.histogram_tensorflow), an image one pack
                                                launch, and what leaves the device is copied behind the caller's stream"""

from __future__ import annotations

import os

import torch

from . import ops
from .events import EventWriter  # noqa: F401  (events.py: the writer kb.training.train opens)

COLORMAPS = tuple(ops.SUMMARY_COLORMAPS)   # the maps log_summary uses: 'viridis' (depths) and 'inferno' (errors)


def log(s, filepath=None, to_console=True):
    """reference src/log_utils.py:23-46: prints `s`, and writes it as a line into `filepath` -- a new file when the file's directory
    had to be made, appended otherwise."""
    if to_console:
        print(s)
    if filepath is not None:
        if not os.path.isdir(os.path.dirname(filepath)):
            os.makedirs(os.path.dirname(filepath))
            with open(filepath, "w+") as o:
                o.write(s + "\n")
        else:
            with open(filepath, "a+") as o:
                o.write(s + "\n")


def colorize(T, colormap="magma"):
    """reference src/log_utils.py:48-75 for an N x 1 x H x W fp32 tensor -> N x 3 x H x W fp32 on T's device: matplotlib's colours
    (Colormap.__call__ on float32: entry (int)(x * 256), entry 0 below 0, entry 255 from 1 on, black for NaN) looked up by a HIP
    kernel instead of a host round trip.  Serves the maps log_summary uses, 'viridis' and 'inferno'; any other name -- the
    reference's default 'magma' included -- raises ValueError.  A CPU tensor raises KbnError (no CPU fallback)."""
    if colormap not in COLORMAPS:
        raise ValueError(f"colorize: colormap {colormap!r} is not built in (have: {', '.join(COLORMAPS)})")
    return ops.summary_colorize(T, colormap)


def log_summary(max_predict_depth, summary_writer, tag, step, image0=None, image01=None, image02=None, output_depth0=None, sparse_depth0=None,
                validity_map0=None, ground_truth0=None, pose01=None, pose02=None, scalars={}, n_display=4):
    """KBNetModel.log_summary for a model with this max_predict_depth: the reference's calls on `summary_writer`, in its order --
    add_histogram (output depth, sparse depth, ground truth, the poses' translations; handed the tensors as they are), add_scalar
    for every item of `scalars`, add_image for the image panel and for the depth panel, each where the reference makes it and under
    the reference's tag string."""
    with torch.no_grad():
        image_text = depth_text = tag
        if image0 is not None:
            image_text += "_image0"
            depth_text += "_image0"
            if image01 is not None:
                image_text += "_image01-error"
            if image02 is not None:
                image_text += "_image02-error"
        image_panel = ops.summary_image_panel(image0, image01, image02, n_display=n_display)
        depth_panel = ops.summary_depth_panel(output_depth0, max_predict_depth, image0, sparse_depth0, validity_map0, ground_truth0,
                                              n_display=n_display)
        if output_depth0 is not None:
            depth_text += "_output0"
            summary_writer.add_histogram(tag + "_output_depth0_distro", output_depth0, global_step=step)
            if sparse_depth0 is not None and validity_map0 is not None:
                depth_text += "_sparse0-error"
                summary_writer.add_histogram(tag + "_sparse_depth0_distro", sparse_depth0, global_step=step)
            if ground_truth0 is not None:
                depth_text += "_groundtruth0-error"
                summary_writer.add_histogram(tag + "_ground_truth0_distro", torch.unsqueeze(ground_truth0[:, 0, :, :], dim=1), global_step=step)
        for pose, name in ((pose01, "01"), (pose02, "02")):
            if pose is not None:
                for row, axis in enumerate("xyz"):
                    summary_writer.add_histogram(tag + "_t" + axis + name + "_distro", pose[:, row, 3], global_step=step)
    for name, value in scalars.items():
        summary_writer.add_scalar(tag + "_" + name, value, global_step=step)
    if image_panel is not None:
        summary_writer.add_image(image_text, image_panel, global_step=step)
    if depth_panel is not None:
        summary_writer.add_image(depth_text, depth_panel, global_step=step)


# ------------------------------------------------------------------------------------------------ the settings log
# The six blocks the reference writes at the head of results.txt (run) and of its training log (train): src/kbnet.py:1032-1296.
# Character for character the reference's lines for the same arguments -- its quirks included: the doubled 'n_parameter=' text
# it builds and never logs, and log_system_settings' NameError when checkpoint_path is None.
def log_input_settings(log_path, n_batch=None, n_height=None, n_width=None, input_channels_image=3, input_channels_depth=2,
                       normalized_image_range=[0, 1], outlier_removal_kernel_size=7, outlier_removal_threshold=1.5):
    """reference src/kbnet.py:1032-1077; the batch line only when n_batch, n_height or n_width is given (training)."""
    # the reference appends two spaces after n_batch and after n_height whenever the text so far is not empty -- and never strips
    text = ""
    for name, value, spaced in (("n_batch", n_batch, True), ("n_height", n_height, True), ("n_width", n_width, False)):
        if value is not None:
            text += "{}={}".format(name, value)
        if spaced and len(text) > 0:
            text += "  "
    log("Input settings:", log_path)
    if n_batch is not None or n_height is not None or n_width is not None:
        log(text, log_path)
    log("input_channels_image={}  input_channels_depth={}".format(input_channels_image, input_channels_depth), log_path)
    log("normalized_image_range={}".format(normalized_image_range), log_path)
    log("outlier_removal_kernel_size={}  outlier_removal_threshold={:.2f}".format(outlier_removal_kernel_size, outlier_removal_threshold), log_path)
    log("", log_path)


def log_network_settings(log_path, min_pool_sizes_sparse_to_dense_pool, max_pool_sizes_sparse_to_dense_pool, n_convolution_sparse_to_dense_pool,
                         n_filter_sparse_to_dense_pool, n_filters_encoder_image, n_filters_encoder_depth, resolutions_backprojection,
                         n_filters_decoder, deconv_type, min_predict_depth, max_predict_depth, weight_initializer, activation_func,
                         parameters_depth_model=[], parameters_pose_model=[]):
    """reference src/kbnet.py:1079-1156."""
    n_parameter_depth = sum(p.numel() for p in parameters_depth_model)
    n_parameter_pose = sum(p.numel() for p in parameters_pose_model)
    n_parameter = n_parameter_depth + n_parameter_pose
    log("Sparse to dense pooling settings:", log_path)
    log("min_pool_sizes_sparse_to_dense_pool={}".format(min_pool_sizes_sparse_to_dense_pool), log_path)
    log("max_pool_sizes_sparse_to_dense_pool={}".format(max_pool_sizes_sparse_to_dense_pool), log_path)
    log("n_convolution_sparse_to_dense_pool={}".format(n_convolution_sparse_to_dense_pool), log_path)
    log("n_filter_sparse_to_dense_pool={}".format(n_filter_sparse_to_dense_pool), log_path)
    log("", log_path)
    log("Depth network settings:", log_path)
    log("n_filters_encoder_image={}".format(n_filters_encoder_image), log_path)
    log("n_filters_encoder_depth={}".format(n_filters_encoder_depth), log_path)
    log("resolutions_backprojection={}".format(resolutions_backprojection), log_path)
    log("n_filters_decoder={}".format(n_filters_decoder), log_path)
    log("deconv_type={}".format(deconv_type), log_path)
    log("min_predict_depth={:.2f}  max_predict_depth={:.2f}".format(min_predict_depth, max_predict_depth), log_path)
    log("", log_path)
    log("Weight settings:", log_path)
    log("n_parameter={}  n_parameter_depth={}  n_parameter_pose={}".format(n_parameter, n_parameter_depth, n_parameter_pose), log_path)
    log("weight_initializer={}  activation_func={}".format(weight_initializer, activation_func), log_path)
    log("", log_path)


def _schedule_text(n_train_sample, n_batch, schedule, values):
    return ", ".join("{}-{} : {}".format(ls * (n_train_sample // n_batch), le * (n_train_sample // n_batch), v)
                     for ls, le, v in zip([0] + schedule[:-1], schedule, values))


def log_training_settings(log_path, n_batch, n_train_sample, n_train_step, learning_rates, learning_schedule, augmentation_probabilities,
                          augmentation_schedule, augmentation_random_crop_type, augmentation_random_flip_type,
                          augmentation_random_remove_points, augmentation_random_noise_type, augmentation_random_noise_spread):
    """reference src/kbnet.py:1158-1200."""
    log("Training settings:", log_path)
    log("n_sample={}  n_epoch={}  n_step={}".format(n_train_sample, learning_schedule[-1], n_train_step), log_path)
    log("learning_schedule=[%s]" % _schedule_text(n_train_sample, n_batch, learning_schedule, learning_rates), log_path)
    log("", log_path)
    log("Augmentation settings:", log_path)
    log("augmentation_schedule=[%s]" % _schedule_text(n_train_sample, n_batch, augmentation_schedule, augmentation_probabilities), log_path)
    log("augmentation_random_crop_type={}".format(augmentation_random_crop_type), log_path)
    log("augmentation_random_flip_type={}".format(augmentation_random_flip_type), log_path)
    log("augmentation_random_remove_points={}".format(augmentation_random_remove_points), log_path)
    log("augmentation_random_noise_type={}  augmentation_random_noise_spread={}".format(
        augmentation_random_noise_type, augmentation_random_noise_spread), log_path)
    log("", log_path)


def log_loss_func_settings(log_path, w_color, w_structure, w_sparse_depth, w_smoothness, w_weight_decay_depth, w_weight_decay_pose):
    """reference src/kbnet.py:1202-1220."""
    log("Loss function settings:", log_path)
    log("w_color={:.1e}  w_structure={:.1e}  w_sparse_depth={:.1e}".format(w_color, w_structure, w_sparse_depth), log_path)
    log("w_smoothness={:.1e}".format(w_smoothness), log_path)
    log("w_weight_decay_depth={:.1e}  w_weight_decay_pose={:.1e}".format(w_weight_decay_depth, w_weight_decay_pose), log_path)
    log("", log_path)


def log_evaluation_settings(log_path, min_evaluate_depth, max_evaluate_depth):
    """reference src/kbnet.py:1222-1230."""
    log("Evaluation settings:", log_path)
    log("min_evaluate_depth={:.2f}  max_evaluate_depth={:.2f}".format(min_evaluate_depth, max_evaluate_depth), log_path)
    log("", log_path)


def log_system_settings(log_path, checkpoint_path, n_checkpoint=None, summary_event_path=None, n_summary=None, n_summary_display=None,
                        validation_start_step=None, depth_model_restore_path=None, pose_model_restore_path=None,
                        device=torch.device("cuda"), n_thread=8):
    """reference src/kbnet.py:1232-1296.  `device`: a torch.device (its .type is logged)."""
    log("Checkpoint settings:", log_path)
    if checkpoint_path is not None:
        log("checkpoint_path={}".format(checkpoint_path), log_path)
        if n_checkpoint is not None:
            log("checkpoint_save_frequency={}".format(n_checkpoint), log_path)
        if validation_start_step is not None:
            log("validation_start_step={}".format(validation_start_step), log_path)
        log("", log_path)
    if summary_event_path is not None:
        log("Tensorboard settings:", log_path)
        log("event_path={}".format(summary_event_path), log_path)
    if checkpoint_path is None:
        # the reference creates its summary text only under `checkpoint_path is not None` and fails at this point the same way
        raise NameError("name 'summary_settings_text' is not defined")
    # each given setting is followed by two spaces in the reference's text, the last one too
    summary_settings_text = "".join("{}={}  ".format(name, value) for name, value in
                                    (("log_summary_frequency", n_summary), ("n_summary_display", n_summary_display)) if value is not None)
    if len(summary_settings_text) > 0:
        log(summary_settings_text, log_path)
    if depth_model_restore_path is not None and depth_model_restore_path != "":
        log("depth_model_restore_path={}".format(depth_model_restore_path), log_path)
    if pose_model_restore_path is not None and pose_model_restore_path != "":
        log("pose_model_restore_path={}".format(pose_model_restore_path), log_path)
    log("", log_path)
    log("Hardware settings:", log_path)
    log("device={}".format(device.type), log_path)
    log("n_thread={}".format(n_thread), log_path)
    log("", log_path)
