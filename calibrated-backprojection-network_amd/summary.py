"""The training loop's monitoring: what the reference's loop calls between optimizer.step() and save_model besides validate()
(validation.py) -- KBNetModel.log_summary (reference src/kbnet_model.py:417-650) and the two helpers of src/log_utils.py.

    reference                                   here
    log_utils.log(s, filepath, to_console)      log: the same lines into the same file
    log_utils.colorize(T, colormap)             colorize: matplotlib's lookup as a HIP kernel, on T's device
    KBNetModel.log_summary(...)                 log_summary (KBNetModel.log_summary calls it): the same add_histogram / add_scalar /
                                                add_image calls, the two image panels written by one launch each
                                                (ops.summary_image_panel, ops.summary_depth_panel)

The reference copies every tensor to the host, colourises frame by frame through matplotlib, concatenates on the CPU and calls
torchvision.utils.make_grid.  Here a panel is one kernel launch and stays on the device; the writer -- any object with add_image,
add_histogram and add_scalar, TensorBoard's SummaryWriter among them -- is handed device tensors and decides when they leave it.
Neither tensorboard, matplotlib nor torchvision is imported."""

from __future__ import annotations

import os

import torch

from . import ops

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
