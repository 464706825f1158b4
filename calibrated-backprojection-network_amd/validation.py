"""In-training validation: the reference's validate() (src/kbnet.py:520-674), called every n_checkpoint steps from its training loop
(:483-501), on this package's device path.

    reference, per frame (batch 1)                          here, per batch of any size
    validity map, outlier removal, transforms.transform     ops.preprocess: one launch
    depth_model.forward                                     the fused forward under no_grad, on the UNFILTERED sparse depth and the
                                                            filtered validity map, as the reference
    .cpu().numpy(), mask, four NumPy metrics                ops.eval_metrics: the frame's four metrics stay on the device
    np.mean over the frames, log lines, best_results        one copy of the N x 4 rows to the host at the end, then the same

The model is never switched with train() / eval() here: the reference's loop does that around the call (src/kbnet.py:485, 504), and
KBNetModel has no second mode (no BatchNorm, no dropout; its train() raises).  One process validates on one GPU: the frames are not
sharded over ranks, and under kb.dist every rank that calls validate() runs all of them."""

from __future__ import annotations

import numpy as np
import torch

from . import ops
from ._lib import KbnError
from .summary import log

METRICS = ("mae", "rmse", "imae", "irmse")


def update_best_results(best_results, step, mae, rmse, imae, irmse):
    """The reference's rule (src/kbnet.py:646-661) as a function of its inputs: a metric improved when np.round(value, 2) <=
    np.round(best, 2); with MORE THAN TWO of the four improved, step and all four values replace the best ones.  Returns a new dict
    (the other keys of `best_results` kept); `best_results` itself is left as it was."""
    values = dict(zip(METRICS, (mae, rmse, imae, irmse)))
    n_improve = sum(1 for k in METRICS if np.round(values[k], 2) <= np.round(best_results[k], 2))
    best = dict(best_results)
    if n_improve > 2:
        best["step"] = step
        best.update(values)
    return best


def _ground_truth_batch(ground_truths, first: int, n: int, device):
    """Frames first .. first + n - 1 as an n x 2 x H x W fp32 device tensor, from the reference's list of H x W x 2 arrays (what
    data_utils.load_depth_with_validity_map gives, src/kbnet.py:556-558) or from one N x 2 x H x W tensor."""
    if first + n > len(ground_truths):
        raise KbnError(f"validate: {len(ground_truths)} ground truths, but the loader delivered frame {first + n - 1}")
    if isinstance(ground_truths, torch.Tensor):
        batch = ground_truths[first:first + n]
    else:
        batch = torch.from_numpy(np.stack([np.transpose(np.asarray(g), (2, 0, 1)) for g in ground_truths[first:first + n]], axis=0))
    if batch.dim() != 4 or batch.shape[1] != 2:
        raise KbnError(f"validate: a ground truth is depth and validity map, H x W x 2 in a list or N x 2 x H x W as a tensor; got {tuple(batch.shape)}")
    return batch.to(device=device, dtype=torch.float32)


@torch.no_grad()
def validate(depth_model, dataloader, ground_truths, step, best_results, min_evaluate_depth, max_evaluate_depth, device, summary_writer=None,
             n_summary_display=4, n_summary_display_interval=250, log_path=None, outlier_removal_kernel_size=7, outlier_removal_threshold=1.5,
             normalized_image_range=(0, 1), return_metrics=False):
    """The reference's validate() (src/kbnet.py:520-674) -> best_results, or (best_results, N x 4 fp64 host tensor of each frame's
    MAE, RMSE [mm], iMAE, iRMSE [1/km]) with return_metrics.

    dataloader: any iterable of (image in 0..255, sparse_depth, intrinsics) batches of any size -- kb.loader.InferenceFrameLoader
    fits.  The reference's `transforms` and `outlier_removal` objects are their settings here (normalized_image_range,
    outlier_removal_kernel_size, outlier_removal_threshold).  ground_truths: frame by frame in the loader's order, a list of
    H x W x 2 arrays (depth, validity map) or one N x 2 x H x W tensor; fewer or more of them than frames raises KbnError (the
    reference's zip stops at the shorter and averages zeros for the rest).

    The metrics are the mean over the FRAMES of each frame's metric, whatever the batch size.  Every n_summary_display_interval-th
    frame goes to depth_model.log_summary(tag='eval') when a summary_writer is given.  The log lines and the best_results rule
    (update_best_results) are the reference's.  The device is waited for once, by the copy of the N x 4 rows."""
    rows = []
    shown = [[], [], [], [], []]   # image, output depth, filtered sparse depth, filtered validity map, ground truth
    seen = 0
    for inputs in dataloader:
        image, sparse_depth, intrinsics = [in_.to(device) for in_ in inputs]
        n = image.shape[0]
        ground_truth = _ground_truth_batch(ground_truths, seen, n, device)
        image, filtered_validity_map, filtered_sparse_depth = ops.preprocess(
            image, sparse_depth, kernel_size=outlier_removal_kernel_size, threshold=outlier_removal_threshold,
            normalized_image_range=normalized_image_range)
        output_depth = depth_model.forward(image=image, sparse_depth=sparse_depth, validity_map_depth=filtered_validity_map,
                                           intrinsics=intrinsics)
        if summary_writer is not None:
            for i in range(n):
                if (seen + i) % n_summary_display_interval == 0:
                    for lst, t in zip(shown, (image, output_depth, filtered_sparse_depth, filtered_validity_map, ground_truth)):
                        lst.append(t[i:i + 1])
        rows.append(ops.eval_metrics(output_depth, ground_truth[:, 0], ground_truth[:, 1], min_evaluate_depth, max_evaluate_depth))
        seen += n
    if seen == 0:
        raise KbnError("validate: the loader delivered no frame")
    if seen != len(ground_truths):
        raise KbnError(f"validate: {len(ground_truths)} ground truths for the loader's {seen} frames")
    per_frame = torch.cat(rows, dim=0).cpu()   # the one copy to the host
    mae, rmse, imae, irmse = (np.mean(column) for column in per_frame.numpy().T)

    if summary_writer is not None:
        depth_model.log_summary(
            summary_writer=summary_writer, tag="eval", step=step, image0=torch.cat(shown[0], dim=0), output_depth0=torch.cat(shown[1], dim=0),
            sparse_depth0=torch.cat(shown[2], dim=0), validity_map0=torch.cat(shown[3], dim=0), ground_truth0=torch.cat(shown[4], dim=0),
            scalars={"mae": mae, "rmse": rmse, "imae": imae, "irmse": irmse}, n_display=n_summary_display)

    header = "{:>8}  {:>8}  {:>8}  {:>8}  {:>8}".format("Step", "MAE", "RMSE", "iMAE", "iRMSE")
    line = "{:8}  {:8.3f}  {:8.3f}  {:8.3f}  {:8.3f}"
    log("Validation results:", log_path)
    log(header, log_path)
    log(line.format(step, mae, rmse, imae, irmse), log_path)
    best_results = update_best_results(best_results, step, mae, rmse, imae, irmse)
    log("Best results:", log_path)
    log(header, log_path)
    log(line.format(best_results["step"], best_results["mae"], best_results["rmse"], best_results["imae"], best_results["irmse"]), log_path)
    return (best_results, per_frame) if return_metrics else best_results
