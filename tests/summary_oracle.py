"""Host oracle of the training loop's image summaries (csrc/summary.hip, kb.summary, KBNetModel.log_summary).

Two independent statements of what the reference's log_summary (src/kbnet_model.py:417-650) puts into its two add_image calls:

  * NumPy, float32, operation by operation: the cells (photo_err, depth, rel_err), matplotlib's lookup (lookup) and
    torchvision's make_grid (grid) -> image_panel / depth_panel.  This is what the kernel is compared with, bit for bit.
  * torch on the CPU: the reference's own expressions (torch.mean, torch.where, tensor / python float, torch.cat), with a
    `colorize` callable handed in -- matplotlib's, through the reference's log_utils.colorize or restated -- and make_grid
    restated (torch_make_grid): torch_panels.  tests/test_summary_cpu.py holds the two against each other and against the
    golden file, which records log_utils.colorize itself.

The colour tables come from tests/golden/summary.npz: log_utils.colorize run on a ramp that hits every entry."""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "summary.npz")
EPSILON = 1e-8          # reference src/kbnet_model.py:21
MAPS = ("viridis", "inferno")

_golden = {}


def golden():
    if not _golden:
        _golden.update(np.load(GOLDEN))
    return _golden


def ramp():
    """256 float32 values, the k-th inside entry k's interval [k / 256, (k + 1) / 256): the input the golden's tables were recorded on."""
    return ((np.arange(256, dtype=np.float64) + 0.5) / 256.0).astype(np.float32)


def table(name):
    """256 x 3 float32: what the reference's colorize returned for ramp()."""
    return golden()["table::" + name]


# ------------------------------------------------------------------------------------------------ NumPy, float32
def lookup(x, name):
    """matplotlib's Colormap.__call__ on float32 data, x of any shape -> x.shape + (3,) float32."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = x * np.float32(256.0)
        index = np.where(t < 0, 0, np.where(t >= 256, 255, np.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0).astype(np.int64)))
    out = table(name)[index]
    out[np.isnan(t)] = 0.0
    return out


def photo_err(a, b, mistake=None):
    """x of PHOTO_ERR for N x 3 x H x W float32 a, b -> N x H x W.  mistake 'reciprocal': / 0.10f written as * (1 / 0.10f)."""
    e = np.abs(a - b)
    mean = ((e[:, 0] + e[:, 1]) + e[:, 2]) / np.float32(3.0)
    if mistake == "reciprocal":
        return mean * (np.float32(1.0) / np.float32(0.10))
    return mean / np.float32(0.10)


def depth_value(d, max_predict_depth):
    return d / np.float32(max_predict_depth)


def rel_err(out, ref, v):
    """x of REL_ERR for float32 arrays of one shape."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        rel = (np.abs(out - ref) + np.float32(EPSILON)) / (ref + np.float32(EPSILON))
        return np.where(v == np.float32(1.0), rel, v) / np.float32(0.05)


def _chw(rgb):
    """N x H x W x 3 -> N x 3 x H x W"""
    return np.ascontiguousarray(np.transpose(rgb, (0, 3, 1, 2)))


def grid(tiles, nrow, padding=2):
    """torchvision.utils.make_grid(tiles, nrow=nrow) for B x 3 x h x w float32 tiles (padding 2, pad_value 0; one tile comes back
    as it is), from its documented behaviour."""
    b, c, h, w = tiles.shape
    if b == 1:
        return tiles[0].copy()
    xmaps = min(nrow, b)
    ymaps = -(-b // xmaps)
    height, width = h + padding, w + padding
    out = np.zeros((c, height * ymaps + padding, width * xmaps + padding), dtype=np.float32)
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= b:
                break
            out[:, y * height + padding:y * height + padding + h, x * width + padding:x * width + padding + w] = tiles[k]
            k += 1
    return out


def _np(t):
    return None if t is None else np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float32)


def image_panel(image0, image01=None, image02=None, n_display=4, mistake=None):
    """What ops.summary_image_panel must return (3 x Hg x Wg float32), or None."""
    image0, image01, image02 = (None if t is None else _np(t)[:n_display] for t in (image0, image01, image02))
    rows = []
    if image0 is not None:
        rows.append(np.concatenate([image0, np.zeros_like(image0)], axis=3))
        for warped in (image01, image02):
            if warped is not None:
                rows.append(np.concatenate([warped, _chw(lookup(photo_err(image0, warped, mistake), "inferno"))], axis=3))
    return grid(np.concatenate(rows, axis=2), n_display) if len(rows) > 1 else None


def depth_panel(output_depth0, max_predict_depth, image0=None, sparse_depth0=None, validity_map0=None, ground_truth0=None, n_display=4):
    """What ops.summary_depth_panel must return, or None."""
    image0, out, sparse, validity, gt = (None if t is None else _np(t)[:n_display]
                                         for t in (image0, output_depth0, sparse_depth0, validity_map0, ground_truth0))
    rows = []
    if image0 is not None:
        rows.append(np.concatenate([image0, np.zeros_like(image0)], axis=3))
    if out is not None:
        left = _chw(lookup(depth_value(out[:, 0], max_predict_depth), "viridis"))
        rows.append(np.concatenate([left, np.zeros_like(left)], axis=3))
        pairs = []
        if sparse is not None and validity is not None:
            pairs.append((sparse[:, 0], validity[:, 0]))
        if gt is not None:
            pairs.append((gt[:, 0], gt[:, 1]))
        for ref, v in pairs:
            rows.append(np.concatenate([_chw(lookup(depth_value(ref, max_predict_depth), "viridis")),
                                        _chw(lookup(rel_err(out[:, 0], ref, v), "inferno"))], axis=3))
    return grid(np.concatenate(rows, axis=2), n_display) if len(rows) > 1 else None


def panel_shape(n_rows, frames, h, w):
    pad = 2 if frames > 1 else 0
    return 3, n_rows * h + 2 * pad, frames * (2 * w + pad) + pad


# ------------------------------------------------------------------------------------------------ torch on the CPU
def torch_make_grid(tensor, nrow):
    return torch.from_numpy(grid(tensor.numpy(), nrow))


def table_colorize(T, colormap):
    """log_utils.colorize restated on the recorded tables (for machines without matplotlib): N x 1 x H x W -> N x 3 x H x W."""
    return torch.from_numpy(_chw(lookup(T.numpy()[:, 0], colormap)))


def matplotlib_colorize(T, colormap):
    """log_utils.colorize restated on matplotlib itself (reference src/log_utils.py:48-75, with the colormap registry of current
    matplotlib in place of plt.cm.get_cmap)."""
    from matplotlib import colormaps
    cm = colormaps[colormap]
    color = np.stack([cm(T.numpy()[n, 0])[..., 0:3] for n in range(T.shape[0])], axis=0)
    return torch.from_numpy(np.transpose(color, (0, 3, 1, 2)).astype(np.float32))


def torch_panels(colorize, max_predict_depth, image0=None, image01=None, image02=None, output_depth0=None, sparse_depth0=None,
                 validity_map0=None, ground_truth0=None, n_display=4):
    """The reference's expressions (src/kbnet_model.py:468-617, 636-650) on CPU tensors -> (image panel or None, its tag suffix,
    depth panel or None, its tag suffix)."""
    display_summary_image, display_summary_depth = [], []
    image_text = depth_text = ""
    if image0 is not None:
        image0_summary = image0[0:n_display, ...]
        image_text += "_image0"
        depth_text += "_image0"
        display_summary_image.append(torch.cat([image0_summary, torch.zeros_like(image0_summary)], dim=-1))
        display_summary_depth.append(display_summary_image[-1])
    for warped, name in ((image01, "_image01-error"), (image02, "_image02-error")):
        if image0 is not None and warped is not None:
            warped_summary = warped[0:n_display, ...]
            image_text += name
            error = torch.mean(torch.abs(image0_summary - warped_summary), dim=1, keepdim=True)
            error = colorize(error / 0.10, "inferno")
            display_summary_image.append(torch.cat([warped_summary, error], dim=3))
    if output_depth0 is not None:
        output_depth0_summary = output_depth0[0:n_display, ...]
        depth_text += "_output0"
        n_batch, _, n_height, n_width = output_depth0_summary.shape
        display_summary_depth.append(torch.cat([colorize(output_depth0_summary / max_predict_depth, "viridis"),
                                                torch.zeros(n_batch, 3, n_height, n_width)], dim=3))
    pairs = []
    if output_depth0 is not None and sparse_depth0 is not None and validity_map0 is not None:
        pairs.append((sparse_depth0[0:n_display], validity_map0[0:n_display], "_sparse0-error"))
    if output_depth0 is not None and ground_truth0 is not None:
        pairs.append((torch.unsqueeze(ground_truth0[:, 0, :, :], dim=1)[0:n_display], torch.unsqueeze(ground_truth0[:, 1, :, :], dim=1)[0:n_display],
                      "_groundtruth0-error"))
    for ref_summary, validity_summary, name in pairs:
        depth_text += name
        error = torch.abs(output_depth0_summary - ref_summary)
        error = torch.where(validity_summary == 1.0, (error + EPSILON) / (ref_summary + EPSILON), validity_summary)
        display_summary_depth.append(torch.cat([colorize(ref_summary / max_predict_depth, "viridis"), colorize(error / 0.05, "inferno")], dim=3))
    image = torch_make_grid(torch.cat(display_summary_image, dim=2), n_display) if len(display_summary_image) > 1 else None
    depth = torch_make_grid(torch.cat(display_summary_depth, dim=2), n_display) if len(display_summary_depth) > 1 else None
    return image, image_text, depth, depth_text


def expected_calls(max_predict_depth, tag, step, image0=None, image01=None, image02=None, output_depth0=None, sparse_depth0=None,
                   validity_map0=None, ground_truth0=None, pose01=None, pose02=None, scalars={}, n_display=4):
    """The reference's calls on the writer, in its order (src/kbnet_model.py:550-650): (method, tag, payload, step); the payload of
    an add_image is the oracle's panel (NumPy), that of an add_histogram the tensor the reference hands over."""
    calls = []
    if output_depth0 is not None:
        calls.append(("add_histogram", tag + "_output_depth0_distro", output_depth0, step))
        if sparse_depth0 is not None and validity_map0 is not None:
            calls.append(("add_histogram", tag + "_sparse_depth0_distro", sparse_depth0, step))
        if ground_truth0 is not None:
            calls.append(("add_histogram", tag + "_ground_truth0_distro", torch.unsqueeze(ground_truth0[:, 0, :, :], dim=1), step))
    for pose, name in ((pose01, "01"), (pose02, "02")):
        if pose is not None:
            for row, axis in enumerate("xyz"):
                calls.append(("add_histogram", tag + "_t" + axis + name + "_distro", pose[:, row, 3], step))
    for name, value in scalars.items():
        calls.append(("add_scalar", tag + "_" + name, value, step))
    image_text = depth_text = tag
    if image0 is not None:
        image_text += "_image0" + ("_image01-error" if image01 is not None else "") + ("_image02-error" if image02 is not None else "")
        depth_text += "_image0"
    if output_depth0 is not None:
        depth_text += "_output0" + ("_sparse0-error" if sparse_depth0 is not None and validity_map0 is not None else "") + \
            ("_groundtruth0-error" if ground_truth0 is not None else "")
    panel = image_panel(image0, image01, image02, n_display)
    if panel is not None:
        calls.append(("add_image", image_text, panel, step))
    panel = depth_panel(output_depth0, max_predict_depth, image0, sparse_depth0, validity_map0, ground_truth0, n_display)
    if panel is not None:
        calls.append(("add_image", depth_text, panel, step))
    return calls


# ------------------------------------------------------------------------------------------------ inputs
EDGE_VALUES = np.array([-1.0, -0.0, 0.0, 1.0, 1.5, np.inf, -np.inf, np.nan, 255.0 / 256.0, np.nextafter(np.float32(1.0), np.float32(0.0))],
                       dtype=np.float32)


def case(n, h, w, seed=0, edges=False, max_predict_depth=100.0):
    """The tensors of one log_summary call as CPU fp32 tensors: images in [0, 1], a warped pair close to image0 (errors spread over
    the inferno map), depths up to a little above max_predict_depth, a sparse depth map with its validity map, a ground truth of two
    planes.  `edges`: the lookup's edge values scattered over the depths and the images, and a validity map of 0, 1 and 0.5."""
    rng = np.random.default_rng(seed)
    f = lambda a: a.astype(np.float32)
    image0 = f(rng.random((n, 3, h, w)))
    image01 = f(np.clip(image0 + rng.normal(0, 0.06, image0.shape), 0, 1))
    image02 = f(np.clip(image0 + rng.normal(0, 0.12, image0.shape), 0, 1))
    output = f(rng.uniform(1.5, 1.05 * max_predict_depth, (n, 1, h, w)))
    validity = f(rng.random((n, 1, h, w)) < 0.4)
    sparse = f(output * rng.uniform(0.9, 1.1, output.shape)) * validity
    gt_validity = f(rng.random((n, 1, h, w)) < 0.6)
    gt = np.concatenate([f(output * rng.uniform(0.93, 1.07, output.shape)) * gt_validity, gt_validity], axis=1)
    if edges:
        for a in (output, sparse, gt[:, 0:1], image01):
            where = rng.random(a.shape) < 0.15
            a[where] = rng.choice(EDGE_VALUES, size=int(where.sum()))
        for v in (validity, gt[:, 1:2]):
            v[...] = rng.choice(np.array([0.0, 1.0, 0.5], dtype=np.float32), size=v.shape)
    t = torch.from_numpy
    return dict(image0=t(image0), image01=t(image01), image02=t(image02), output_depth0=t(output), sparse_depth0=t(sparse),
                validity_map0=t(validity), ground_truth0=t(np.ascontiguousarray(gt)))
