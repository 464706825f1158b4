"""CPU oracle of the objective's forward value (KBNetModel.compute_loss): test infrastructure, never imported by the package.

A functional restatement of what the reference computes in src/kbnet_model.py:188-304 with src/net_utils.py:1601-1739 and
src/losses.py, written against the arithmetic and not against its code.  Everything runs in the dtype (and on the device) of
`image0`: fp32 gives what a user of the reference gets, fp64 gives the value both are measured against.

    points  = K^-1 [x y 1]^T z                         (homogeneous, 4 x HW)
    xy      = (T p)[0:2] / ((T p)[2] + 1e-7),  T = rows 0-2 of (K | 0) pose
    warp    = bilinear sample at xy, border padding, align_corners, through normalised coordinates
              x / (W-1), 2 (t - 0.5) -- the round trip decides the last bits of the sample position in fp32
    colour  = mean_n sum_chw |warp - image0| / (H W)           (3 channels over a 1-channel weight sum: 3 x a mean)
    ssim    = clamp((1 - score) / 2, 0, 1) on 3 x 3 unpadded means, stretched (H-2) x (W-2) -> H x W by nearest
    sparse  = mean_n sum v |sparse - depth| / sum v            (NaN for a frame without a valid point)
    smooth  = mean exp(-mean_c |dx image0|) |dx depth| + the same in y
"""
import torch
import torch.nn.functional as F

W_COLOR, W_STRUCTURE, W_SPARSE_DEPTH, W_SMOOTHNESS = 0.15, 0.95, 0.60, 0.04


def pose_matrix(v):
    """N x 6 (axis-angle rotation, then translation) -> N x 4 x 4: Rodrigues with axis = r / (|r| + 1e-7), translation in column 3."""
    r, t = v[:, :3], v[:, 3:]
    angle = r.norm(dim=1, keepdim=True)
    x, y, z = (r / (angle + 1e-7)).unbind(1)
    ca, sa = torch.cos(angle[:, 0]), torch.sin(angle[:, 0])
    c = 1 - ca
    m = torch.zeros(v.shape[0], 4, 4, dtype=v.dtype, device=v.device)
    m[:, 0, 0], m[:, 0, 1], m[:, 0, 2] = x * (x * c) + ca, x * (y * c) - z * sa, z * (x * c) + y * sa
    m[:, 1, 0], m[:, 1, 1], m[:, 1, 2] = x * (y * c) + z * sa, y * (y * c) + ca, y * (z * c) - x * sa
    m[:, 2, 0], m[:, 2, 1], m[:, 2, 2] = z * (x * c) - y * sa, y * (z * c) + x * sa, z * (z * c) + ca
    m[:, :3, 3] = t
    m[:, 3, 3] = 1
    return m


def backproject(depth, intrinsics):
    """N x 1 x H x W depth -> N x 4 x HW homogeneous camera points."""
    n, _, h, w = depth.shape
    kw = dict(dtype=depth.dtype, device=depth.device)
    ys, xs = torch.meshgrid(torch.linspace(0.0, h - 1, h, **kw), torch.linspace(0.0, w - 1, w, **kw), indexing="ij")
    pix = torch.stack([xs, ys, torch.ones_like(xs)], 0).reshape(1, 3, h * w).repeat(n, 1, 1)
    z = depth.reshape(n, 1, h * w)
    return torch.cat([torch.matmul(torch.inverse(intrinsics), pix) * z, torch.ones_like(z)], 1)


def project(points, pose, intrinsics, height, width):
    """N x 4 x HW points -> N x 2 x H x W pixel positions in the frame `pose` leads to."""
    n = points.shape[0]
    k4 = torch.zeros(n, 4, 4, dtype=points.dtype, device=points.device)
    k4[:, :3, :3] = intrinsics
    k4[:, 3, 3] = 1
    q = torch.matmul(torch.matmul(k4, pose)[:, :3], points)
    return (q / (q[:, 2:3] + 1e-7))[:, :2].reshape(n, 2, height, width)


def warp(image, xy):
    """Bilinear border sampling of `image` at the pixel positions `xy` (N x 2 x H x W), through normalised coordinates."""
    h, w = image.shape[2:]
    g = xy.permute(0, 2, 3, 1).clone()
    g[..., 0] /= (w - 1.0)
    g[..., 1] /= (h - 1.0)
    return F.grid_sample(image, 2.0 * (g - 0.5), mode="bilinear", padding_mode="border", align_corners=True)


def ssim_distance(x, y):
    """N x C x (H-2) x (W-2): clamp((1 - SSIM) / 2, 0, 1) on unpadded 3 x 3 means."""
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    pool = lambda t: F.avg_pool2d(t, 3, 1)
    mu_x, mu_y = pool(x), pool(y)
    mu_xy, mu_xx, mu_yy = mu_x * mu_y, mu_x ** 2, mu_y ** 2
    sg_x, sg_y, sg_xy = pool(x ** 2) - mu_xx, pool(y ** 2) - mu_yy, pool(x * y) - mu_xy
    score = ((2 * mu_xy + c1) * (2 * sg_xy + c2)) / ((mu_xx + mu_yy + c1) * (sg_x + sg_y + c2))
    return torch.clamp((1.0 - score) / 2.0, 0.0, 1.0)


def _frame_sums(t):
    return t.sum(dim=(1, 2, 3))


def _gradients(t):
    return t[..., :, :-1] - t[..., :, 1:], t[..., :-1, :] - t[..., 1:, :]


def _pixel_maps(image0, image01, image02, depth, sparse, validity):
    """The eight per-pixel maps whose per-frame sums the kernel returns, in its order: |image01 - image0|, |image02 - image0|,
    the two stretched SSIM distances, v |sparse - depth|, v, wx |dx depth| (N x 1 x H x (W-1)), wy |dy depth| (N x 1 x (H-1) x W)."""
    h, w = image0.shape[2:]
    c = [(image0 - im).abs() for im in (image01, image02)]
    s = [F.interpolate(ssim_distance(im, image0), size=(h, w), mode="nearest") for im in (image01, image02)]
    ix, iy = _gradients(image0)
    dx, dy = _gradients(depth)
    sx = torch.exp(-ix.abs().mean(1, keepdim=True)) * dx.abs()
    sy = torch.exp(-iy.abs().mean(1, keepdim=True)) * dy.abs()
    return c[0], c[1], s[0], s[1], validity * (sparse - depth).abs(), validity, sx, sy


def frame_sums(image0, image01, image02, depth, sparse, validity):
    """-> N x 8, in the dtype of the inputs: what kbn_photometric_loss_forward writes for each frame (ops.photometric_loss),
    { sum |image01 - image0|, sum |image02 - image0|, sum ssim01, sum ssim02, sum v |sparse - depth|, sum v, sum wx |dx depth|,
    sum wy |dy depth| }."""
    return torch.stack([_frame_sums(m) for m in _pixel_maps(image0, image01, image02, depth, sparse, validity)], 1)


def loss_sums(image0, image1, image2, depth, sparse, validity, intrinsics, pose01, pose02):
    """compute_loss's arguments -> frame_sums of its two warped images."""
    h, w = image0.shape[2:]
    points = backproject(depth, intrinsics)
    image01 = warp(image1, project(points, pose01, intrinsics, h, w))
    image02 = warp(image2, project(points, pose02, intrinsics, h, w))
    return frame_sums(image0, image01, image02, depth, sparse, validity)


def loss_terms(image0, image01, image02, depth, sparse, validity):
    """-> (terms, per_frame): the batch's (colour, structure, sparse depth, smoothness) as 0-dim tensors, formed in the order the
    reference forms them (each pair's batch mean first, the smoothness means over the whole batch), and the N x 4 terms of each
    frame.  The column means of per_frame equal the batch terms up to rounding."""
    h, w = image0.shape[2:]
    hw = float(h * w)
    c01, c02, s01, s02, spd, v, sx, sy = _pixel_maps(image0, image01, image02, depth, sparse, validity)
    c = [_frame_sums(m) / hw for m in (c01, c02)]
    s = [_frame_sums(m) / hw for m in (s01, s02)]
    sp = _frame_sums(spd) / _frame_sums(v)
    terms = (c[0].mean() + c[1].mean(), s[0].mean() + s[1].mean(), sp.mean(), sx.mean() + sy.mean())
    per_frame = torch.stack([c[0] + c[1], s[0] + s[1], sp, sx.mean(dim=(1, 2, 3)) + sy.mean(dim=(1, 2, 3))], 1)
    return terms, per_frame


def compute_loss(image0, image1, image2, depth, sparse, validity, intrinsics, pose01, pose02, w_color=W_COLOR,
                 w_structure=W_STRUCTURE, w_sparse_depth=W_SPARSE_DEPTH, w_smoothness=W_SMOOTHNESS):
    """-> dict: loss_color, loss_structure, loss_sparse_depth, loss_smoothness, loss (0-dim), image01, image02, per_frame (N x 4)."""
    h, w = image0.shape[2:]
    points = backproject(depth, intrinsics)
    image01 = warp(image1, project(points, pose01, intrinsics, h, w))
    image02 = warp(image2, project(points, pose02, intrinsics, h, w))
    (color, structure, sparse_term, smooth), per_frame = loss_terms(image0, image01, image02, depth, sparse, validity)
    loss = w_color * color + w_structure * structure + w_sparse_depth * sparse_term + w_smoothness * smooth
    return {"loss_color": color, "loss_structure": structure, "loss_sparse_depth": sparse_term, "loss_smoothness": smooth,
            "loss": loss, "image01": image01, "image02": image02, "per_frame": per_frame}
