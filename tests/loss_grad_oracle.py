"""Closed-form backward of the objective, WITHOUT autograd: test infrastructure, never imported by the package.

tests/loss_oracle.py under torch.autograd is the definition of the gradient; this file restates that gradient operation by
operation, the way csrc/loss_backward.hip computes it, so that (a) the kernel has arithmetic to be written against and (b) a
deliberate mistake of the kind one can make in the kernel can be planted in one place (tests/test_loss_grad_power_cpu.py).

    backward(args, grad_sums) -> grad_depth (N x 1 x H x W), grad_pose01, grad_pose02 (N x 4 x 4, row 3 zero)

`args`: the nine arguments of compute_loss, poses as matrices; `grad_sums`: N x 8, the gradient of the N x 8 sums of
loss_oracle.loss_sums (column 5, sum v, depends on nothing differentiable).  Everything runs in the dtype of image0.

Kinks.  Where a pixel sits exactly on a kink torch's convention wins and is followed here:
  abs        sgn(0) = 0
  clamp      the gradient passes where 0 <= v <= 1, both ends included
  grid_sample (border padding)  the gradient with respect to the sample position is zero where the position is <= 0 or
             >= size - 1: the border itself counts as outside
  floor      the position's integer part has no gradient

`mistakes`: a set of names from MISTAKES; each plants one error.
"""
import torch
import torch.nn.functional as F

TILE_H, TILE_W = 16, 64     # csrc/loss_backward.hip: the tile a workgroup owns ("halo of 1" needs to know the seams)

MISTAKES = (
    "gradient kept where the position was clamped",
    "-(g_u u + g_v v) / d dropped",
    "d without the 1e-7",
    "frame 0's K for every frame",
    "K instead of K^T in the pose gradient",
    "SSIM coefficient C dropped",
    "stretch weights ignored",
    "halo of 1 instead of 2",
    "smoothness sign flipped for the left / upper neighbour",
    "validity weight squared",
    "validity weight dropped",
    "pair 1 accumulated into pose01",
)


INVISIBLE = ("d without the 1e-7",)      # no case has a point within 0.1 of the camera plane: it moves a gradient by ~1e-6


def stretch_weights(size, dtype=torch.float64):
    """How many of the `size` output pixels torch's nearest interpolation copies each of the size - 2 SSIM scores to."""
    src = torch.arange(size - 2, dtype=torch.float64).reshape(1, 1, -1, 1)
    idx = F.interpolate(src, size=(size, 1), mode="nearest").reshape(-1).long()
    return torch.bincount(idx, minlength=size - 2).to(dtype)


def _ssim_image_gradient(x, y, weight, mistakes):
    """d(sum of the stretched SSIM distance) / dx: x the warped image, y image0 (N x 3 x H x W), weight N x 1 x (H-2) x (W-2),
    the upstream gradient times the stretch weight of every window."""
    n, _, h, w = x.shape
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    pool = lambda t: F.avg_pool2d(t, 3, 1)
    mu_x, mu_y = pool(x), pool(y)
    sg_x, sg_y, sg_xy = pool(x * x) - mu_x * mu_x, pool(y * y) - mu_y * mu_y, pool(x * y) - mu_x * mu_y
    n1, n2 = 2 * mu_x * mu_y + c1, 2 * sg_xy + c2
    d1, d2 = mu_x * mu_x + mu_y * mu_y + c1, sg_x + sg_y + c2
    den = d1 * d2
    score = n1 * n2 / den
    v = (1.0 - score) / 2.0
    # dv/dx_p = -1/2 dS/dx_p,  dS/dx_p = [2 mu_y n2 + 2 n1 (y_p - mu_y) - S (2 mu_x d2 + 2 d1 (x_p - mu_x))] / (9 D)
    coef = torch.where((v >= 0) & (v <= 1), -0.5 * weight, torch.zeros_like(v)) / (9.0 * den)
    b = coef * (-2.0 * score * d1)
    c = coef * (2.0 * n1)
    a = coef * (2.0 * mu_y * n2 - 2.0 * score * mu_x * d2) - b * mu_x - c * mu_y
    if "SSIM coefficient C dropped" in mistakes:
        c = torch.zeros_like(c)
    g = torch.zeros_like(x)
    cy, cx = torch.meshgrid(torch.arange(1, h - 1), torch.arange(1, w - 1), indexing="ij")      # the window centres
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            sl = (slice(None), slice(None), slice(1 + dy, h - 1 + dy), slice(1 + dx, w - 1 + dx))
            term = a + b * x[sl] + c * y[sl]
            if "halo of 1 instead of 2" in mistakes:     # a window centred in another tile than the pixel is missing
                same = ((cy + dy) // TILE_H == cy // TILE_H) & ((cx + dx) // TILE_W == cx // TILE_W)
                term = term * same.to(term.dtype)
            g[sl] += term
    return g


def _pair(image0, src, depth, k, pose, gs_color, gs_ssim, mistakes):
    """One neighbour frame: -> (d/d depth N x 1 x H x W, d/d T N x 3 x 4), T = rows 0-2 of (K | 0) pose."""
    n, _, h, w = image0.shape
    kw = dict(dtype=image0.dtype, device=image0.device)
    eps = 0.0 if "d without the 1e-7" in mistakes else 1e-7
    ys, xs = torch.meshgrid(torch.linspace(0.0, h - 1, h, **kw), torch.linspace(0.0, w - 1, w, **kw), indexing="ij")
    pix = torch.stack([xs, ys, torch.ones_like(xs)], 0).reshape(1, 3, h * w)
    ray = torch.matmul(torch.inverse(k), pix)                                    # N x 3 x HW
    z = depth.reshape(n, 1, h * w)
    p = torch.cat([ray * z, torch.ones_like(z)], 1)                              # N x 4 x HW
    t = torch.matmul(k, pose[:, :3])                                             # N x 3 x 4
    q = torch.matmul(t, p)
    d = q[:, 2] + eps
    u, v = q[:, 0] / d, q[:, 1] / d
    # the forward's round trip through normalised coordinates; its derivative is 1
    ix = ((2.0 * (u / (w - 1.0) - 0.5) + 1.0) / 2.0) * (w - 1.0)
    iy = ((2.0 * (v / (h - 1.0) - 0.5) + 1.0) / 2.0) * (h - 1.0)
    in_x, in_y = (ix > 0) & (ix < w - 1), (iy > 0) & (iy < h - 1)                # torch: the border counts as outside
    if "gradient kept where the position was clamped" in mistakes:
        in_x, in_y = torch.ones_like(in_x), torch.ones_like(in_y)
    ix, iy = ix.clamp(0, w - 1), iy.clamp(0, h - 1)
    fx0, fy0 = ix.floor(), iy.floor()
    xa, ya = fx0.long(), fy0.long()
    flat = src.reshape(n, 3, h * w)

    def tap(yy, xx):
        inside = ((xx <= w - 1) & (yy <= h - 1)).to(src.dtype)                   # a tap outside the image counts as 0
        idx = (yy.clamp(max=h - 1) * w + xx.clamp(max=w - 1))[:, None].expand(n, 3, h * w)
        return torch.gather(flat, 2, idx) * inside[:, None]
    nw, ne, sw, se = tap(ya, xa), tap(ya, xa + 1), tap(ya + 1, xa), tap(ya + 1, xa + 1)
    ax, ay = (ix - fx0)[:, None], (iy - fy0)[:, None]
    warped = (nw * (1 - ax) + ne * ax) * (1 - ay) + (sw * (1 - ax) + se * ax) * ay
    dw_dx = (ne - nw) * (1 - ay) + (se - sw) * ay
    dw_dy = (sw - nw) * (1 - ax) + (se - ne) * ax

    x4, y4 = warped.reshape(n, 3, h, w), image0
    g_w = gs_color.reshape(n, 1, 1, 1) * torch.sign(x4 - y4)
    wy, wx = stretch_weights(h, image0.dtype).to(image0.device), stretch_weights(w, image0.dtype).to(image0.device)
    weight = wy[:, None] * wx[None, :]
    if "stretch weights ignored" in mistakes:
        weight = torch.ones_like(weight)
    g_w = g_w + _ssim_image_gradient(x4, y4, gs_ssim.reshape(n, 1, 1, 1) * weight[None, None], mistakes)
    g_w = g_w.reshape(n, 3, h * w)

    g_u = (g_w * dw_dx).sum(1) * in_x.to(src.dtype)
    g_v = (g_w * dw_dy).sum(1) * in_y.to(src.dtype)
    g_q2 = -(g_u * u + g_v * v) / d
    if "-(g_u u + g_v v) / d dropped" in mistakes:
        g_q2 = torch.zeros_like(g_q2)
    g_q = torch.stack([g_u / d, g_v / d, g_q2], 1)                               # N x 3 x HW
    g_z = (g_q * torch.matmul(t[:, :, :3], ray)).sum(1)
    g_t = torch.matmul(g_q, p.transpose(1, 2))                                   # N x 3 x 4
    return g_z.reshape(n, 1, h, w), g_t


def backward(args, grad_sums, mistakes=()):
    image0, image1, image2, depth, sparse, validity, k, pose01, pose02 = args
    mistakes = set(mistakes)
    assert mistakes <= set(MISTAKES), mistakes - set(MISTAKES)
    n, _, h, w = image0.shape
    gs = grad_sums.to(image0.dtype)
    k_used = k[:1].expand_as(k) if "frame 0's K for every frame" in mistakes else k

    g_depth = torch.zeros_like(depth)
    g_pose = []
    for pair, (src, pose) in enumerate(((image1, pose01), (image2, pose02))):
        g_z, g_t = _pair(image0, src, depth, k_used, pose, gs[:, pair], gs[:, 2 + pair], mistakes)
        g_depth = g_depth + g_z
        kt = k_used if "K instead of K^T in the pose gradient" in mistakes else k_used.transpose(1, 2)
        gp = torch.zeros_like(pose)
        gp[:, :3] = torch.matmul(kt, g_t)
        g_pose.append(gp)
    if "pair 1 accumulated into pose01" in mistakes:
        g_pose = [g_pose[0] + g_pose[1], torch.zeros_like(g_pose[1])]

    # sparse depth: gs[4] v sgn(z - sparse)
    vw = validity
    if "validity weight squared" in mistakes:
        vw = validity * validity
    if "validity weight dropped" in mistakes:
        vw = torch.ones_like(validity)
    g_depth = g_depth + gs[:, 4].reshape(n, 1, 1, 1) * vw * torch.sign(depth - sparse)

    # smoothness: every neighbouring pair (p, p + 1) gives +w sgn to p and -w sgn to p + 1
    flip = -1.0 if "smoothness sign flipped for the left / upper neighbour" in mistakes else 1.0
    wx = torch.exp(-(image0[..., :, :-1] - image0[..., :, 1:]).abs().mean(1, keepdim=True))
    wy = torch.exp(-(image0[..., :-1, :] - image0[..., 1:, :]).abs().mean(1, keepdim=True))
    sx = gs[:, 6].reshape(n, 1, 1, 1) * wx * torch.sign(depth[..., :, :-1] - depth[..., :, 1:])
    sy = gs[:, 7].reshape(n, 1, 1, 1) * wy * torch.sign(depth[..., :-1, :] - depth[..., 1:, :])
    g_depth = g_depth.clone()
    g_depth[..., :, :-1] += sx
    g_depth[..., :, 1:] -= flip * sx
    g_depth[..., :-1, :] += sy
    g_depth[..., 1:, :] -= flip * sy
    return g_depth, g_pose[0], g_pose[1]


def autograd(args, grad_sums, loss_sums):
    """The definition: torch.autograd through `loss_sums` (loss_oracle.loss_sums), in the dtype of `args`."""
    a = [t.clone() for t in args]
    for i in (3, 7, 8):
        a[i].requires_grad_(True)
    sums = loss_sums(*a)
    return torch.autograd.grad(sums, [a[3], a[7], a[8]], grad_outputs=grad_sums.to(sums.dtype))


# ---------------------------------------------------------------- the yardstick and the gates, shared by the CPU and the GPU tests
DEPTH_REL, DEPTH_RMS, POSE_REL = 1e-3, 1e-3, 5e-3
COLUMNS = tuple(range(8)) + ("random",)


def grad_sums_of(column, n, dtype=torch.float64):
    """One-hot in `column` for every frame, or ("random") a fixed positive N x 8 in [0.5, 1.5)."""
    if column == "random":
        return (torch.rand(n, 8, dtype=torch.float64, generator=torch.Generator().manual_seed(20)) + 0.5).to(dtype)
    gs = torch.zeros(n, 8, dtype=dtype)
    gs[:, column] = 1
    return gs


def autograd_columns(args, loss_sums, columns=COLUMNS):
    """{column: (grad_depth, grad_pose01, grad_pose02)} by torch.autograd through `loss_sums`, in the dtype of `args`: one forward,
    one backward per column."""
    a = [t.clone() for t in args]
    for i in (3, 7, 8):
        a[i].requires_grad_(True)
    sums = loss_sums(*a)
    return {col: torch.autograd.grad(sums, [a[3], a[7], a[8]], grad_outputs=grad_sums_of(col, sums.shape[0], sums.dtype), retain_graph=True)
            for col in columns}


def depth_gate(got, want):
    """Per pixel |g - g64| / (1e-3 |g64| + 1e-3 rms_frame(g64)); where the bound is 0 (a column without a gradient) an exact
    0 gives 0 and anything else inf.  NaN in `got` gives inf."""
    got, want = got.detach().double().cpu(), want.double()
    rms = want.pow(2).mean(dim=(1, 2, 3), keepdim=True).sqrt()
    bound = DEPTH_REL * want.abs() + DEPTH_RMS * rms
    err = (got - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)


def pose_gate(got, want):
    """Per frame max |g - g64| over rows 0-2 / (5e-3 max |g64|), N values; exact zeros against zeros give 0."""
    got, want = got.detach().double().cpu()[:, :3], want.double()[:, :3]
    err = (got - want).abs().amax(dim=(1, 2))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / (POSE_REL * want.abs().amax(dim=(1, 2))))
    return torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)


def check_gates(label, got, want, fraction=1.0):
    """The issue's gates on (grad_depth, grad_pose01, grad_pose02) against the fp64 autograd `want`: every pixel within
    `fraction` of the depth gate except at most pixels // 1000 of the case, those finite too; every frame's pose gradients within
    `fraction` of theirs; row 3 exactly 0.  -> the figures, printed before anything is asserted."""
    ratio = depth_gate(got[0], want[0])
    cap = ratio.numel() // 1000
    missed = int((ratio > fraction).sum())
    inside = ratio[ratio <= fraction]
    p1, p2 = pose_gate(got[1], want[1]), pose_gate(got[2], want[2])
    figures = {"depth_missed": missed, "cap": cap, "depth_worst_inside": float(inside.max()) if inside.numel() else 0.0,
               "pose01": float(p1.max()), "pose02": float(p2.max())}
    print(f"{label}: depth {missed} of {ratio.numel()} pixels miss (cap {cap}), the others at most {figures['depth_worst_inside']:.3g} "
          f"of the gate; pose01 {figures['pose01']:.3g} pose02 {figures['pose02']:.3g} of theirs")
    assert bool(torch.isfinite(got[0].detach().double()).all()), (label, "grad_depth is not finite")
    assert missed <= cap, (label, figures)
    assert figures["pose01"] <= fraction and figures["pose02"] <= fraction, (label, figures)
    for g in got[1:]:
        assert bool((g.detach()[:, 3] == 0).all()), (label, "row 3 of a pose gradient is not 0")
    return figures
