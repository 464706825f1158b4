"""CPU: do the inputs of tests/loss_cases.py have the power to tell a wrong loss kernel from a right one?

Every entry of MISTAKES is the oracle (tests/loss_oracle.py, fp64) with one deliberate mistake of the kind one can make in
csrc/loss.hip.  For each, at least one case of loss_cases.CASES must move at least one GATED quantity by at least 10 x its gate:

  a term (loss_color ... loss) or one of the N x 8 per-frame sums   relative to the true fp64 value, gate 2e-5 (TIGHT)
  image01 or image02                                                 max abs, gate 1e-4 (TOL)

These are the gates of tests/test_loss_gpu.py.  The other half of the argument, `test_fp32_oracle_is_three_times_inside_the_gates`,
keeps a CORRECT fp32 evaluation at most a third of each gate away from fp64 on every case, so the same inputs cannot fail a right
kernel.  With make_triplet's own inputs (one symmetric camera for the whole batch) the camera mistakes (frame 0's K, fx and fy swapped, no skew, a centred principal point) move nothing at all:
`test_make_triplet_alone_cannot_see_the_camera_mistakes` records that, which is why the cases exist.

    python -m pytest tests/test_loss_power_cpu.py -s -q      (prints the table: mistake, best case, factor over the gate)
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import kbnet_amd as kb

import loss_cases
import loss_oracle as lo

TIGHT, TOL, POWER = 2e-5, 1e-4, 10.0
SCALARS = ("loss_color", "loss_structure", "loss_sparse_depth", "loss_smoothness", "loss")
WEIGHTS = (lo.W_COLOR, lo.W_STRUCTURE, lo.W_SPARSE_DEPTH, lo.W_SMOOTHNESS)


# ---------------------------------------------------------------- the oracle taken apart, so that one piece can be replaced
def positions(args):
    """The two N x 2 x H x W maps of sample positions."""
    i0, _, _, depth, _, _, k, p01, p02 = args
    h, w = i0.shape[2:]
    points = lo.backproject(depth, k)
    return [lo.project(points, p, k, h, w) for p in (p01, p02)]


def terms_of(sums, h, w):
    """N x 8 sums -> the five scalars, normalised as ops.loss_terms normalises them."""
    hw = float(h * w)
    per_frame = torch.stack([(sums[:, 0] + sums[:, 1]) / hw, (sums[:, 2] + sums[:, 3]) / hw, sums[:, 4] / sums[:, 5],
                             sums[:, 6] / float(h * (w - 1)) + sums[:, 7] / float((h - 1) * w)], 1)
    t = per_frame.mean(0)
    return dict(zip(SCALARS, list(t) + [sum(wt * x for wt, x in zip(WEIGHTS, t))]))


def outcome(args, images=None, edit_sums=None):
    """What a kernel hands back: the two warped images, the N x 8 sums and the scalars that follow from them."""
    i0, i1, i2, depth, sparse, validity = args[:6]
    if images is None:
        xy = positions(args)
        images = [lo.warp(i1, xy[0]), lo.warp(i2, xy[1])]
    sums = lo.frame_sums(i0, images[0], images[1], depth, sparse, validity)
    if edit_sums is not None:
        sums = edit_sums(sums.clone(), args, images)
    return {"image01": images[0], "image02": images[1], "sums": sums, **terms_of(sums, *i0.shape[2:])}


def gather_warp(image, xy, east_tap_lost_at_last_column=False):
    """lo.warp without grid_sample: clamp the position into the image (border padding), four taps, a tap outside the image
    skipped.  The mistake: `xb >= W - 1` instead of `xb > W - 1` drops the east taps of every sample between the last two columns."""
    n, c, h, w = image.shape
    ix, iy = xy[:, 0].clamp(0, w - 1), xy[:, 1].clamp(0, h - 1)
    x0, y0 = ix.floor(), iy.floor()
    wx1, wy1 = ix - x0, iy - y0
    x0, y0 = x0.long(), y0.long()
    flat = image.reshape(n, c, h * w)
    out = torch.zeros_like(image)
    for dy, dx, wgt in ((0, 0, (1 - wx1) * (1 - wy1)), (0, 1, wx1 * (1 - wy1)), (1, 0, (1 - wx1) * wy1), (1, 1, wx1 * wy1)):
        x, y = x0 + dx, y0 + dy
        lost = (x > w - 1) | (y > h - 1)
        if east_tap_lost_at_last_column and dx:
            lost = lost | (x >= w - 1)
        idx = (y.clamp(max=h - 1) * w + x.clamp(max=w - 1)).reshape(n, 1, h * w).expand(n, c, h * w)
        out += torch.gather(flat, 2, idx).reshape(n, c, h, w) * torch.where(lost, torch.zeros_like(wgt), wgt)[:, None]
    return out


def grid_sample_as(args, padding_mode="border", align_corners=True, shift=(0.0, 0.0)):
    """lo.warp's normalisation, then grid_sample with other settings, or at positions `shift` pixels away."""
    i0, i1, i2 = args[:3]
    h, w = i0.shape[2:]
    images = []
    for im, xy in zip((i1, i2), positions(args)):
        g = xy.permute(0, 2, 3, 1).clone()
        g[..., 0] = (g[..., 0] + shift[0]) / (w - 1.0)
        g[..., 1] = (g[..., 1] + shift[1]) / (h - 1.0)
        images.append(F.grid_sample(im, 2.0 * (g - 0.5), mode="bilinear", padding_mode=padding_mode, align_corners=align_corners))
    return images


def with_inputs(**changed):
    """A mistake that amounts to reading other inputs: `changed` maps an argument's position to a function of the argument list."""
    def run(args):
        a = list(args)
        for i, f in changed.items():
            a[int(i[1:])] = f(args)
        return outcome(a)
    return run


def _frame0(i):
    return lambda args: args[i][:1].expand_as(args[i]).contiguous()


def _k(edit):
    def f(args):
        k = args[6].clone()
        edit(k, *args[0].shape[2:])
        return k
    return f


def _swap_focals(k, h, w):
    k[:, 0, 0], k[:, 1, 1] = k[:, 1, 1].clone(), k[:, 0, 0].clone()


def _no_skew(k, h, w):
    k[:, 0, 1] = 0


def _centre(k, h, w):
    k[:, 0, 2], k[:, 1, 2] = 0.5 * (w - 1), 0.5 * (h - 1)


def _ssim_sums(args, images, stretch):
    """sums 2 and 3 with another way from the (H-2) x (W-2) scores to the frame's sum."""
    i0 = args[0]
    return [stretch(lo.ssim_distance(im, i0), *i0.shape[2:]) for im in images]


def _ssim_plain_mean(scores, h, w):
    return scores.mean(dim=(1, 2, 3)) * 3 * h * w


def _ssim_integer_index_plus_one(scores, h, w):
    rows = torch.tensor([min(d * (h - 2) // h + 1, h - 3) for d in range(h)])
    cols = torch.tensor([min(d * (w - 2) // w + 1, w - 3) for d in range(w)])
    return scores[:, :, rows][:, :, :, cols].sum(dim=(1, 2, 3))


def _edit_ssim(stretch):
    def edit(sums, args, images):
        sums[:, 2], sums[:, 3] = _ssim_sums(args, images, stretch)
        return sums
    return edit


def _binary_validity(sums, args, images):
    depth, sparse, validity = args[3:6]
    v = (validity > 0).to(validity.dtype)
    sums[:, 4], sums[:, 5] = (v * (sparse - depth).abs()).sum(dim=(1, 2, 3)), v.sum(dim=(1, 2, 3))
    return sums


def _unweighted_smoothness(sums, args, images):
    depth = args[3]
    sums[:, 6] = (depth[..., :, :-1] - depth[..., :, 1:]).abs().sum(dim=(1, 2, 3))
    sums[:, 7] = (depth[..., :-1, :] - depth[..., 1:, :]).abs().sum(dim=(1, 2, 3))
    return sums


def _smoothness_axes_exchanged(sums, args, images):
    sums[:, 6], sums[:, 7] = sums[:, 7].clone(), sums[:, 6].clone()
    return sums


MISTAKES = {
    # camera and pose
    "frame 0's intrinsics for every frame": with_inputs(a6=_frame0(6)),
    "frame 0's pose01 for every frame": with_inputs(a7=_frame0(7)),
    "frame 0's pose02 for every frame": with_inputs(a8=_frame0(8)),
    "fx and fy swapped": with_inputs(a6=_k(_swap_focals)),
    "skew ignored": with_inputs(a6=_k(_no_skew)),
    "principal point taken as the frame centre": with_inputs(a6=_k(_centre)),
    "pose01 and pose02 exchanged": with_inputs(a7=lambda a: a[8], a8=lambda a: a[7]),
    "image1 and image2 exchanged": with_inputs(a1=lambda a: a[2], a2=lambda a: a[1]),
    # sampling
    "zero padding instead of border padding": lambda a: outcome(a, grid_sample_as(a, padding_mode="zeros")),
    "align_corners=False": lambda a: outcome(a, grid_sample_as(a, align_corners=False)),
    "sample positions one pixel off in x": lambda a: outcome(a, grid_sample_as(a, shift=(1.0, 0.0))),
    "sample positions one pixel off in y": lambda a: outcome(a, grid_sample_as(a, shift=(0.0, 1.0))),
    "east tap left out at the last column": lambda a: outcome(a, [gather_warp(im, xy, True) for im, xy in zip(a[1:3], positions(a))]),
    # terms
    "SSIM scores averaged, not stretched": lambda a: outcome(a, edit_sums=_edit_ssim(_ssim_plain_mean)),
    "SSIM stretch by d (L-2) // L + 1": lambda a: outcome(a, edit_sums=_edit_ssim(_ssim_integer_index_plus_one)),
    "validity binarised (v > 0)": lambda a: outcome(a, edit_sums=_binary_validity),
    "smoothness without its exp(-image gradient) weight": lambda a: outcome(a, edit_sums=_unweighted_smoothness),
    "dx and dy exchanged in the smoothness sums": lambda a: outcome(a, edit_sums=_smoothness_axes_exchanged),
}


# ---------------------------------------------------------------- the measure
@functools.lru_cache(maxsize=None)
def _case64(name):
    args = [a.double() for a in loss_cases.case(name)]
    return args, _truth(args)


def _truth(args):
    out = lo.compute_loss(*args)
    out["sums"] = lo.loss_sums(*args)
    return out


def gate_factors(got, want):
    """Every gated quantity of `got` as a multiple of its gate, against the fp64 truth `want`."""
    f = {k: abs(float(got[k]) - float(want[k])) / abs(float(want[k])) / TIGHT for k in SCALARS}
    rel = (got["sums"].double() - want["sums"]).abs() / want["sums"].abs()
    assert bool((want["sums"] != 0).all())                 # no case of the table has an empty sum; the GPU test handles one
    for i in range(rel.shape[0]):
        for j in range(8):
            f[f"sums[{i}][{j}]"] = float(rel[i, j]) / TIGHT
    for k in ("image01", "image02"):
        f[k] = float((got[k].double() - want[k]).abs().max()) / TOL
    return f


def test_the_pieces_put_together_are_the_oracle():
    """outcome(), gather_warp() and grid_sample_as() without a mistake give lo.compute_loss: what a mistake moves is the mistake."""
    for name in loss_cases.CASES:
        args, want = _case64(name)
        for label, got in (("outcome", outcome(args)), ("grid_sample_as", outcome(args, grid_sample_as(args))),
                           ("gather_warp", outcome(args, [gather_warp(im, xy) for im, xy in zip(args[1:3], positions(args))]))):
            worst = max(gate_factors(got, want).values())
            assert worst <= 1e-6, (name, label, worst)          # 1e-6 of a gate: 2e-11 relative, 1e-10 absolute
        per_frame = want["per_frame"]
        sums, (h, w) = want["sums"], args[0].shape[2:]
        mine = torch.stack([(sums[:, 0] + sums[:, 1]) / (h * w), (sums[:, 2] + sums[:, 3]) / (h * w), sums[:, 4] / sums[:, 5],
                            sums[:, 6] / (h * (w - 1)) + sums[:, 7] / ((h - 1) * w)], 1)
        assert float(((mine - per_frame).abs() / per_frame.abs()).max()) <= 1e-12


@pytest.mark.parametrize("mistake", list(MISTAKES))
def test_every_mistake_is_caught_ten_times_over(mistake):
    best = (0.0, None, None)
    rows = []
    for name in loss_cases.CASES:
        args, want = _case64(name)
        f = gate_factors(MISTAKES[mistake](args), want)
        q = max(f, key=f.get)
        rows.append(f"{name} {f[q]:.3g} ({q})")
        best = max(best, (f[q], name, q))
    print(f"\n| {mistake} | {best[1]} | {best[2]} | {best[0]:.3g} |   all: " + "; ".join(rows))
    assert best[0] >= POWER, (mistake, rows)


@pytest.mark.parametrize("name", list(loss_cases.CASES))
def test_fp32_oracle_is_three_times_inside_the_gates(name):
    args, want = _case64(name)
    f = gate_factors(_truth(loss_cases.case(name)), want)
    q = max(f, key=f.get)
    pf32, pf64 = lo.compute_loss(*loss_cases.case(name))["per_frame"], want["per_frame"]
    per_frame = float(((pf32.double() - pf64).abs() / pf64.abs()).max()) / TIGHT
    print(f"\n{name}: fp32 oracle at most {f[q]:.3g} of a gate ({q}), per_frame {per_frame:.3g}")
    assert f[q] <= 1 / 3 and per_frame <= 1 / 3, (name, q, f[q], per_frame)


def test_make_triplet_alone_cannot_see_the_camera_mistakes():
    """Why the cases exist: on make_triplet's inputs four of the camera mistakes are no mistakes."""
    *frames, v01, v02 = kb.synthetic.make_triplet(3, 37, 45, "void", seed=12)
    args = [a.double() for a in frames + [lo.pose_matrix(v01), lo.pose_matrix(v02)]]
    want = _truth(args)
    for mistake in ("frame 0's intrinsics for every frame", "fx and fy swapped", "skew ignored", "principal point taken as the frame centre"):
        f = gate_factors(MISTAKES[mistake](args), want)
        assert f["image01"] == f["image02"] == 0.0 and max(f.values()) <= 1e-6, mistake    # the scalars: summation order only


def test_the_table_has_what_the_issue_asks_for():
    sizes = {(c["h"], c["w"]) for c in loss_cases.CASES.values()}
    assert any(h <= 16 and w <= 64 for h, w in sizes)                                  # one case inside a single tile
    assert sum(1 for h, w in sizes if h > 16 and w > 64 and h % 16 and w % 64) >= 2    # several tiles, ragged both ways
    used = set().union(*[set(c["families"]) for c in loss_cases.CASES.values()])
    assert used == set(loss_cases.FAMILIES)
    assert any(set(c["families"]) == set(loss_cases.FAMILIES) and c["n"] == 3 for c in loss_cases.CASES.values())
    for name, c in loss_cases.CASES.items():
        args = loss_cases.case(name)
        assert all(torch.equal(a, b) for a, b in zip(args, loss_cases.case(name))), name       # deterministic
        k = args[6]
        if "general_camera" in c["families"]:
            assert bool(((k[:, 0, 0] / k[:, 1, 1] - 1).abs() >= 0.05).all()) and bool((k[:, 0, 1] != 0).all())
            assert not torch.equal(k[0], k[1]) and not torch.equal(args[7][0], args[7][1]) and not torch.equal(args[8][0], args[8][1])
        if "weighted_validity" in c["families"]:
            assert set(args[5].unique().tolist()) == {0.0, 0.25, 1.0}
        if "two_plane" in c["families"]:
            step = (args[3][..., :, 1:] - args[3][..., :, :-1]).abs()
            assert float(step.max()) > 5 and float(step.median()) < 0.1                # piecewise constant plus a smooth part
