"""The inputs of tests/test_pre_eval_gpu.py, built once from seeds in NumPy, the oracles of the three small kernels around the model
(csrc/pre_eval.hip: kbn_preprocess_forward, kbn_eval_accumulate; csrc/unpack.hip: kbn_unpack_frames_forward) and the comparisons the
GPU tests make -- shared with tests/test_pre_eval_power_cpu.py, which plants mistakes into the oracles at these very inputs and asserts
that the comparisons see each of them.  Nothing here needs a GPU.

Preprocess   oracle.kbnet_oracle.validity_and_outlier_removal as it is; `outlier_removal` restates it in NumPy (bit-equal, asserted on
             every case) so that a mistake can be planted; the image normalisation is float32 NumPy, one rounding per operation.
Evaluation   `eval_oracle`: the reference's mask, NumPy float32 per-pixel terms formed as oracle.kbnet_oracle.evaluation_metrics forms
             them, summed in float64 and divided by the count; NaN where the count is 0.
Unpack       `unpack_oracle`: slice, transpose, convert('RGB')'s rule, uint16 / 256.

The only tolerances: EVAL_GATE (count * 2**-51 relative to eval_oracle: the fp32 terms are identical and non-negative, only the order
of at most `count` float64 additions differs; the square root halves the error) and REFERENCE_RTOL (the 2e-5 of
test_eval_metrics_golden, against evaluation_metrics, whose means are fp32).  Everything else is bit equality."""
import warnings

import numpy as np
import torch

from oracle import kbnet_oracle as orc

F32 = np.float32
EVAL_GATE = 2.0 ** -51      # times the frame's count, relative
REFERENCE_RTOL = 2e-5
SENTINEL = F32(-7777.0)     # what the GPU test leaves in freed memory before ops.unpack_frames allocates; the value of an unwritten element


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _bit_findings(role, got, want):
    if got is None or want is None:
        return [] if got is None and want is None else [f"{role}: {'missing' if got is None else 'unexpected'}"]
    got = np.asarray(got)
    if got.shape != want.shape or got.dtype != want.dtype:
        return [f"{role}: {got.dtype} {got.shape}, expected {want.dtype} {want.shape}"]
    bad = int((_bits(got) != _bits(want)).sum())
    return [f"{role}: {bad} of {want.size} elements differ in bits"] if bad else []


# ===================================================================================================================== preprocess
PRE_MISTAKES = ("radius_minus_1", "pad_zero", "seam64", "seam16", "le", "per_frame_max", "binary_validity", "max_skips_last")


def _window_min(filled, pad_value, radius, seam):
    """k x k minimum of one H x W frame whose border is padded with pad_value; seam = (rows, columns) of a tile the window must not
    leave (a planted mistake), or None."""
    h, w = filled.shape
    padded = np.pad(filled, radius, constant_values=pad_value) if radius else filled
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    mn = filled.copy()
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            cand = padded[radius + dy:radius + dy + h, radius + dx:radius + dx + w]
            if seam is not None:
                inside = ((ys + dy) // seam[0] == ys // seam[0]) & ((xs + dx) // seam[1] == xs // seam[1])
                cand = np.where(inside, cand, F32(np.inf))
            mn = np.minimum(mn, cand)
    return mn


def outlier_removal(sparse, kernel_size=7, threshold=1.5, mistake=None):
    """validity_and_outlier_removal restated in float32 NumPy: (filtered sparse depth, filtered validity) of an N x 1 x H x W batch.
    With no mistake it equals the oracle bit for bit."""
    assert mistake is None or mistake in PRE_MISTAKES, mistake
    s = np.asarray(sparse, dtype=F32)
    validity = np.where(s > 0, F32(1), F32(0) if mistake == "binary_validity" else s)
    radius = kernel_size // 2
    if mistake == "radius_minus_1":
        radius = max(radius - 1, 0)
    seam = {"seam64": (1 << 30, 64), "seam16": (16, 1 << 30)}.get(mistake)
    batch_max = s.reshape(-1)[:-1].max() if mistake == "max_skips_last" and s.size > 1 else s.max()
    mins = np.empty_like(s)
    for i in range(s.shape[0]):
        fill = F32(10) * (s[i].max() if mistake == "per_frame_max" else batch_max)
        filled = np.where(validity[i, 0] <= 0, fill, s[i, 0])
        mins[i, 0] = _window_min(filled, F32(0) if mistake == "pad_zero" else fill, radius, seam)
    limit = s - F32(threshold)
    remove = mins <= limit if mistake == "le" else mins < limit
    clean = validity * np.where(remove, F32(0), F32(1))
    return s * clean, clean


def normalize_image(image, value_range):
    """ops.preprocess's image for run_kbnet.py --normalized_image_range: each operation rounded to fp32."""
    x = np.asarray(image, dtype=F32)
    if list(value_range) == [0, 255]:
        return x
    t = x / F32(255)
    return t if list(value_range) == [0, 1] else F32(2) * t - F32(1)


def _depths(rng, n, h, w, density):
    """Sparse depth quantised to multiples of 0.5 in 1.0 .. 8.0, so that minimum == depth - threshold happens for the thresholds in use."""
    z = rng.integers(2, 17, size=(n, 1, h, w)).astype(F32) * F32(0.5)
    return np.where(rng.random((n, 1, h, w)) < density, z, F32(0)).astype(F32)


def _plant_seams(s):
    """A 6.0 in the first column / row of the second tile whose only smaller neighbour is a 1.0 across the 64-column / 16-row seam."""
    n, _, h, w = s.shape
    if w > 64 and h >= 5:
        s[:, 0, 0:13, 64:72] = 0
        s[:, 0, 5, 63], s[:, 0, 5, 64] = 1.0, 6.0
    if h > 16 and w >= 28:
        s[:, 0, 16:24, 13:28] = 0
        s[:, 0, 15, 20], s[:, 0, 16, 20] = 1.0, 6.0


PRE_SHAPES = ((1, 1, 1), (2, 5, 3), (1, 16, 64), (2, 17, 65), (2, 37, 130), (3, 33, 70))
PRE_KERNEL_SIZES = (1, 3, 7, 9, 15)
PRE_THRESHOLDS = (1.5, 0.5, 0.0)


def _pre_case(name, sparse, kernel_size, threshold, image=None, value_range=(0, 1), kind="plain"):
    return dict(name=name, sparse=np.ascontiguousarray(sparse, dtype=F32), kernel_size=kernel_size, threshold=float(threshold),
                image=image, range=list(value_range), kind=kind)


def pre_shape_name(shape):
    return "x".join(str(v) for v in shape)


def pre_grid_cases(shape):
    """One seeded batch per shape under every kernel size and threshold.  A few percent of the pixels are valid where the frame is
    large enough for that to leave neighbours; the frames of a few dozen pixels are 40 % valid."""
    n, h, w = shape
    rng = np.random.default_rng([21, n, h, w])
    s = _depths(rng, n, h, w, 0.4 if h * w < 200 else 0.08)
    if shape == (1, 1, 1):
        s[...] = 2.5
    _plant_seams(s)
    return [_pre_case(f"{pre_shape_name(shape)} k{k} t{t}", s, k, t) for k in PRE_KERNEL_SIZES for t in PRE_THRESHOLDS]


NEGATIVE_THRESHOLD = -300.0     # between 10 x 20 (the other frames' maximum) and 10 x 77.5 (the batch's)


def _negative_batch(rng, n, h, w):
    """Positive depths up to 20, negative ones down to -8, the batch maximum 77.5 planted by the caller.  Under threshold -300 every
    point with a valid one in its window goes; a negative point alone in its window stays only while the fill is 775, not 200."""
    s = _depths(rng, n, h, w, 0.02)
    s = np.where(s > 0, s * F32(2.5), s)
    negative = (rng.random(s.shape) < 0.04) & (s == 0)
    s[negative] = -rng.integers(1, 17, size=int(negative.sum())).astype(F32) * F32(0.5)
    return s


def pre_negative_cases():
    rng = np.random.default_rng(22)
    s = _negative_batch(rng, 3, 20, 70)
    s[0, 0, 7, 30] = 77.5
    assert s[1:].max() == 20.0 and s.max() == 77.5
    return [_pre_case(f"negative k{k}", s, k, NEGATIVE_THRESHOLD, kind="negative") for k in (3, 7)]


def pre_zero_case():
    return _pre_case("all zero", np.zeros((2, 1, 17, 65), F32), 7, 1.5, kind="zero")


def pre_large_case():
    """1 x 2049 x 2048 = 4 196 352 elements, 2048 past what max_reduce_kernel's capped grid covers in one pass.  The maximum is the
    last element: a reduction that stops at the cap (or anywhere short of the end) fills with 200 and removes the lone negatives."""
    rng = np.random.default_rng(23)
    s = _negative_batch(rng, 1, 2049, 2048)
    s[0, 0, -1, -1] = 77.5
    assert s.reshape(-1)[:-1].max() == 20.0
    return _pre_case("large 1x2049x2048", s, 3, NEGATIVE_THRESHOLD, kind="large")


def _byte_image(rng, n, c, h, w):
    """Every integer 0 .. 255 in every channel, and non-integers between and beside them."""
    x = rng.integers(0, 256, size=(n, c, h * w)).astype(F32)
    assert n * h * w >= 256 + 8
    flat = x.transpose(1, 0, 2).reshape(c, -1)
    for ch in range(c):
        at = rng.permutation(flat.shape[1])
        flat[ch, at[:256]] = np.arange(256, dtype=F32)
        flat[ch, at[256:264]] = np.array([0.5, 1e-3, 127.25, 254.999, 255.0 - 2.0 ** -16, 1.0 / 3.0, 200.7, 85.0 + 2.0 ** -17], dtype=F32)
    return np.ascontiguousarray(flat.reshape(c, n, h * w).transpose(1, 0, 2).reshape(n, c, h, w))


def pre_image_cases():
    rng = np.random.default_rng(24)
    s = _depths(rng, 2, 17, 65, 0.08)
    cases = []
    for c in (1, 3):
        image = _byte_image(rng, 2, c, 17, 65)
        for value_range in ([0, 1], [-1, 1], [0, 255]):
            cases.append(_pre_case(f"image c{c} {value_range}", s, 7, 1.5, image=image, value_range=value_range, kind="image"))
    return cases


def pre_small_cases():
    return [c for shape in PRE_SHAPES for c in pre_grid_cases(shape)] + pre_negative_cases() + [pre_zero_case()] + pre_image_cases()


def pre_expected(case, mistake=None):
    """(image or None, filtered validity, filtered sparse depth) as ops.preprocess returns them: the oracle's, or with a mistake the
    restatement's."""
    if mistake is None:
        filtered, validity = orc.validity_and_outlier_removal(torch.from_numpy(case["sparse"]), case["kernel_size"], case["threshold"])
        filtered, validity = filtered.numpy(), validity.numpy()
    else:
        filtered, validity = outlier_removal(case["sparse"], case["kernel_size"], case["threshold"], mistake=mistake)
    image = None if case["image"] is None else normalize_image(case["image"], case["range"])
    return image, validity, filtered


def pre_mismatches(case, got, want=None):
    """What the GPU test asserts to be empty: got = (image or None, validity, filtered) against the oracle bit for bit."""
    want = pre_expected(case) if want is None else want
    return [f for role, g, w in zip(("image", "validity", "filtered"), got, want) for f in _bit_findings(role, g, w)]


def pre_points(case, want=None):
    """(removed, kept): the nonzero input pixels whose filtered validity is zero / is not -- from the oracle alone."""
    want = pre_expected(case) if want is None else want
    points = case["sparse"] != 0
    return int((points & (want[1] == 0)).sum()), int((points & (want[1] != 0)).sum())


# ===================================================================================================================== evaluation
EVAL_MISTAKES = ("closed_bounds", "validity_nonzero", "fma_terms", "batch_count", "empty_is_zero")


def eval_oracle(output_depth, ground_truth, validity, dmin, dmax, mistake=None):
    """(N x 4 float64 metrics, N counts).  The per-pixel terms are the float32 values evaluation_metrics forms; their sums are float64."""
    assert mistake is None or mistake in EVAL_MISTAKES, mistake
    n = output_depth.shape[0]
    o_all, g_all, v_all = (np.asarray(a, dtype=F32).reshape(n, -1) for a in (output_depth, ground_truth, validity))
    dmin, dmax = F32(dmin), F32(dmax)
    sums, counts = np.zeros((n, 4)), np.zeros(n)
    with np.errstate(all="ignore"):
        for i in range(n):
            g, v = g_all[i], v_all[i]
            valid = v != 0 if mistake == "validity_nonzero" else v > 0
            mask = valid & ((g >= dmin) & (g <= dmax) if mistake == "closed_bounds" else (g > dmin) & (g < dmax))
            o, g = o_all[i][mask], g[mask]
            src, tgt = F32(1000.0) * o, F32(1000.0) * g
            if mistake == "fma_terms":      # what a contraction of 1000 o - fl(1000 g) into one FMA computes: the product is never rounded
                e = (np.float64(1000.0) * o.astype(np.float64) - tgt.astype(np.float64)).astype(F32)
            else:
                e = tgt - src
            ie = (F32(1.0) / (F32(0.001) * g)) - (F32(1.0) / (F32(0.001) * o))
            terms = (np.abs(e), e * e, np.abs(ie), ie * ie)
            assert all(t.dtype == F32 for t in terms)
            sums[i] = [t.astype(np.float64).sum() for t in terms]
            counts[i] = mask.sum()
        divisor = np.full(n, counts.sum()) if mistake == "batch_count" else counts.copy()
        if mistake == "empty_is_zero":
            divisor = np.maximum(divisor, 1.0)
        mean = sums / divisor[:, None]
        return np.stack([mean[:, 0], np.sqrt(mean[:, 1]), mean[:, 2], np.sqrt(mean[:, 3])], axis=1), counts


def reference_metrics(case):
    """oracle.kbnet_oracle.evaluation_metrics frame by frame, N x 4 float64 (NaN for a frame that counts nothing, inf where a counted
    prediction is 0, as NumPy gives them).  It squeezes its arguments, and a frame of one pixel would become a scalar it cannot index:
    such a frame is handed over with a second pixel of validity 0 beside it, which the mask drops."""
    rows = []
    n = case["output_depth"].shape[0]
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for i in range(n):
            o, g, v = (case[k][i].reshape(-1) for k in ("output_depth", "ground_truth", "validity"))
            if o.size == 1:
                o, g, v = np.append(o, F32(1)), np.append(g, F32(1)), np.append(v, F32(0))
            rows.append(orc.evaluation_metrics(o, g, v, case["dmin"], case["dmax"]))
    return np.asarray(rows, dtype=np.float64)


def _eval_case(name, o, g, v, dmin=1e-3, dmax=50.0, layout="n1hw", planted=False, empty=()):
    o, g, v = (np.ascontiguousarray(a, dtype=F32) for a in (o, g, v))
    assert o.ndim == 3 and o.shape == g.shape == v.shape
    return dict(name=name, output_depth=o, ground_truth=g, validity=v, dmin=dmin, dmax=dmax, layout=layout, planted=planted, empty=tuple(empty))


def _ordinary(rng, n, h, w, density=0.3):
    """Ground truth in 1 .. 60 (so some of it is past max_evaluate_depth = 50), predictions about 1 m off, every frame with a counted pixel."""
    g = rng.uniform(1.0, 60.0, size=(n, h, w)).astype(F32)
    v = (rng.random((n, h, w)) < density).astype(F32)
    g[:, 0, 0], v[:, 0, 0] = rng.uniform(1.0, 40.0, size=n).astype(F32), 1.0
    o = np.clip(g + rng.normal(size=(n, h, w)).astype(F32), 1.5, 100.0).astype(F32)
    return o, g, v


def eval_size_cases():
    rng = np.random.default_rng(31)
    return [_eval_case(f"size {h * w}", *_ordinary(rng, 3, h, w)) for h, w in ((1, 1), (15, 17), (64, 64), (17, 241))]


def eval_large_case():
    """1 x 1025 x 1024 = 1 049 600 pixels: 1024 past what the 256-block grid covers in one pass."""
    return _eval_case("large 1x1025x1024", *_ordinary(np.random.default_rng(32), 1, 1025, 1024))


def eval_bounds_case():
    """Ground truth exactly at min_evaluate_depth and max_evaluate_depth (both representable), valid: the strict bounds drop it."""
    o, g, v = _ordinary(np.random.default_rng(33), 3, 15, 17)
    g[:, 2, 3:6], v[:, 2, 3:6] = 0.5, 1.0
    g[:, 4, 3:6], v[:, 4, 3:6] = 50.0, 1.0
    o[:, 2, 3:6], o[:, 4, 3:6] = 3.0, 30.0
    return _eval_case("bounds", o, g, v, dmin=0.5, dmax=50.0, planted=True)


def eval_validity_case():
    """Validity 0, negative and NaN count nothing; 1e-30 counts.  The ground truth under them is in range, the prediction far off."""
    o, g, v = _ordinary(np.random.default_rng(34), 3, 15, 17)
    for col, value in enumerate((0.0, -1.0, np.nan, 1e-30, -1e-30, -np.inf)):
        v[:, 3, col], g[:, 3, col], o[:, 3, col] = value, 10.0 + col, 90.0
    return _eval_case("validity", o, g, v, planted=True)


def eval_poison_case():
    """Masked-out pixels holding NaN, inf and 0 in the prediction and in the ground truth: under validity 0, and -- for the ground
    truth -- under validity 1, where the bounds drop them (NaN compares false, inf is past the maximum, 0 is not above the minimum)."""
    o, g, v = _ordinary(np.random.default_rng(35), 3, 15, 17)
    poison = (np.nan, np.inf, -np.inf, 0.0)
    for col, value in enumerate(poison):
        v[:, 5, col], o[:, 5, col] = 0.0, value                                      # poisoned prediction, masked by the validity
        v[:, 6, col], g[:, 6, col], o[:, 6, col] = 0.0, value, value                 # both poisoned, masked by the validity
        v[:, 7, col], g[:, 7, col] = 1.0, value                                      # poisoned ground truth, valid: masked by the bounds
        v[:, 8, col], g[:, 8, col], o[:, 8, col] = 1.0, value, np.nan                # ... with a NaN prediction behind it
    return _eval_case("poison", o, g, v, planted=True)


def eval_ulp_case(ulps):
    """Every pixel counted, the prediction `ulps` float32 steps above the ground truth: |1000 o - 1000 g| is then a few steps of the
    products' rounding, which an FMA would not make."""
    rng = np.random.default_rng(36)
    g = rng.uniform(1.0, 60.0, size=(3, 15, 17)).astype(F32)
    o = (g.view(np.int32) + np.int32(ulps)).view(F32)
    return _eval_case(f"ulp {ulps}", o, g, np.ones_like(g), dmax=100.0)


def eval_empty_case():
    """A frame without an evaluated pixel between two ordinary ones: half of it invalid, the other half valid and past the maximum."""
    o, g, v = _ordinary(np.random.default_rng(37), 3, 15, 17)
    v[1, :7], v[1, 7:], g[1, 7:] = 0.0, 1.0, 55.0
    return _eval_case("empty frame", o, g, v, empty=(1,))


def eval_zero_prediction_case():
    """A counted pixel whose prediction is 0 (frame 1): 1 / (0.001 x 0) = inf, so iMAE and iRMSE are inf while MAE and RMSE are finite."""
    o, g, v = _ordinary(np.random.default_rng(38), 3, 15, 17)
    o[1, 4, 4], g[1, 4, 4], v[1, 4, 4] = 0.0, 12.0, 1.0
    return _eval_case("zero prediction", o, g, v)


def eval_layout_cases():
    rng = np.random.default_rng(39)
    return [_eval_case(f"layout {layout}", *_ordinary(rng, 3, 17, 67), layout=layout) for layout in ("n1hw", "nhw", "view")]


def eval_small_cases():
    return (eval_size_cases() + [eval_bounds_case(), eval_validity_case(), eval_poison_case()] + [eval_ulp_case(u) for u in (1, 4, 64)] +
            [eval_empty_case(), eval_zero_prediction_case()] + eval_layout_cases())


def eval_expected(case, mistake=None):
    return eval_oracle(case["output_depth"], case["ground_truth"], case["validity"], case["dmin"], case["dmax"], mistake=mistake)


def eval_distances(case, got, want=None):
    """(|got - want| / |want|, the same over count x EVAL_GATE) for every finite, nonzero oracle value: the second is the figure the
    gate bounds by 1."""
    metrics, counts = eval_expected(case) if want is None else want
    got = np.asarray(got, dtype=np.float64)
    ok = np.isfinite(metrics) & (metrics != 0) & np.isfinite(got)
    with np.errstate(all="ignore"):
        relative = np.abs(got - metrics) / np.abs(metrics)
        in_gates = relative / (counts[:, None] * EVAL_GATE)
    return relative[ok], in_gates[ok]


def eval_mismatches(case, got, want=None, reference=None):
    """What the GPU test asserts to be empty.  got: N x 4 float64.  Each metric within count * EVAL_GATE relative of eval_oracle,
    within REFERENCE_RTOL of evaluation_metrics where that is finite, NaN and inf exactly where either oracle has them."""
    metrics, counts = eval_expected(case) if want is None else want
    reference = reference_metrics(case) if reference is None else reference
    got = np.asarray(got)
    if got.shape != metrics.shape or got.dtype != np.float64:
        return [f"{got.dtype} {got.shape}, expected float64 {metrics.shape}"]
    found = []
    for i in range(metrics.shape[0]):
        for k, what in enumerate(("MAE", "RMSE", "iMAE", "iRMSE")):
            g, w, r = float(got[i, k]), float(metrics[i, k]), float(reference[i, k])
            for name, x in (("float64 oracle", w), ("evaluation_metrics", r)):
                if not np.isfinite(x) and not (np.isnan(g) if np.isnan(x) else g == x):
                    found.append(f"frame {i} {what}: {g!r} where the {name} has {x!r}")
            if np.isfinite(w) and not abs(g - w) <= counts[i] * EVAL_GATE * abs(w):
                found.append(f"frame {i} {what}: {g!r}, float64 oracle {w!r}: {abs(g - w) / max(abs(w), 1e-300):.3e} relative, "
                             f"gate {counts[i] * EVAL_GATE:.3e} (count {int(counts[i])})")
            if np.isfinite(r) and not abs(g - r) <= REFERENCE_RTOL * abs(r):
                found.append(f"frame {i} {what}: {g!r}, evaluation_metrics {r!r}: more than {REFERENCE_RTOL} relative")
    return found


def eval_masked_out(case):
    """Pixels per frame that the mask drops: what a case with planted boundary or poison values must have."""
    _, counts = eval_expected(case)
    return case["output_depth"][0].size - counts


# ========================================================================================================================= unpack
UNPACK_MISTAKES = ("alpha_first", "gray_not_replicated", "signed_depth", "x_offset_ignored", "tail_dropped")
DEPTH_SAMPLES = (0, 255, 256, 32767, 32768, 65535)


def unpack_oracle(image_u8, depth_raw, width=None, x_offset=0, mistake=None):
    """(image N x 3 x H x W float32 in 0 .. 255 or None, sparse depth N x 1 x H x W float32 = sample / 256 or None) from decoded pixels:
    image_u8 N x H x Wraw x C uint8 (gray replicated, alpha dropped, as PIL's convert('RGB') does), depth_raw N x H x W uint16 or uint8."""
    assert mistake is None or mistake in UNPACK_MISTAKES, mistake
    image = depth = None
    if image_u8 is not None:
        c = image_u8.shape[3]
        width = image_u8.shape[2] if width is None else width
        x0 = 0 if mistake == "x_offset_ignored" else x_offset
        px = image_u8[:, :, x0:x0 + width, :]
        if c == 1:
            rest = np.zeros_like(px) if mistake == "gray_not_replicated" else px
            px = np.concatenate([px, rest, rest], axis=3)
        elif c == 4:
            px = px[..., 1:4] if mistake == "alpha_first" else px[..., :3]
        image = np.ascontiguousarray(np.transpose(px, (0, 3, 1, 2))).astype(F32)
    if depth_raw is not None:
        samples = depth_raw.view(np.int16) if mistake == "signed_depth" and depth_raw.dtype == np.uint16 else depth_raw
        depth = (samples.astype(F32) / F32(256.0))[:, None]
    if mistake == "tail_dropped":       # the columns past the last whole group of four are never written
        for out in (image, depth):
            if out is not None:
                out[..., (out.shape[-1] // 4) * 4:] = SENTINEL
    return image, depth


def _unpack_case(n, h, w, c=3, raw=None, x_offset=0, depth="u16", image=True):
    raw = w if raw is None else raw
    kind = {"u16": 0, "u8": 1, None: 2}[depth]
    rng = np.random.default_rng([41, n, h, w, c, raw, x_offset, kind, int(image)])
    img = rng.integers(0, 256, size=(n, h, raw, c), dtype=np.uint8) if image else None
    dep = None
    if depth == "u16":
        dep = rng.integers(0, 65536, size=(n, h, w), dtype=np.uint16)
        flat = dep.reshape(-1)
        at = rng.permutation(flat.size)[:len(DEPTH_SAMPLES)]
        flat[at] = np.array(DEPTH_SAMPLES, dtype=np.uint16)[:at.size]
        if flat.size < len(DEPTH_SAMPLES):
            flat[0] = 32768 + flat.size         # the frames too small for all six still carry a sample with the top bit set
    elif depth == "u8":
        dep = rng.integers(0, 256, size=(n, h, w), dtype=np.uint8)
    name = f"n{n} h{h} w{w} " + (f"c{c} raw{raw} x{x_offset}" if image else "no image") + f" depth {depth}"
    return dict(name=name, image_u8=img, depth_raw=dep, width=w, x_offset=x_offset, quads=n * h * ((w + 3) // 4))


UNPACK_WIDTHS = (1, 3, 5, 64, 67)


def unpack_cases(c):
    """Image cases of one channel count: every width, batch and height, the whole image and each third of a triplet, with 16-bit depth;
    then the raw width 3 W + 2 with x_offset 1, 8-bit depth, and the image alone with several frames.  n3 h7 w67 is 357 quads of four
    pixels: more than one block of 256 threads."""
    cases = []
    for w in UNPACK_WIDTHS:
        for n in (1, 3):
            for h in (1, 7):
                cases.append(_unpack_case(n, h, w, c))
                cases += [_unpack_case(n, h, w, c, raw=3 * w, x_offset=x) for x in (0, w, 2 * w)]
        cases.append(_unpack_case(3, 7, w, c, raw=3 * w + 2, x_offset=1))
        cases.append(_unpack_case(3, 7, w, c, raw=3 * w, x_offset=w, depth="u8"))
        cases.append(_unpack_case(3, 7, w, c, raw=3 * w, x_offset=w, depth=None))
    return cases


def unpack_depth_only_cases():
    return [_unpack_case(n, h, w, depth=d, image=False) for w in UNPACK_WIDTHS for n, h in ((1, 1), (3, 7)) for d in ("u16", "u8")]


def unpack_all_cases():
    return [case for c in (1, 3, 4) for case in unpack_cases(c)] + unpack_depth_only_cases()


def unpack_expected(case, mistake=None):
    return unpack_oracle(case["image_u8"], case["depth_raw"], case["width"], case["x_offset"], mistake=mistake)


def unpack_mismatches(case, got, want=None):
    """What the GPU test asserts to be empty: got = (image or None, depth or None) against the oracle bit for bit."""
    want = unpack_expected(case) if want is None else want
    return [f for role, g, w in zip(("image", "depth"), got, want) for f in _bit_findings(role, g, w)]
