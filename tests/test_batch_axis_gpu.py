"""GPU tests of the batch axis.  Every split-operand kernel places its fp16 windows on per-frame state (absmax slots, pair
scales, per-tile maxima) and decodes a linear block id into (frame, tile); a frame read through another frame's window,
scale or partial sums is what these tests catch.  Batches of 1, 3, 5 and 17 frames, each frame with a magnitude of its own
(powers of two from 2^-24 to 2^24, one all-zero frame in the middle), and per frame:
  (a) the bars of the n = 2 test of the same kernel against an fp64 evaluation, in units of that frame's (and filter's) rms;
  (b) the output slot holds max |out| of that frame, bit for bit (pair outputs: a window within 2^16 of the data);
  (c) the permuted batch gives the permuted outputs, bit for bit;
  (d) the frame run alone gives the bits it had in the batch;
  (e) the all-zero frame gives the exact result (zeros, or what the coordinate channels alone make).
At model level: the bench's 32-frame KITTI batch with per-frame variations on both sides of the 16-frame graph branches.

    python -m pytest tests/test_batch_axis_gpu.py -m gpu -q
"""
import random

import pytest
import torch

import kbnet_amd as kb
from conftest import rel_err
from oracle import kbnet_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 1e-4
TIGHT = 2e-5
NS = (1, 3, 5, 17)   # 17: odd, above one graph branch's 16 frames; most block counts are then no multiple of 8
lrelu = torch.nn.functional.leaky_relu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need a visible MI355X (run with -m gpu on a GPU box)")
    kb._lib.load()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ helpers
_EXPS = list(range(-24, 25, 3))       # 17 binades, 2^-24 .. 2^24
random.Random(5).shuffle(_EXPS)


def frame_scales(n, lo=-24, hi=24):
    """One power of two per frame, from 2^lo to 2^hi in a fixed shuffled order; with n >= 3 the middle frame is zero."""
    s = torch.tensor([2.0 ** (lo + round((e + 24) * (hi - lo) / 48)) for e in _EXPS[:n]], dtype=torch.float64)
    if n >= 3:
        s[n // 2] = 0.0
    return s


def scaled(t, s):
    """t[i] x s[i]: exact (powers of two far from the fp32 range's ends)."""
    return (t.double() * s.view(-1, *[1] * (t.dim() - 1))).float()


def permutation(n):
    p = torch.randperm(n, generator=torch.Generator().manual_seed(100 + n))
    return torch.roll(p, 1) if n > 1 and torch.equal(p, torch.arange(n)) else p


def slot_of(slot):
    return kb.ops.slot_values(slot).clone()


def check_slot(name, slot_vals, t):
    """(b): the slot holds max |t| of every frame, bit for bit."""
    assert torch.equal(slot_vals.cpu(), t.abs().amax(dim=tuple(range(1, t.dim()))).cpu()), f"{name}: absmax slot"


def check_frames(name, got, r64, r32, max_bar=2e-5):
    """(a) + (e), frame by frame: errors in units of each (frame, filter)'s rms -- rms within max(3.5 x the fp32 reference's, 6e-7)
    and below 1.5e-6, max below `max_bar`; a frame whose exact result is all zero must be exactly zero."""
    got = got.detach().cpu().double()
    for i in range(got.shape[0]):
        ref = r64[i]
        if float(ref.abs().max()) == 0.0:
            assert float(got[i].abs().max()) == 0.0, f"{name}: frame {i} is zero and must stay exactly zero"
            continue
        rms = ref.pow(2).mean(dim=(1, 2), keepdim=True).sqrt().clamp_min(1e-300)
        e = ((got[i] - ref) / rms).abs()
        eo = ((r32[i].double() - ref) / rms).abs()
        rh, ro, mh = float(e.pow(2).mean().sqrt()), float(eo.pow(2).mean().sqrt()), float(e.max())
        assert rh < max(3.5 * ro, 6e-7) and rh < 1.5e-6 and mh < max_bar, f"{name}: frame {i}: rms {rh:.2e} (fp32 {ro:.2e}) max {mh:.2e}"


def pair_errs_frame(got, ref64):
    """tests/test_hip_parity.py _pair_errs for one frame: rms / max error over the filters within 2^-9 of the frame's maximum."""
    rms = ref64.pow(2).mean(dim=(1, 2), keepdim=True).sqrt()
    live = rms >= ref64.abs().amax() * 2.0 ** -9
    e = ((got.double() - ref64) / rms.clamp_min(1e-300)).abs() * live
    return float((e.pow(2).sum() / (live.sum() * ref64.shape[1] * ref64.shape[2])).sqrt()), float(e.max())


def check_pair_frames(name, got, got_f32, ref64, rms_floor, max_floor):
    """Pair-format bars per frame: within 1.5x (rms) / 2x (max) of the fp32-output form of the same kernel."""
    got, got_f32 = got.detach().cpu(), got_f32.detach().cpu()
    for i in range(got.shape[0]):
        if float(ref64[i].abs().max()) == 0.0:
            assert float(got[i].abs().max()) == 0.0, f"{name}: frame {i} is zero and must stay exactly zero"
            continue
        rp, mp = pair_errs_frame(got[i], ref64[i])
        rf, mf = pair_errs_frame(got_f32[i], ref64[i])
        assert rp < max(1.5 * rf, rms_floor) and mp < max(2.0 * mf, max_floor), f"{name}: frame {i}: pair rms {rp:.2e} max {mp:.2e}, fp32 {rf:.2e} / {mf:.2e}"


def check_batch_axis(run, frames):
    """(c) and (d).  `run(frames)` -> dict of tensors with the frame as dim 0 (outputs, slot values, pair data and scales);
    `frames`: device tensors with the frame as dim 0.  Returns the batch's result."""
    out = run(frames)
    n = frames[0].shape[0]
    if n > 1:
        p = permutation(n)
        pd = p.to(frames[0].device)
        got = run([f[pd] for f in frames])
        for k, v in out.items():
            assert torch.equal(got[k], v[pd]), f"{k}: the permuted batch {p.tolist()} must give the permuted outputs"
        for i in range(n):
            alone = run([f[i:i + 1] for f in frames])
            for k, v in out.items():
                assert torch.equal(alone[k], v[i:i + 1]), f"{k}: frame {i} alone must give the bits it had in the batch of {n}"
    return out


def kmats(n, h, w):
    k = torch.tensor([[60.0, 0.0, w / 2.0], [0.0, 58.0, h / 2.0], [0.0, 0.0, 1.0]]).repeat(n, 1, 1)
    k[:, 0, 0] += torch.arange(n, dtype=torch.float32) * 1.5      # every frame its own focal length
    return k


# ------------------------------------------------------------------------------------- absmax_frames
@pytest.mark.parametrize("chw", [(16, 22, 76), (3, 7, 5), (1, 1, 3), (5, 9, 13)])   # per-frame sizes: multiples of 4 and not
@pytest.mark.parametrize("n", NS)
def test_absmax_frames_every_frame(dev, chw, n):
    """kbn_absmax_frames: slot i = max |t[i]|, bit for bit, for every frame -- dense batches and a channel slice (batch stride
    other than C x H x W, odd offsets); a permuted batch permutes the slot."""
    c, h, w = chw
    g = torch.Generator().manual_seed(n * 31 + c * h * w)
    s = frame_scales(n)
    wide = scaled(torch.randn(n, c + 3, h, w, generator=g), s).to(dev)
    for t in (wide[:, :c].contiguous(), wide[:, 1:1 + c], wide[:, 3:]):
        stats = kb.ops.ActStats(n, dev)
        check_slot("absmax_frames", slot_of(stats.measure(t)), t)
        if n > 1:
            p = permutation(n).to(dev)
            stats = kb.ops.ActStats(n, dev)
            assert torch.equal(slot_of(stats.measure(t[p])), slot_of(kb.ops.ActStats(n, dev).measure(t))[p])


# ------------------------------------------------------------------------------------- conv3x3_split
CONV_FORMS = {
    # name: (source channels, filters, output size, kind, source 0 as a channel slice of a wider tensor)
    "plain_tail_tiles": ((64, 64), 64, (22, 76), "plain", True),    # width % 32 = 12: the transposed tail tiles of the MIXED grid
    "plain": ((32,), 48, (16, 64), "plain", False),                 # whole 32-column tiles
    "plain_130_filters": ((16, 32), 130, (9, 40), "plain", True),    # a partial filter block, width % 32 = 8
    "stride2": ((48,), 96, (23, 44), "s2", False),
    "stride2_small": ((16,), 64, (5, 8), "s2", True),
    "up_64_tp64_tail": ((64,), 128, (22, 76), "up", False),          # 64-filter tiles, low-resolution width 38: the TP64 tail
    "up_64": ((16,), 64, (6, 12), "up", False),                      # 64-filter tiles, no tail
    "up_narrow16": ((64,), 12, (36, 76), "up", False),               # <= 16 filters: the 16-filter tiles
    "transposed": ((64,), 64, (22, 76), "tr", False),
}


def _conv_ref(xcat, wt, kind, dt):
    """The layer in dtype `dt` (fp64: torch; fp32: the oracle's conv, torch's for the transposed conv)."""
    if kind == "tr":
        y = torch.nn.functional.conv_transpose2d(xcat.to(dt), wt.to(dt), stride=2, padding=1, output_padding=1)
        return lrelu(y, 0.2)
    if kind == "up":
        xcat = torch.nn.functional.interpolate(xcat, scale_factor=2, mode="nearest")
    stride = 2 if kind == "s2" else 1
    if dt == torch.float64:
        return lrelu(torch.nn.functional.conv2d(xcat.double(), wt.double(), stride=stride, padding=1), 0.2)
    return orc.conv2d(xcat, wt, stride, 0.2)


def _conv_case(form, n, seed):
    cins, cout, (h, w), kind, sliced = CONV_FORMS[form]
    g = torch.Generator().manual_seed(seed + sum(cins) + cout + h)
    sh, sw = (h // 2, w // 2) if kind in ("up", "tr") else ((2 * h - 1, 2 * w) if kind == "s2" else (h, w))
    s = frame_scales(n)
    xs = [scaled(lrelu(torch.randn(n, c, sh, sw, generator=g), 0.2), s) for c in cins]
    cin = sum(cins)
    if kind == "tr":
        wt = torch.randn(cin, cout, 3, 3, generator=g) / (cin * 9 / 4) ** 0.5
        wt[:, 1] *= 1e-3
        wt[:, 2] *= 50.0
    else:
        wt = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
        wt[1] *= 1e-3                     # filters of very different magnitude: the per-filter exponent
        wt[2] *= 50.0
    frames = []
    for j, x in enumerate(xs):
        if sliced and j == 0:             # the batch stride is not C x H x W
            wide = torch.randn(n, x.shape[1] + 9, sh, sw, generator=g)
            wide[:, 5:5 + x.shape[1]] = x
            frames.append(wide)
        else:
            frames.append(x)
    return cins, cout, h, w, kind, sliced, xs, wt, frames


def _srcs_of(fr, cins, sliced):
    return [f[:, 5:5 + c] if (sliced and j == 0) else f for j, (f, c) in enumerate(zip(fr, cins))]


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("form", list(CONV_FORMS))
def test_conv3x3_split_batch_axis(dev, form, n):
    """kbn_conv3x3_split_forward, every form (plain with and without the transposed tail tiles, stride 2, the folded up-conv's
    64-filter tiles with and without the TP64 tail and its 16-filter tiles, the transposed conv): (a)-(e) per frame."""
    cins, cout, h, w, kind, sliced, xs, wt, frames = _conv_case(form, n, 0)
    up = kind in ("up", "tr")
    stride = 2 if kind == "s2" else 1
    xcat = torch.cat(xs, 1)
    ref64, ref32 = _conv_ref(xcat, wt, kind, torch.float64), _conv_ref(xcat, wt, kind, torch.float32)
    assert tuple(ref64.shape) == (n, cout, h, w)
    packed = kb.ops.pack_conv3x3_split_weight(wt.to(dev), stride=stride, folded_up2x=up, transposed=kind == "tr")

    def run(fr):
        nn = fr[0].shape[0]
        stats = kb.ops.ActStats(nn, dev)
        src_t = _srcs_of(fr, cins, sliced)
        slots = [stats.measure(x) for x in src_t]
        out = torch.full((nn, cout, h, w), float("nan"), device=dev)
        slot = stats.new()
        res = kb.ops.conv3x3_split([kb.ops.tensor_src(x, "x", sl) for x, sl in zip(src_t, slots)], packed, nn, cout, h, w, out,
                                   up2x=up, negative_slope=0.2, stride=stride, folded_up2x=up, transposed=kind == "tr", out_absmax=slot)
        assert res is not None
        return {"out": out, "slot": slot_of(slot), **{f"in_slot{j}": slot_of(sl) for j, sl in enumerate(slots)}}

    res = check_batch_axis(run, [f.to(dev) for f in frames])
    check_slot(form, res["slot"], res["out"])
    for j, x in enumerate(xs):
        check_slot(f"{form} source {j}", res[f"in_slot{j}"], x)
    check_frames(form, res["out"], ref64, ref32)


KSPLIT_FORMS = {"plain": ((64, 64), 64, (22, 76), "plain", 4), "stride2": ((96,), 192, (23, 44), "s2", 3),
                "up_64": ((128,), 128, (36, 140), "up", 3)}


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("form", list(KSPLIT_FORMS))
def test_conv3x3_split_ksplit_batch_axis(dev, form, n):
    """kbn_conv3x3_split_forward_ksplit: the partial planes [ksplit][n][...] and their reduce, per frame; a frame alone at the same
    ksplit gives its bits; within the suite's single-op tolerance of the one-workgroup form."""
    cins, cout, (h, w), kind, ks = KSPLIT_FORMS[form]
    g = torch.Generator().manual_seed(sum(cins) + cout + h + ks)
    up = kind == "up"
    stride = 2 if kind == "s2" else 1
    sh, sw = (h // 2, w // 2) if up else ((2 * h - 1, 2 * w) if stride == 2 else (h, w))
    s = frame_scales(n)
    xs = [scaled(lrelu(torch.randn(n, c, sh, sw, generator=g), 0.2), s) for c in cins]
    cin = sum(cins)
    wt = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    wt[1] *= 1e-3
    xcat = torch.cat(xs, 1)
    ref64, ref32 = _conv_ref(xcat, wt, kind, torch.float64), _conv_ref(xcat, wt, kind, torch.float32)
    packed = kb.ops.pack_conv3x3_split_weight(wt.to(dev), stride=stride, folded_up2x=up)
    kw = dict(negative_slope=0.2, stride=stride, up2x=up, folded_up2x=up)

    def run(fr):
        nn = fr[0].shape[0]
        stats = kb.ops.ActStats(nn, dev)
        srcs = [kb.ops.tensor_src(x, "x", stats.measure(x)) for x in fr]
        out = torch.full((nn, cout, h, w), float("nan"), device=dev)
        base = torch.full_like(out, float("nan"))
        slot = stats.new()
        assert kb.ops.conv3x3_split(srcs, packed, nn, cout, h, w, out, out_absmax=slot, ksplit=ks, **kw) is not None
        assert kb.ops.conv3x3_split(srcs, packed, nn, cout, h, w, base, **kw) is not None
        return {"out": out, "slot": slot_of(slot), "base": base}

    res = check_batch_axis(run, [x.to(dev) for x in xs])
    out = res["out"]
    check_slot(form, res["slot"], out)
    got = out.cpu().double()
    for i in range(n):
        if float(ref64[i].abs().max()) == 0.0:
            assert float(got[i].abs().max()) == 0.0, f"frame {i} is zero"
            continue
        rms = ref64[i].pow(2).mean(dim=(1, 2), keepdim=True).sqrt()
        e = ((got[i] - ref64[i]) / rms).abs()
        assert float(e.pow(2).mean().sqrt()) < 1.5e-6 and float(e.max()) < 2e-5, f"frame {i}: rms {float(e.pow(2).mean().sqrt()):.2e} max {float(e.max()):.2e}"
        assert rel_err(out[i], ref32[i]) < TIGHT and rel_err(out[i], res["base"][i]) < TIGHT, f"frame {i}"


# ---------------------------------------------------------------------------- pair tensors in and out
PAIR_FORMS = {
    # name: (source channels, filters, output size, kind)
    "concat": ((64, 64), 64, (22, 76), "plain"),
    "concat_odd": ((16, 32), 72, (9, 33), "plain"),
    "stride2": ((48,), 96, (23, 44), "s2"),
    "stride2_sub": ((48,), 96, (23, 44), "s2_sub"),
    "up_64": ((32,), 64, (22, 76), "up"),
    "up_narrow16": ((64,), 12, (36, 76), "up"),
}


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("form", list(PAIR_FORMS))
def test_pair_out_batch_axis(dev, form, n):
    """conv3x3_split(out=PairTensor): the per-frame 2^k from the bound of each frame's own sources, written by every workgroup of that
    frame.  Decoded against fp64 per frame (the bars of the n = 2 pair tests), slot exact, window within 2^16 of each frame's data,
    the side output of the stride-2 form (with_sub) the fp32 result's even pixels; data, scales and slots permute and stand alone."""
    cins, cout, (h, w), kind = PAIR_FORMS[form]
    g = torch.Generator().manual_seed(sum(cins) + cout + h + 3)
    up = kind == "up"
    stride = 2 if kind.startswith("s2") else 1
    sh, sw = (h // 2, w // 2) if up else ((2 * h - 1, 2 * w) if stride == 2 else (h, w))
    s = frame_scales(n)
    xs = [scaled(lrelu(torch.randn(n, c, sh, sw, generator=g), 0.2), s) for c in cins]
    cin = sum(cins)
    wt = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    wt[1] *= 1e-3
    wt[2] *= 50.0
    xcat = torch.cat(xs, 1)
    ref64 = _conv_ref(xcat, wt, kind[:2] if stride == 2 else kind, torch.float64)
    packed = kb.ops.pack_conv3x3_split_weight(wt.to(dev), stride=stride, folded_up2x=up)
    cp = 16 if (up and cout <= 16) else cout
    kw = dict(negative_slope=0.2, stride=stride, up2x=up, folded_up2x=up)

    def run(fr):
        nn = fr[0].shape[0]
        stats = kb.ops.ActStats(nn, dev)
        srcs = [kb.ops.tensor_src(x, "x", stats.measure(x)) for x in fr]
        out32 = torch.empty(nn, cout, h, w, device=dev)
        assert kb.ops.conv3x3_split(srcs, packed, nn, cout, h, w, out32, **kw) is not None
        pt = kb.ops.PairTensor(nn, cp, h, w, dev, stats)
        if kind == "s2_sub":
            pt.with_sub()
            pt.sub.fill_(float("nan"))
        pt.data.fill_(float("nan"))
        assert kb.ops.conv3x3_split(srcs, packed, nn, cout, h, w, pt, **kw) is not None
        r = {"data": pt.data, "scale": pt.scale, "slot": slot_of(pt.absmax), "out32": out32, "dec": pt.float(),
             "slack": pt.window_slack_log2()}
        if pt.sub is not None:
            r["sub"] = pt.sub
        return r

    res = check_batch_axis(run, [x.to(dev) for x in xs])
    assert torch.isfinite(res["data"]).all(), "every granule, the zero granules included, is written"
    assert float(res["data"][:, :, :, h * w].abs().max()) == 0.0
    check_slot(form, res["slot"], res["out32"])
    live = res["slot"].cpu() > 0
    assert float(res["slack"].cpu()[live].max()) < 16 and float(res["slack"].cpu()[live].min()) >= 0, res["slack"].tolist()
    if cp > cout:
        assert float(res["dec"][:, cout:].abs().max()) == 0.0, "channels past the last filter are zero"
    if kind == "s2_sub":
        assert torch.equal(res["sub"], res["out32"][:, :, ::2, ::2]), "the side output: the fp32 result at the even pixels"
    check_pair_frames(form, res["dec"][:, :cout], res["out32"], ref64, 2e-7, 2e-6)


PAIR_SRC_FORMS = {"into_stride2": (48, 96, 192, (23, 44), "s2"), "into_up_64": (32, 64, 128, (22, 76), "up")}


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("form", list(PAIR_SRC_FORMS))
def test_pair_src_batch_axis(dev, form, n):
    """A PairTensor as source 0 (KBN_SRC_PAIR): the consumer stages frame i's planes under frame i's scale.  The producer is a
    concat conv (stride 2 for the stride-2 consumer); against the same consumer on the DECODED tensor, both vs fp64, per frame."""
    c0, c1, c2, (h, w), kind = PAIR_SRC_FORMS[form]
    g = torch.Generator().manual_seed(c0 + c1 + c2 + h)
    s = frame_scales(n)
    mid_stride = 2 if kind == "s2" else 1
    ph, pw = (h // 2, w // 2) if kind == "up" else (h, w)              # the pair tensor's size
    x0 = scaled(lrelu(torch.randn(n, c0, *((2 * ph - 1, 2 * pw) if mid_stride == 2 else (ph, pw)), generator=g), 0.2), s)
    w1 = torch.randn(c1, c0, 3, 3, generator=g) / (c0 * 9) ** 0.5
    w2 = torch.randn(c2, c1, 3, 3, generator=g) / (c1 * 9) ** 0.5
    w2[1] *= 1e-3
    p1 = kb.ops.pack_conv3x3_split_weight(w1.to(dev), stride=mid_stride)
    up = kind == "up"
    stride = 2 if kind == "s2" else 1
    oh, ow = ((ph + 1) // 2, (pw + 1) // 2) if stride == 2 else (h, w)
    p2 = kb.ops.pack_conv3x3_split_weight(w2.to(dev), stride=stride, folded_up2x=up)
    kw = dict(negative_slope=0.2, stride=stride, up2x=up, folded_up2x=up)

    def run(fr):
        nn = fr[0].shape[0]
        stats = kb.ops.ActStats(nn, dev)
        pt = kb.ops.PairTensor(nn, c1, ph, pw, dev, stats)
        assert kb.ops.conv3x3_split([kb.ops.tensor_src(fr[0], "x", stats.measure(fr[0]))], p1, nn, c1, ph, pw, pt, negative_slope=0.2,
                                    stride=mid_stride) is not None
        dec = pt.float()
        out_f32 = torch.empty(nn, c2, oh, ow, device=dev)
        assert kb.ops.conv3x3_split([kb.ops.tensor_src(dec, "x", pt.absmax)], p2, nn, c2, oh, ow, out_f32, **kw) is not None
        out = torch.full((nn, c2, oh, ow), float("nan"), device=dev)
        slot = stats.new()
        assert kb.ops.conv3x3_split([kb.ops.pair_src(pt, "x")], p2, nn, c2, oh, ow, out, out_absmax=slot, **kw) is not None
        return {"out": out, "slot": slot_of(slot), "f32": out_f32, "dec": dec}

    res = check_batch_axis(run, [x0.to(dev)])
    check_slot(form, res["slot"], res["out"])
    ref64 = _conv_ref(res["dec"].cpu(), w2, kind, torch.float64)
    check_pair_frames(form, res["out"], res["f32"], ref64, 3e-7, 3e-6)


# ----------------------------------------------------------------------------------- conv1x1s2_split
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("ci,cf,cd,cout,hw", [(48, 48, 16, 96, (35, 70)), (16, 32, 5, 130, (9, 131)), (48, 0, 16, 48, (38, 67))])
def test_conv1x1s2_split_batch_axis(dev, ci, cf, cd, cout, hw, n):
    """kbn_conv1x1s2_split_forward + kbn_kb_xyz_s2_forward (the KB block's conv_fused): image, fused and depth of frame i x s_i (the
    backprojection channels scale with the depth), intrinsics per frame; the fused source a channel slice of a wider tensor."""
    h, w = hw
    oh, ow = (h + 1) // 2, (w + 1) // 2
    g = torch.Generator().manual_seed(ci + cf + cout + h + n)
    s = frame_scales(n)
    image = scaled(lrelu(torch.randn(n, ci, h, w, generator=g), 0.2), s)
    fwide = scaled(lrelu(torch.randn(n, cf + 7, h, w, generator=g), 0.2), s)
    depth = scaled(lrelu(torch.randn(n, cd, h, w, generator=g), 0.2), s)
    proj = torch.randn(1, cd, 1, 1, generator=g) / cd ** 0.5
    kmat = kmats(n, h, w)
    cin = ci + 3 + cf
    wt = torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5
    wt[1] *= 1e-3
    wt[2] *= 50.0
    fused = fwide[:, 4:4 + cf]
    coords = orc.camera_coordinates(kmat, h, w)
    z64 = lrelu(torch.nn.functional.conv2d(depth.double(), proj.double()), 0.2)
    cat64 = torch.cat([image.double(), coords.double() * z64] + ([fused.double()] if cf else []), 1)
    ref64 = lrelu(torch.nn.functional.conv2d(cat64, wt.double(), stride=2), 0.2)
    cat32 = torch.cat([image, coords * lrelu(orc.conv2d(depth, proj, 1, None), 0.2)] + ([fused] if cf else []), 1)
    ref32 = orc.conv2d(cat32, wt, 2, 0.2)
    packed = kb.ops.pack_conv1x1s2_split_weight(wt.to(dev), ci)
    projd = proj.to(dev)

    def run(fr):
        im, fw, dp, km = fr
        nn = im.shape[0]
        kinv = kb.ops.intrinsics_inverse(km)
        xyz = kb.ops.kb_xyz_s2(dp, projd, kinv, 0.2)
        stats = kb.ops.ActStats(nn, dev)
        srcs = [kb.ops.tensor_src(im, "image", stats.measure(im))]
        if cf:
            fu = fw[:, 4:4 + cf]
            srcs.append(kb.ops.tensor_src(fu, "fused", stats.measure(fu)))
        out = torch.full((nn, cout, oh, ow), float("nan"), device=dev)
        slot = stats.new()
        assert kb.ops.conv1x1s2_split(srcs, packed, xyz, nn, cout, oh, ow, out, negative_slope=0.2, out_absmax=slot) is not None
        return {"out": out, "slot": slot_of(slot), "xyz": xyz}

    res = check_batch_axis(run, [image.to(dev), fwide.to(dev), depth.to(dev), kmat.to(dev)])
    check_slot("conv1x1s2_split", res["slot"], res["out"])
    check_frames("conv1x1s2_split", res["out"], ref64, ref32)
    xyz64 = (coords.double() * z64)[:, :, ::2, ::2]
    for i in range(n):
        assert rel_err(res["xyz"][i], xyz64[i]) < TIGHT if float(xyz64[i].abs().max()) > 0 else float(res["xyz"][i].abs().max()) == 0.0


# --------------------------------------------------------------------------------------- the fronts
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("hw,with_next", [((35, 70), False), ((33, 47), False), ((35, 70), True), ((64, 26), True)])
def test_kb1_front_batch_axis(dev, hw, with_next, n):
    """kbn_kb1_front_forward (and _next_forward): conv0_image's per-tile windows and the per-frame windows of the two (three) outputs
    for images of every magnitude; the next level's output a channel slice of a wider tensor."""
    h, w = hw
    oh, ow = (h + 1) // 2, (w + 1) // 2
    h2, w2 = (oh + 1) // 2, (ow + 1) // 2
    g = torch.Generator().manual_seed(h * w + n)
    c, f0, fi, fo = 3, 48, 48, 96
    s = frame_scales(n)
    image = scaled(torch.rand(n, c, h, w, generator=g), s)
    xyz = scaled(torch.randn(n, 3, oh, ow, generator=g), s)
    xyz2 = scaled(torch.randn(n, 3, h2, w2, generator=g), s)
    w0 = torch.randn(f0, c, 3, 3, generator=g) / (c * 9) ** 0.5
    wi = torch.randn(fi, f0, 3, 3, generator=g) / (f0 * 9) ** 0.5
    wf = torch.randn(fi, f0 + 3, 1, 1, generator=g) / (f0 + 3) ** 0.5
    wn = torch.randn(fo, fi + 3 + fi, 1, 1, generator=g) / (2 * fi + 3) ** 0.5
    w0[1] *= 1e-3; wi[2] *= 40.0; wf[3] *= 1e-2; wn[5] *= 30.0; wn[7] *= 1e-3

    def chain(dt, conv):
        x0 = conv(image.to(dt), w0.to(dt), 1)
        img = conv(x0, wi.to(dt), 2)
        up = torch.zeros(n, 3, h, w, dtype=dt)
        up[:, :, ::2, ::2] = xyz.to(dt)
        fus = conv(torch.cat([x0, up], 1), wf.to(dt), 2)
        up2 = torch.zeros(n, 3, oh, ow, dtype=dt)
        up2[:, :, ::2, ::2] = xyz2.to(dt)
        return img, fus, conv(torch.cat([img, up2, fus], 1), wn.to(dt), 2)

    c64 = lambda x, wt, stride: lrelu(torch.nn.functional.conv2d(x, wt, stride=stride, padding=wt.shape[-1] // 2), 0.2)
    r64 = chain(torch.float64, c64)
    r32 = chain(torch.float32, lambda x, wt, stride: orc.conv2d(x, wt, stride, 0.2))
    packed = kb.ops.pack_kb1_front_weight(w0.to(dev), wi.to(dev), wf.to(dev))
    packed_n = kb.ops.pack_kb1_front_next_weight(wn.to(dev), fi) if with_next else None
    assert packed is not None and (packed_n is not None or not with_next)

    def run(fr):
        im, xz, xz2 = fr
        nn = im.shape[0]
        stats = kb.ops.ActStats(nn, dev)
        oi = torch.full((nn, fi, oh, ow), float("nan"), device=dev)
        of = torch.full((nn, fi, oh, ow), float("nan"), device=dev)
        si, sf, sn = stats.new(), stats.new(), stats.new()
        r = {"image": oi, "fused": of}
        if with_next:
            skip = torch.full((nn, fo + 5, h2, w2), float("nan"), device=dev)
            assert kb.ops.kb1_front(im, packed, xz, f0, fi, oi, of, 0.2, 0.2, si, sf, next_fused=(packed_n, xz2, skip[:, 2:2 + fo], 0.2, sn)) is not None
            assert bool(torch.isnan(skip[:, :2]).all()) and bool(torch.isnan(skip[:, 2 + fo:]).all())
            r["next"], r["slot_next"] = skip[:, 2:2 + fo], slot_of(sn)
        else:
            assert kb.ops.kb1_front(im, packed, xz, f0, fi, oi, of, 0.2, 0.2, si, sf) is not None
        r["slot_image"], r["slot_fused"] = slot_of(si), slot_of(sf)
        return r

    res = check_batch_axis(run, [image.to(dev), xyz.to(dev), xyz2.to(dev)])
    for name, j in (("image", 0), ("fused", 1)) + ((("next", 2),) if with_next else ()):
        check_slot(name, res[f"slot_{name}"], res[name])
        check_frames(f"kb1_front {name}", res[name], r64[j], r32[j])


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("hw", [(35, 70), (33, 47)])
def test_kb1_depth_front_batch_axis(dev, hw, n):
    """kbn_kb1_depth_front_forward: conv0_depth's per-tile windows, conv_depth's per-frame slot and the fp32 coordinate channels
    (per-frame intrinsics); the all-zero frame's conv_depth is what the coordinate channels alone give, its xyz exactly zero."""
    h, w = hw
    oh, ow = (h + 1) // 2, (w + 1) // 2
    g = torch.Generator().manual_seed(h * w + 1 + n)
    c, f0, fd = 8, 16, 16
    s = frame_scales(n)
    depth = scaled(lrelu(torch.randn(n, c, h, w, generator=g), 0.2), s)
    w0 = torch.randn(f0, c, 3, 3, generator=g) / (c * 9) ** 0.5
    wc = torch.randn(fd, f0 + 3, 3, 3, generator=g) / ((f0 + 3) * 9) ** 0.5
    proj = torch.randn(1, f0, 1, 1, generator=g) / f0 ** 0.5
    w0[1] *= 1e-3; wc[2] *= 40.0
    kmat = kmats(n, h, w)
    coords = orc.camera_coordinates(kmat, h, w)
    c64 = lambda x, wt, stride: lrelu(torch.nn.functional.conv2d(x.double(), wt.double(), stride=stride, padding=wt.shape[-1] // 2), 0.2)
    x0_64 = c64(depth, w0, 1)
    dep_64 = c64(torch.cat([x0_64, coords.double()], 1), wc, 2)
    xyz_64 = (coords.double() * c64(x0_64, proj, 1))[:, :, ::2, ::2]
    x0_32 = orc.conv2d(depth, w0, 1, 0.2)
    dep_32 = orc.conv2d(torch.cat([x0_32, coords], 1), wc, 2, 0.2)
    xyz_32 = (coords * orc.conv2d(x0_32, proj, 1, 0.2))[:, :, ::2, ::2]
    packed = kb.ops.pack_kb1_depth_front_weight(w0.to(dev), wc.to(dev), proj.to(dev))

    def run(fr):
        dp, km = fr
        nn = dp.shape[0]
        stats = kb.ops.ActStats(nn, dev)
        out = torch.full((nn, fd, oh, ow), float("nan"), device=dev)
        slot = stats.new()
        res = kb.ops.kb1_depth_front(dp, kb.ops.intrinsics_inverse(km), packed, f0, fd, out, 0.2, 0.2, 0.2, out_depth_absmax=slot)
        assert res is not None
        return {"out": out, "xyz": res[1], "slot": slot_of(slot)}

    res = check_batch_axis(run, [depth.to(dev), kmat.to(dev)])
    check_slot("kb1_depth_front", res["slot"], res["out"])
    check_frames("kb1_depth_front conv_depth", res["out"], dep_64, dep_32)
    check_frames("kb1_depth_front xyz", res["xyz"], xyz_64, xyz_32)


def _s2d_case(n, h, w, seed):
    """Sparse depth maps at 30 % density, depths 1-80 m x a per-frame power of two from 2^-8 to 2^3 (the min pool's 999 sentinel
    bounds the range; the validity channel stays 0 / 1): the middle frame an EMPTY map."""
    cfg = kb.kitti_config()
    mins, maxs = list(cfg.min_pools), list(cfg.max_pools)
    g = torch.Generator().manual_seed(seed)
    mask = (torch.rand(n, 1, h, w, generator=g) < 0.3).float()
    z = torch.round((1.0 + 79.0 * torch.rand(n, 1, h, w, generator=g)) * 256.0) / 256.0 * mask
    z = scaled(z, frame_scales(n, -8, 3))
    x = torch.cat([z, (z > 0).float()], 1)
    npool = len(mins) + len(maxs)
    nf = 8
    sd = {"pool_convs.0.conv.weight": torch.randn(nf, npool, 1, 1, generator=g) / npool ** 0.5,
          "pool_convs.1.conv.weight": torch.randn(nf, nf, 1, 1, generator=g) / nf ** 0.5,
          "pool_convs.2.conv.weight": torch.randn(nf, nf, 1, 1, generator=g) / nf ** 0.5,
          "conv.conv.weight": torch.randn(nf, nf + 2, 3, 3, generator=g) / ((nf + 2) * 9) ** 0.5}
    sd["pool_convs.1.conv.weight"][3] *= 1e-2
    sd["conv.conv.weight"][5] *= 30.0
    return mins, maxs, x, sd


@pytest.mark.parametrize("n", NS)
def test_s2d_forward_batch_axis(dev, n):
    """kbn_s2d_forward / kbn_s2d_pyramid (fp32 kernels, the min/max pools bit-exact): per frame against the oracle."""
    h, w = 37, 70
    mins, maxs, x, sd = _s2d_case(n, h, w, 11 + n)
    pyr_ref, out_ref = orc.sparse_to_dense_pool(x, sd, mins, maxs, return_pyramid=True)
    ws = [sd[f"pool_convs.{i}.conv.weight"].to(dev) for i in range(3)]
    wc = sd["conv.conv.weight"].to(dev)

    def run(fr):
        return {"pyr": kb.ops.s2d_pyramid(fr[0], mins, maxs), "out": kb.ops.s2d_forward(fr[0], ws, wc, mins, maxs, 0.2)}

    res = check_batch_axis(run, [x.to(dev)])
    assert torch.equal(res["pyr"].cpu(), pyr_ref)
    for i in range(n):
        if float(out_ref[i].abs().max()) == 0.0:
            assert float(res["out"][i].abs().max()) == 0.0
        else:
            assert rel_err(res["out"][i], out_ref[i]) < TIGHT, i


@pytest.mark.parametrize("n", NS)
def test_s2d_depth_front_batch_axis(dev, n):
    """kbn_s2d_depth_front_forward: S2D's per-tile windows and bounds, conv0_depth's and conv_depth's, for every frame; the empty map
    of the middle frame (every window on the 999 sentinel path) next to maps of other scales."""
    h, w = 35, 70
    oh, ow = (h + 1) // 2, (w + 1) // 2
    mins, maxs, x, sd = _s2d_case(n, h, w, 21 + n)
    g = torch.Generator().manual_seed(5 + n)
    nf, f0, fd = 8, 16, 16
    w0 = torch.randn(f0, nf, 3, 3, generator=g) / (nf * 9) ** 0.5
    wc = torch.randn(fd, f0 + 3, 3, 3, generator=g) / ((f0 + 3) * 9) ** 0.5
    proj = torch.randn(1, f0, 1, 1, generator=g) / f0 ** 0.5
    kmat = kmats(n, h, w)
    coords = orc.camera_coordinates(kmat, h, w)
    s2d_32 = orc.sparse_to_dense_pool(x, sd, mins, maxs)
    x0_32 = orc.conv2d(s2d_32, w0, 1, 0.2)
    dep_32 = orc.conv2d(torch.cat([x0_32, coords], 1), wc, 2, 0.2)
    xyz_32 = (coords * orc.conv2d(x0_32, proj, 1, 0.2))[:, :, ::2, ::2]
    torch.set_default_dtype(torch.float64)
    try:
        s2d_64 = orc.sparse_to_dense_pool(x.double(), {k: v.double() for k, v in sd.items()}, mins, maxs)
    finally:
        torch.set_default_dtype(torch.float32)
    c64 = lambda t, wt, stride: lrelu(torch.nn.functional.conv2d(t.double(), wt.double(), stride=stride, padding=wt.shape[-1] // 2), 0.2)
    x0_64 = c64(s2d_64, w0, 1)
    dep_64 = c64(torch.cat([x0_64, coords.double()], 1), wc, 2)
    xyz_64 = (coords.double() * c64(x0_64, proj, 1))[:, :, ::2, ::2]
    assert kb.ops.s2d_depth_front_supported(2, mins, maxs, 3, nf, f0, fd, h, w, 0.2, 0.2)
    packed_s = kb.ops.pack_s2d_depth_front_weight([sd[f"pool_convs.{i}.conv.weight"].to(dev) for i in range(3)], sd["conv.conv.weight"].to(dev))
    packed_d = kb.ops.pack_kb1_depth_front_weight(w0.to(dev), wc.to(dev), proj.to(dev))

    def run(fr):
        xx, km = fr
        nn = xx.shape[0]
        stats = kb.ops.ActStats(nn, dev)
        out = torch.full((nn, fd, oh, ow), float("nan"), device=dev)
        slot = stats.new()
        res = kb.ops.s2d_depth_front(xx, kb.ops.intrinsics_inverse(km), packed_s, packed_d, mins, maxs, f0, fd, out, 0.2, 0.2, 0.2, 0.2,
                                     out_depth_absmax=slot)
        assert res is not None
        return {"out": out, "xyz": res[1], "slot": slot_of(slot)}

    res = check_batch_axis(run, [x.to(dev), kmat.to(dev)])
    check_slot("s2d_depth_front", res["slot"], res["out"])
    check_frames("s2d_depth_front conv_depth", res["out"], dep_64, dep_32, max_bar=3e-5)
    check_frames("s2d_depth_front xyz", res["xyz"], xyz_64, xyz_32, max_bar=3e-5)


# ------------------------------------------------------------------------------------------ conv_tail
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("c,shape,pair", [(12, (37, 72), False), (8, (130, 67), False), (12, (33, 31), False), (12, (36, 76), True)])
def test_conv_tail_batch_axis(dev, c, shape, pair, n):
    """kbn_conv_tail_forward (per-tile windows) and kbn_conv_tail_forward_pair (a 16-channel PairTensor from the narrow folded up-conv,
    per-frame scales): logits per frame against fp64 with the bar of test_conv_tail_kernel, depth against the fp64 head of the frame's
    logits; the all-zero
    frame's logits exactly zero, its depth the head's constant."""
    h, wd = shape
    g = torch.Generator().manual_seed(c * 1000 + h + n)
    s = frame_scales(n)
    wc = torch.randn(c, c, 3, 3, generator=g) * (1.3 / (c * 9) ** 0.5)
    wc[1] *= 1e-2
    wo = torch.randn(1, c, 3, 3, generator=g) * 0.5
    packed = kb.ops.pack_conv_tail_weight(wc.to(dev))
    wod = wo.to(dev)
    if pair:
        cin = 64
        x0 = scaled(lrelu(torch.randn(n, cin, h // 2, wd // 2, generator=g), 0.2), s)
        wu = torch.randn(c, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
        pu = kb.ops.pack_conv3x3_split_weight(wu.to(dev), folded_up2x=True)
        frames = [x0.to(dev)]
    else:
        frames = [scaled(torch.randn(n, c, h, wd, generator=g), s).to(dev)]

    def run(fr):
        nn = fr[0].shape[0]
        r = {}
        if pair:
            stats = kb.ops.ActStats(nn, dev)
            pt = kb.ops.PairTensor(nn, 16, h, wd, dev, stats)
            assert kb.ops.conv3x3_split([kb.ops.tensor_src(fr[0], "x", stats.measure(fr[0]))], pu, nn, c, h, wd, pt, up2x=True,
                                        negative_slope=0.2, folded_up2x=True) is not None
            x = pt
            r["x"] = pt.float()[:, :c]
        else:
            x = r["x"] = fr[0]
        res = kb.ops.conv_tail(x, packed, wod, 1.5, 100.0, 0.2, return_logits=True)
        assert res is not None
        r["depth"], r["logits"] = res
        return r

    res = check_batch_axis(run, frames)
    xin = res["x"].cpu()
    f64 = lrelu(torch.nn.functional.conv2d(xin.double(), wc.double(), padding=1), 0.2)
    l64 = torch.nn.functional.conv2d(f64, wo.double(), padding=1)
    l32 = orc.conv2d(orc.conv2d(xin, wc, 1, 0.2), wo, 1, None)
    d64 = orc.depth_head(l64, 1.5, 100.0)
    lg, d = res["logits"].cpu().double(), res["depth"].cpu().double()
    for i in range(n):
        if float(l64[i].abs().max()) == 0.0:
            assert float(lg[i].abs().max()) == 0.0, f"frame {i}: zero logits"
            assert float((d[i] - d64[i]).abs().max()) <= 2.0 ** -22 * float(d64[i].abs().max()) and float(d[i].max()) == float(d[i].min())
            continue
        rms = l64[i].pow(2).mean().sqrt()
        e_hip = float((((lg[i] - l64[i]) / rms).pow(2).mean()).sqrt())
        e_orc = float((((l32[i].double() - l64[i]) / rms).pow(2).mean()).sqrt())
        assert e_hip < max(3.5 * e_orc, 6e-7) and e_hip < 1.5e-6, f"frame {i}: logits rms {e_hip:.2e}, fp32 {e_orc:.2e}"
        # the head of THIS frame's logits (a frame of 2^12 carries logits in the thousands: the fp32 rounding of the logits alone then
        # moves the depth by more than 1e-4, in any fp32 evaluation)
        dl = orc.depth_head(lg[i], 1.5, 100.0)
        assert float(((d[i] - dl).abs() / dl).max()) < 1e-5, f"frame {i}: depth of the frame's logits"


# -------------------------------------------------------------------------------- model level: batch 32
def _to(dev, frames):
    return [f.to(dev) for f in frames]


def bench_batch(h=352, w=1216):
    """make_frames(32) with per-frame variations on both sides of the 16-frame graph branches (index 15 | 16).  Returns the
    frames and {index: variation}."""
    image, sparse, valid, k = [f.clone() for f in kb.synthetic.make_frames(32, h, w, "kitti", seed=1, jitter_intrinsics=0.1)]
    vi, vs, vv, vk = kb.synthetic.make_frames(2, h, w, "void", seed=4, jitter_intrinsics=0.1)
    mods = {15: "image x 255", 16: "sparse x 10", 3: "sparse x 0.1", 20: "empty sparse map", 9: "VOID statistics",
            25: "VOID statistics", 12: "black image", 31: "black image + empty sparse map"}
    image[15] *= 255.0
    sparse[16] *= 10.0
    sparse[3] *= 0.1
    for i in (20, 31):
        sparse[i] = 0.0
        valid[i] = 0.0
    for i, j in ((9, 0), (25, 1)):
        image[i], sparse[i], valid[i], k[i] = vi[j], vs[j], vv[j], vk[j]
    image[12] = 0.0
    image[31] = 0.0
    return (image, sparse, valid, k), mods


def _oracle(cfg, sds, fr):
    return orc.kbnet_forward(*fr, *sds, cfg.min_pools, cfg.max_pools, cfg.min_predict_depth, cfg.max_predict_depth)


def _oracle64(cfg, sds, fr):
    torch.set_default_dtype(torch.float64)      # the oracle's pixel grid follows the default dtype (reference quirk Q8)
    try:
        return orc.kbnet_forward(*[f.double() for f in fr], *[{k_: v.double() for k_, v in d.items()} for d in sds],
                                 cfg.min_pools, cfg.max_pools, cfg.min_predict_depth, cfg.max_predict_depth)
    finally:
        torch.set_default_dtype(torch.float32)


PERMUTATIONS = {"reverse": list(range(31, -1, -1)), "halves swapped": list(range(16, 32)) + list(range(16)),
                "cross-branch shuffle": torch.randperm(32, generator=torch.Generator().manual_seed(7)).tolist()}


def test_forward_batch32_every_frame(dev, slow):
    """The bench's batch (KITTI 352 x 1216, 32 frames) with a scale, a statistics or an empty input of its own in eight frames on both
    sides of the graph branches' boundary.  Eager = replay of capture() (2 x 16) = replay of capture(split_graphs=True), bit for
    bit; every frame alone gives its batch bits; reversed, half-swapped and shuffled batches -- eager and replayed through the graph
    captured in the original order -- give the permuted outputs.  Against the oracle (test_forward_follows_input_scale_without_calibration's
    criterion) for every varied frame, and the 1e-4 gate for frames 0, 7 and 23; under --slow the criterion for all 32."""
    cfg = kb.kitti_config()
    sds = kb.synthetic.make_state_dicts(cfg, seed=0, gain=kb.synthetic.PARITY_GAIN["kitti"])
    frames, mods = bench_batch()
    m = kb.modules.KBNetModel.from_config(cfg, dev)
    m.load_state_dicts(*sds)
    dframes = _to(dev, frames)
    out = m.forward(*dframes).clone()
    assert torch.isfinite(out).all()
    replay = m.capture(*dframes)
    assert replay.branches == 2
    assert torch.equal(replay(*dframes), out), "graph replay (2 x 16 frames) = the eager batch"
    split = m.capture(*dframes, split_graphs=True)
    assert torch.equal(split(*dframes), out), "one graph per sub-batch = the eager batch"
    for i in range(32):
        assert torch.equal(m.forward(*[f[i:i + 1] for f in dframes]), out[i:i + 1]), f"frame {i} ({mods.get(i, 'plain')}) alone"
    for name, p in PERMUTATIONS.items():
        pd = torch.tensor(p, device=dev)
        pf = [f[pd] for f in dframes]
        assert torch.equal(m.forward(*pf), out[pd]), f"eager, {name}"
        assert torch.equal(replay(*pf), out[pd]), f"graph captured in the original order, {name}"
    rel = lambda a, b: float(((a.double() - b.double()).abs() / b.double().abs()).max())
    worst = (0.0, -1)
    for i in (range(32) if slow else sorted({0, 7, 15, 16, 23, 31} | set(mods))):
        fr = [f[i:i + 1] for f in frames]
        got = out[i:i + 1].cpu()
        ref = _oracle(cfg, sds, fr)
        err32 = rel(got, ref)
        worst = max(worst, (err32, i))
        if i not in mods and not slow:     # the recorded statistics: the 1e-4 gate of the batch-32 test
            print(f"frame {i}: HIP vs fp32 oracle {err32:.2e}")
            assert err32 < TOL, f"frame {i}: {err32:.3e} vs the fp32 oracle"
            continue
        ref64 = _oracle64(cfg, sds, fr)
        hip64, orc64 = rel(got, ref64), rel(ref, ref64)
        print(f"frame {i} ({mods.get(i, 'plain')}): HIP vs fp32 oracle {err32:.2e} | HIP vs fp64 {hip64:.2e} | fp32 oracle vs fp64 {orc64:.2e}")
        assert hip64 <= 2.0 * orc64 + 5e-7, f"frame {i}: HIP {hip64:.3e} from the exact result, the fp32 oracle {orc64:.3e}"
        if orc64 < 4e-5:
            assert err32 < TOL, f"frame {i}: {err32:.3e} vs the fp32 oracle"
    print(f"batch 32: worst frame {worst[1]} at {worst[0]:.3e} vs the fp32 oracle")


def test_forward_latency_mode_batch8_every_frame(dev):
    """set_latency_mode(True, frames=4), batch 8, the 2 x 4 graph: every frame alone and the permuted batches (eager and through the
    graph captured in the original order) give the batch's bits."""
    cfg = kb.kitti_config()
    sds = kb.synthetic.make_state_dicts(cfg, seed=0, gain=kb.synthetic.PARITY_GAIN["kitti"])
    image, sparse, valid, k = [f.clone() for f in kb.synthetic.make_frames(8, 352, 1216, "kitti", seed=1, jitter_intrinsics=0.1)]
    image[3] *= 255.0
    sparse[4] = 0.0
    valid[4] = 0.0
    m = kb.modules.KBNetModel.from_config(cfg, dev)
    m.load_state_dicts(*sds)
    m.set_latency_mode(True, frames=4)
    dframes = _to(dev, (image, sparse, valid, k))
    out = m.forward(*dframes).clone()
    assert torch.isfinite(out).all()
    replay = m.capture(*dframes)
    assert replay.branches == 2 and torch.equal(replay(*dframes), out)
    for i in range(8):
        assert torch.equal(m.forward(*[f[i:i + 1] for f in dframes]), out[i:i + 1]), f"frame {i} alone"
    for p in (list(range(7, -1, -1)), [4, 5, 6, 7, 0, 1, 2, 3], torch.randperm(8, generator=torch.Generator().manual_seed(3)).tolist()):
        pd = torch.tensor(p, device=dev)
        pf = [f[pd] for f in dframes]
        assert torch.equal(m.forward(*pf), out[pd]), f"eager, permutation {p}"
        assert torch.equal(replay(*pf), out[pd]), f"graph, permutation {p}"
    m.set_latency_mode(False)


# -------------------------------------------------------------------------- non-finite pixels, op level
BAD = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}


def check_bad_frame(name, got, r64, r32, clean, bad, max_bar=2e-5):
    """Frame `bad` carries one non-finite input value.  Its output is non-finite exactly where the fp64 evaluation's is (the value's
    receptive field: one non-finite term per output there, nonzero weights), and everywhere else it meets the op's fp64 bar -- the
    frame's windows follow its finite data; the other frames keep the bits of the clean batch."""
    got = got.detach().cpu()
    for i in range(got.shape[0]):
        if i != bad:
            assert torch.equal(got[i], clean[i].cpu()), f"{name}: frame {i} beside the bad frame keeps its bits"
    rf = ~torch.isfinite(r64[bad])
    assert bool(rf.any()), "the bad value reaches the output"
    hit = ~torch.isfinite(got[bad])
    assert not bool((rf & ~hit).any()), f"{name}: non-finite wherever the fp64 evaluation is"
    # the kernels may also spread it to a zero tap of the same pixel (0 x Inf; the folded / fused forms): within 2 pixels of the field
    near = torch.nn.functional.max_pool2d(rf[None].double(), 5, stride=1, padding=2)[0] > 0
    assert not bool((hit & ~near).any()), f"{name}: non-finite only next to the receptive field"
    fin = ~hit
    ref = torch.where(fin, r64[bad], torch.zeros_like(r64[bad]))
    rms = (ref.pow(2).sum(dim=(1, 2), keepdim=True) / fin.sum(dim=(1, 2), keepdim=True).clamp_min(1)).sqrt().clamp_min(1e-300)
    e = torch.where(fin, (got[bad].double() - ref) / rms, torch.zeros_like(ref)).abs()
    eo = torch.where(fin, (r32[bad].double() - ref) / rms, torch.zeros_like(ref)).abs()
    cnt = float(fin.sum())
    rh, ro, mh = float((e.pow(2).sum() / cnt).sqrt()), float((eo.pow(2).sum() / cnt).sqrt()), float(e.max())
    assert rh < max(3.5 * ro, 6e-7) and rh < 1.5e-6 and mh < max_bar, f"{name}: bad frame outside the receptive field: rms {rh:.2e} (fp32 {ro:.2e}) max {mh:.2e}"


@pytest.mark.parametrize("bad", list(BAD))
@pytest.mark.parametrize("form", ["plain_tail_tiles", "stride2", "up_64_tp64_tail", "up_narrow16", "transposed"])
def test_conv3x3_split_non_finite_pixel(dev, form, bad):
    """One NaN / +Inf / -Inf in one channel of the middle frame of five (beside frames of other magnitudes): the frame's slot holds
    its FINITE maximum, its window follows it, the rest of the frame is right."""
    n = 5
    cins, cout, h, w, kind, sliced, xs, wt, frames = _conv_case(form, n, 0)
    xs = [x.clone() for x in xs]
    xs[0][2] = lrelu(torch.randn(cins[0], *xs[0].shape[2:], generator=torch.Generator().manual_seed(9)), 0.2) * 3.0
    for x in xs[1:]:
        x[2] = xs[0][2, :x.shape[1]]
    up = kind in ("up", "tr")
    stride = 2 if kind == "s2" else 1
    packed = kb.ops.pack_conv3x3_split_weight(wt.to(dev), stride=stride, folded_up2x=up, transposed=kind == "tr")

    def run(xl):
        stats = kb.ops.ActStats(n, dev)
        xd = [x.to(dev) for x in xl]
        slots = [stats.measure(x) for x in xd]
        out = torch.full((n, cout, h, w), float("nan"), device=dev)
        slot = stats.new()
        assert kb.ops.conv3x3_split([kb.ops.tensor_src(x, "x", sl) for x, sl in zip(xd, slots)], packed, n, cout, h, w, out, up2x=up,
                                    negative_slope=0.2, stride=stride, folded_up2x=up, transposed=kind == "tr", out_absmax=slot) is not None
        return out, [slot_of(sl) for sl in slots], slot_of(slot)

    clean, clean_slots, _ = run(xs)
    dirty = [x.clone() for x in xs]
    sh, sw = dirty[0].shape[2:]
    dirty[0][2, 3, sh // 2, sw // 3] = BAD[bad]
    out, slots, oslot = run(dirty)
    d0 = dirty[0].to(dev)
    assert torch.equal(slots[0], torch.where(torch.isfinite(d0), d0, torch.zeros_like(d0)).abs().amax(dim=(1, 2, 3))), \
        "the slot of a frame with a non-finite value holds its finite maximum"
    assert torch.equal(oslot.cpu(), torch.where(torch.isfinite(out), out, torch.zeros_like(out)).abs().amax(dim=(1, 2, 3)).cpu())
    xcat = torch.cat(dirty, 1)
    check_bad_frame(form, out, _conv_ref(xcat, wt, kind, torch.float64), _conv_ref(xcat, wt, kind, torch.float32), clean, 2)


@pytest.mark.parametrize("bad", list(BAD))
def test_conv1x1s2_and_front_non_finite_pixel(dev, bad):
    """The same for conv1x1s2_split (a bad image value at an even pixel: receptive field one output pixel), kb1_front (per-tile
    windows of conv0, the bound behind conv_image's window) and conv_tail (per-tile windows), middle frame of five."""
    n, g = 5, torch.Generator().manual_seed(4)
    # conv1x1s2_split, image + fused, no xyz
    ci, cf, cout, h, w = 48, 48, 96, 35, 70
    oh, ow = (h + 1) // 2, (w + 1) // 2
    image = lrelu(torch.randn(n, ci, h, w, generator=g), 0.2)
    fused = lrelu(torch.randn(n, cf, h, w, generator=g), 0.2)
    wt = torch.randn(cout, ci + cf, 1, 1, generator=g) / (ci + cf) ** 0.5
    packed = kb.ops.pack_conv1x1s2_split_weight(wt.to(dev))

    def run1(im):
        stats = kb.ops.ActStats(n, dev)
        imd, fd = im.to(dev), fused.to(dev)
        out = torch.empty(n, cout, oh, ow, device=dev)
        assert kb.ops.conv1x1s2_split([kb.ops.tensor_src(imd, "image", stats.measure(imd)), kb.ops.tensor_src(fd, "fused", stats.measure(fd))],
                                      packed, None, n, cout, oh, ow, out, negative_slope=0.2) is not None
        return out

    clean = run1(image)
    dirty = image.clone()
    dirty[2, 5, 20, 30] = BAD[bad]
    cat = torch.cat([dirty, fused], 1)
    check_bad_frame("conv1x1s2_split", run1(dirty), lrelu(torch.nn.functional.conv2d(cat.double(), wt.double(), stride=2), 0.2),
                    orc.conv2d(cat, wt, 2, 0.2), clean, 2)
    # kb1_front
    h, w, c, f0, fi = 35, 70, 3, 48, 48
    oh, ow = (h + 1) // 2, (w + 1) // 2
    img = torch.rand(n, c, h, w, generator=g)
    xyz = torch.randn(n, 3, oh, ow, generator=g)
    w0 = torch.randn(f0, c, 3, 3, generator=g) / (c * 9) ** 0.5
    wi = torch.randn(fi, f0, 3, 3, generator=g) / (f0 * 9) ** 0.5
    wf = torch.randn(fi, f0 + 3, 1, 1, generator=g) / (f0 + 3) ** 0.5
    pf = kb.ops.pack_kb1_front_weight(w0.to(dev), wi.to(dev), wf.to(dev))

    def run2(im):
        oi, of = torch.empty(n, fi, oh, ow, device=dev), torch.empty(n, fi, oh, ow, device=dev)
        assert kb.ops.kb1_front(im.to(dev), pf, xyz.to(dev), f0, fi, oi, of, 0.2, 0.2) is not None
        return oi, of

    ci_, cf_ = run2(img)
    dimg = img.clone()
    dimg[2, 1, 17, 40] = BAD[bad]

    def chain(dt, conv):
        x0 = conv(dimg.to(dt), w0.to(dt), 1)
        up = torch.zeros(n, 3, h, w, dtype=dt)
        up[:, :, ::2, ::2] = xyz.to(dt)
        return conv(x0, wi.to(dt), 2), conv(torch.cat([x0, up], 1), wf.to(dt), 2)

    r64 = chain(torch.float64, lambda x, wt_, s: lrelu(torch.nn.functional.conv2d(x, wt_, stride=s, padding=wt_.shape[-1] // 2), 0.2))
    r32 = chain(torch.float32, lambda x, wt_, s: orc.conv2d(x, wt_, s, 0.2))
    for name, got, a, b, cl in zip(("conv_image", "conv_fused"), run2(dimg), r64, r32, (ci_, cf_)):
        check_bad_frame(f"kb1_front {name}", got, a, b, cl, 2)
    # conv_tail: logits
    c, h, w = 12, 37, 72
    x = torch.randn(n, c, h, w, generator=g)
    wc = torch.randn(c, c, 3, 3, generator=g) * (1.3 / (c * 9) ** 0.5)
    wo = torch.randn(1, c, 3, 3, generator=g) * 0.5
    pt = kb.ops.pack_conv_tail_weight(wc.to(dev))
    run3 = lambda t: kb.ops.conv_tail(t.to(dev), pt, wo.to(dev), 1.5, 100.0, 0.2, return_logits=True)[1]
    clean = run3(x)
    dx = x.clone()
    dx[2, 4, 18, 40] = BAD[bad]
    l64 = torch.nn.functional.conv2d(lrelu(torch.nn.functional.conv2d(dx.double(), wc.double(), padding=1), 0.2), wo.double(), padding=1)
    l32 = orc.conv2d(orc.conv2d(dx, wc, 1, 0.2), wo, 1, None)
    check_bad_frame("conv_tail logits", run3(dx), l64, l32, clean, 2, max_bar=1e-4)


# -------------------------------------------------------------------------- a finite outlier 2^20 x the frame's bulk
def test_forward_full_size_outlier_2e20(dev):
    """The boundary of one window per frame: frame 0 carries a dozen image pixels 2^20 x the rest (frame 1: the same frame without
    them).  Farther than 48 px from an outlier the HIP result is at most 2x as far from an fp64 evaluation as the fp32 oracle is
    anywhere in the frame (the bar of test_forward_full_size_intra_frame_dynamic_range, whose outliers are 1e4), and frame 1 keeps
    the strict bars; INTEGRATION.md states the range."""
    cfg = kb.kitti_config()
    sds = kb.synthetic.make_state_dicts(cfg, seed=2, gain=kb.synthetic.PARITY_GAIN["kitti"])
    image, sparse, valid, k = [f.clone() for f in kb.synthetic.make_frames(2, 352, 1216, "kitti", seed=5, jitter_intrinsics=0.1)]
    g = torch.Generator().manual_seed(17)
    ys, xs = torch.randint(0, 352, (12,), generator=g), torch.randint(0, 1216, (12,), generator=g)
    image[1], sparse[1], valid[1], k[1] = image[0], sparse[0], valid[0], k[0]
    image[0, :, ys, xs] = image[0, :, ys, xs] * 2.0 ** 20 + 2.0 ** 20
    frames = (image, sparse, valid, k)
    m = kb.modules.KBNetModel.from_config(cfg, dev)
    m.load_state_dicts(*sds)
    out = m.forward(*_to(dev, frames)).cpu()
    assert torch.isfinite(out).all()
    yy, xx = torch.meshgrid(torch.arange(352), torch.arange(1216), indexing="ij")
    far = ((yy[None] - ys.view(-1, 1, 1)) ** 2 + (xx[None] - xs.view(-1, 1, 1)) ** 2).amin(0) > 48 ** 2
    for i in (0, 1):
        fr = [f[i:i + 1] for f in frames]
        ref, ref64 = _oracle(cfg, sds, fr), _oracle64(cfg, sds, fr)
        e_hip = ((out[i:i + 1].double() - ref64).abs() / ref64.abs())[0, 0]
        orc64 = float(((ref.double() - ref64).abs() / ref64.abs()).max())
        err32 = float(((out[i:i + 1] - ref).abs() / ref.abs()).max())
        print(f"outlier 2^20, frame {i}: far from the outliers {float(e_hip[far].max()):.2e}, everywhere {float(e_hip.max()):.2e}; "
              f"fp32 oracle vs fp64 {orc64:.2e}; vs the fp32 oracle {err32:.2e}")
        if i == 0:
            assert float(e_hip[far].max()) <= 2.0 * orc64, "away from the outliers the frame's windows hold"
        else:
            assert float(e_hip.max()) <= 2.0 * orc64 + 5e-7 and (orc64 >= 4e-5 or err32 < TOL)
