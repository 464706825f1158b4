"""CPU: what tests/test_grad_extents_gpu.py stands on.

The cases reach what they claim: the split count of every weight-gradient case, read from the library's own plan (host code), is
the number written beside the case in tests/grad_extent_cases.py -- a change of the plan's constants fails here instead of taking
the cases out of the regimes they exist for.

The reference alone stays inside the gate: torch's own fp32 autograd on the CPU against the fp64 result, per operator case, under a
third of the 2e-4 operator gate (6.7e-5).  Measured (of |b| + rms(b)): weight gradients at most 9.8e-6 with one input (k7s2_f24) and
1.3e-5 with two (k5s2_two_inputs), data gradients at most 2.5e-6 (k7s2_f40_c19), the recorded conv 1.3e-5 (weight) and 1.5e-6 (data),
BatchNorm 8.9e-6 (grad_gamma, batch statistics, slope 0.2); a plain sequential fp32 sum of all 71 806 terms of an element 3.9e-6.

Proof of power: a plain stand-in of the split sum (chunks of 32 pixels, `cps` chunks per split, planes added in split order, fp64)
passes the gate when right and leaves it by more than 10 x with each of six mistakes of a split plan or a frame index planted."""
import numpy as np
import pytest
import torch

import kbnet_amd as kb

import grad_extent_cases as ext
import posenet_grad_oracle as pgo

THIRD = pgo.TOL / 3.0
POWER = 10.0 * pgo.TOL


# ---- the cases reach what they claim ---------------------------------------------------------------------------------------
def _splits(c, asked):
    lib = kb._lib.load()
    h, w = c["size"]
    cin, k, oc = sum(c["cins"]), c["k"], c["oc"]
    if (k, c["stride"]) in ext.S2_ENTRY:
        nbytes = lib.kbn_conv2d_s2_backward_weight_scratch_bytes(ext.N, oc, cin, k, h, w, asked)
    else:
        nbytes = lib.kbn_conv2d_backward_weight_scratch_bytes(ext.N, oc, cin, k, c["stride"], h, w, asked)
    planes, rest = divmod(nbytes, 4 * oc * cin * k * k)
    assert rest == 0
    return max(planes, 1)      # no scratch: one split


@pytest.mark.parametrize("name", [c["name"] for c in ext.WGRAD])
def test_split_counts_are_the_ones_written_beside_the_case(name):
    c = ext.by_name(name)
    got = {asked: _splits(c, 0 if asked is None else asked) for asked in ext.SPLITS}
    assert got == {None: c["auto"], 1: 1, 7: 7, 1 << 20: c["most"]}, got


def test_the_two_anchors_of_the_plans_rule():
    """(3, 1), 3 -> 8 channels, one tile: 512 splits aimed for (2244 // 4 = 561 chunks allow them: the cap, not the chunk count,
    decides) -> 5 chunks each -> ceil(2244 / 5) = 449.  1 << 20 asked -> 1024 -> 3 chunks each -> ceil(2244 / 3) = 748."""
    c = ext.by_name("k3s1_f8")
    assert ext.CHUNKS // 4 >= 512 and ext.CHUNKS > 1024
    assert _splits(c, 0) == 449 == -(-ext.CHUNKS // -(-ext.CHUNKS // 512))
    assert _splits(c, 1 << 20) == 748 == -(-ext.CHUNKS // -(-ext.CHUNKS // 1024))
    assert _splits(c, 512) == 449 and _splits(c, 1024) == 748 and _splits(c, 1025) == 748      # asked and given differ only here


def test_the_cases_cover_what_the_extent_is_for():
    pairs = {(c["k"], c["stride"]) for c in ext.WGRAD}
    assert pairs == {(3, 1), (1, 1), (1, 2), (3, 2), (5, 2), (7, 2)} == {(c["k"], c["stride"]) for c in ext.DGRAD}
    for pair in pairs:
        assert {c["oc"] for c in ext.WGRAD if (c["k"], c["stride"]) == pair and c["cins"] == (3,) and not c["sliced"]} == {8, 24, 40}
        assert {(c["oc"], c["cins"]) for c in ext.DGRAD if (c["k"], c["stride"]) == pair} == {(8, (3,)), (40, (19,))}
    for entry in (True, False):
        mine = [c for c in ext.WGRAD if ((c["k"], c["stride"]) in ext.S2_ENTRY) == entry]
        assert sum(c["cins"] == (3, 5) for c in mine) == 1 and sum(c["sliced"] for c in mine) == 1
    for cases in (ext.WGRAD, ext.DGRAD):     # both parities of the stride-2 input
        assert {c["size"] for c in cases if c["stride"] == 2} == {ext.ODD, ext.EVEN}
    assert len({c["name"] for c in ext.WGRAD + ext.DGRAD + [ext.NODE]}) == len(ext.WGRAD) + len(ext.DGRAD) + 1
    for c in ext.WGRAD + ext.DGRAD + [ext.NODE]:
        xs, weight, grad_out = ext.conv_inputs(c)
        assert grad_out.shape[0] * grad_out.shape[2] * grad_out.shape[3] == ext.M == 71806
        for t in (*xs, weight, grad_out):
            assert torch.equal(t, t.float().double())


# ---- the reference alone stays inside the gate ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in ext.WGRAD if not c["sliced"]])
def test_torchs_fp32_weight_gradient_is_under_a_third_of_the_gate(name):
    c = ext.by_name(name)
    f = pgo.fraction(ext.conv_gradients(c, dtype=torch.float32)[0], ext.weight_gradient(name))
    print(f"{name}: torch's fp32 weight gradient at {f:.2e} of |b| + rms(b)")
    assert f <= THIRD
    assert abs(pgo.po.rms(ext.weight_gradient(name)) / ext.M ** 0.5 - 1.0) < 0.2      # a term of size 1 is 1 / rms = 4e-3: 20 x the gate


@pytest.mark.parametrize("name", [c["name"] for c in ext.DGRAD])
def test_torchs_fp32_data_gradient_is_under_a_third_of_the_gate(name):
    c = ext.by_name(name)
    f = pgo.fraction(ext.conv_gradients(c, dtype=torch.float32, weight_grad=False, data_grad=True)[1][0], ext.data_gradient(name))
    print(f"{name}: torch's fp32 data gradient at {f:.2e} of |b| + rms(b)")
    assert f <= THIRD


def test_torchs_fp32_recorded_conv_is_under_a_third_of_the_gate():
    gw, gxs, u = ext.conv_gradients(ext.NODE, data_grad=True)
    mask = u > 0
    gw32, gxs32, _ = ext.conv_gradients(ext.NODE, dtype=torch.float32, data_grad=True, mask=mask)
    for label, a, b in [("weight", gw32, gw)] + [(f"input {i}", a, b) for i, (a, b) in enumerate(zip(gxs32, gxs))]:
        f = pgo.fraction(a, b)
        print(f"recorded conv, {label}: torch's fp32 at {f:.2e} of |b| + rms(b)")
        assert f <= THIRD


@pytest.mark.parametrize("batch", [False, True], ids=["running", "batch"])
@pytest.mark.parametrize("slope", [None, 0.2])
def test_torchs_fp32_batch_norm_is_under_a_third_of_the_gate(slope, batch):
    c = ext.bn_inputs(batch)
    want = ext.bn_gradients(c, slope, batch)
    got = ext.bn_gradients(c, slope, batch, dtype=torch.float32, mask=None if slope is None else want["z"] > 0)
    for k in ("grad_u", "grad_gamma", "grad_beta"):
        f = pgo.fraction(got[k], want[k])
        print(f"batch norm slope {slope} batch {batch} {k}: torch's fp32 at {f:.2e} of |b| + rms(b)")
        assert f <= THIRD


@pytest.mark.parametrize("batch", [False, True], ids=["running", "batch"])
def test_no_batch_norm_pre_activation_is_closer_to_zero_than_fp32_resolves(batch):
    """The seed's rule: it is the first from 1 on at which every |z| exceeds its band (grad_extent_cases.bn_kink_margin)."""
    for seed in range(1, ext.BN_SEED[batch] + 1):
        margin = ext.bn_kink_margin(ext.bn_inputs(batch, seed), batch)
        print(f"batch {batch} seed {seed}: the closest |z| is {margin:.2f} bands from 0")
        assert (margin > 1.0) == (seed == ext.BN_SEED[batch]), (seed, margin)
    c = ext.bn_inputs(batch)
    ratio = c["u"].mean(dim=(0, 2, 3)) / c["u"].std(dim=(0, 2, 3))
    # means 4 to 64 spreads from 0; a sample spread is good to 1 / sqrt(2 x 71 806) = 0.26 %: four times that
    assert float((ratio / torch.tensor(ext.BN_RATIO, dtype=torch.float64) - 1.0).abs().max()) < 0.0106


def test_a_sequential_fp32_sum_of_all_the_terms_is_under_a_third_of_the_gate():
    """Three elements of the 8-filter (3, 1) weight gradient as the plainest kernel would sum them: 71 806 products, each rounded to
    fp32, added one by one in pixel order.  No split plan the kernel may take is a longer chain of fp32 additions than this one."""
    c = ext.by_name("k3s1_f8")
    a, b = ext.gemm_operands(c)
    want = ext.weight_gradient(c["name"]).reshape(c["oc"], -1)
    scale = pgo.po.rms(want)
    worst = 0.0
    for oc, col in ((0, 0), (3, 13), (7, 26)):      # a corner tap, the centre tap, the last column
        terms = (a[:, oc].numpy().astype(np.float32) * b[:, col].numpy().astype(np.float32))
        total = float(np.cumsum(terms, dtype=np.float32)[-1])
        worst = max(worst, abs(total - float(want[oc, col])) / (abs(float(want[oc, col])) + scale))
    print(f"sequential fp32 sum over {ext.M} terms: {worst:.2e} of |b| + rms(b)")
    assert worst <= THIRD


# ---- proof of power -------------------------------------------------------------------------------------------------------
CASE = ext.by_name("k3s1_f8")
EXTRA = 3       # channels on either side of the slice the stand-in reads: what lies around a channel slice


@pytest.fixture(scope="module")
def operands():
    """The case as the kernel sees it: A and B rows by flat pixel index over THREE frames' worth of memory -- the case's two, and
    behind them what a read past the end finds (a frame of values of order one) -- and the same two frames again as a channel slice
    of a wider tensor, flattened with the DENSE batch stride (what a kernel that ignores the slice's own stride reads as frame 1)."""
    a, b = ext.gemm_operands(CASE)
    g = torch.Generator().manual_seed(5)
    per = ext.OH * ext.OW
    behind = (torch.randn(per, a.shape[1], generator=g, dtype=torch.float64), torch.randn(per, b.shape[1], generator=g, dtype=torch.float64))
    xs, _, grad_out = ext.conv_inputs(CASE)
    dense = []
    for t, extra in ((grad_out, EXTRA), (xs[0], EXTRA)):
        n, ch, h, w = t.shape
        whole = torch.randn(n, ch + 2 * extra, h, w, generator=g, dtype=torch.float64)
        whole[:, extra:extra + ch] = t
        view = whole[:, extra:extra + ch]
        dense.append(view.as_strided(view.shape, (ch * h * w,) + tuple(view.stride()[1:]), view.storage_offset()))
    a2 = dense[0].permute(0, 2, 3, 1).reshape(ext.M, -1)
    b2 = torch.nn.functional.unfold(dense[1], 3, padding=1).permute(0, 2, 1).reshape(ext.M, -1)
    assert torch.equal(a2[:per], a[:per]) and torch.equal(b2[:per], b[:per]) and not torch.equal(a2[per:], a[per:])
    return dict(a=torch.cat([a, behind[0]]), b=torch.cat([b, behind[1]]), a_dense=a2, b_dense=b2)


def split_sum(ops, cps, mistake=None):
    """The weight gradient of the stand-in: split z adds chunks [z cps, (z + 1) cps) of 32 pixels into plane z, the planes are
    added in split order.  fp64: what is left of a mistake is the mistake."""
    m_total, chunks = ext.M, ext.CHUNKS
    a, b = ops["a"], ops["b"]
    if mistake == "second frame at the first frame's batch stride":
        a, b = ops["a_dense"], ops["b_dense"]
    splits = -(-chunks // cps)
    span = cps + 1 if mistake == "splits overlap by one chunk" else cps
    planes = []
    for z in range(splits):
        lo, hi = z * cps * ext.CHUNK, min(chunks, z * cps + span) * ext.CHUNK
        m = torch.arange(lo, hi)
        if mistake != "pixels past M read":
            m = m[m < m_total]                                     # zero by predicate
        if mistake == "16-bit wrap of m in the frame index":
            m = m & 0xFFFF                                         # fn = m / OHW and rem = m - fn OHW, both from the wrapped m
        planes.append(a[m].T @ b[m])
    if mistake == "last split dropped":
        planes = planes[:-1]
    if mistake == "first 1024 planes reduced":
        planes = planes[:1024]
    out = planes[0].clone()
    for p in planes[1:]:
        out += p
    return out.reshape(CASE["oc"], 3, 3, 3)


@pytest.mark.parametrize("cps", [5, 3, 1, 321, ext.CHUNKS])
def test_the_right_split_sum_passes(operands, cps):
    f = pgo.fraction(split_sum(operands, cps), ext.weight_gradient(CASE["name"]))
    print(f"the stand-in at {cps} chunks per split: {f:.2e}")
    assert f <= 1e-12


@pytest.mark.parametrize("mistake, cps", [
    ("last split dropped", 5),                                   # 449 splits: the last holds 4 chunks, 126 pixels
    ("splits overlap by one chunk", 5),                          # 448 chunks added twice
    ("pixels past M read", 5),                                   # two pixels behind the last frame
    ("16-bit wrap of m in the frame index", 5),                  # the 6270 pixels from 65 536 on read the first ones again
    ("second frame at the first frame's batch stride", 5),       # frame 1 = the channels behind frame 0's slice
    ("first 1024 planes reduced", 1),                            # a plan of 2244 one-chunk splits, a reduction that knows 1024
])
def test_a_planted_mistake_leaves_the_gate_by_ten_times(operands, mistake, cps):
    f = pgo.fraction(split_sum(operands, cps, mistake), ext.weight_gradient(CASE["name"]))
    print(f"{mistake}: {f:.2e} of |b| + rms(b) (gate {pgo.TOL:.0e})")
    assert f >= POWER, (mistake, f)
