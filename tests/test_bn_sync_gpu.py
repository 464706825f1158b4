"""GPU, one process: the operators of csrc/bn_sync.hip and ops.batch_norm_act_sync.  The ranks are simulated by STACKING: the
operators take the gathered buffers as arguments, so the shards' records and sums are computed one after the other and stacked
in rank order -- the whole algebra without a collective (tests/test_bn_sync_ranks_gpu.py runs it through real ones).

Gates: the ones the existing operators are held to (tests/test_posenet_backward_gpu.py): relative 1e-7 / 1e-6 for the mean / the
variance under cancellation, posenet_grad_oracle.TOL for the gradients, the forward's 1e-4 rule for y; all against fp64.

    python -m pytest tests/test_bn_sync_gpu.py -m gpu -q -s
"""
import pytest
import torch

import kbnet_amd as kb
KbnError = kb._lib.KbnError

import bn_sync_oracle as bso
import posenet_grad_cases as cases
import posenet_grad_oracle as pgo
import posenet_oracle as po
import test_posenet_train_gpu as model_test

pytestmark = pytest.mark.gpu
ops = kb.ops
SENTINEL = -7.25e30


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need a visible MI355X (run with -m gpu on a GPU box)")
    kb._lib.load()   # a missing extension is an error on a GPU box, never a skip
    return torch.device("cuda:0")


def ulps(a, b):
    """The largest distance between two fp32 tensors in units in the last place."""
    def ordered(t):
        i = t.detach().contiguous().view(torch.int32).long()
        return torch.where(i < 0, -(i & 0x7fffffff), i)
    assert a.shape == b.shape and a.dtype == b.dtype == torch.float32
    return int((ordered(a) - ordered(b)).abs().max())


def _close(label, got, want):
    f = pgo.fraction(got, want)
    print(f"{label}: {f:.2e} of |b| + rms(b) (gate {pgo.TOL:.0e})")
    assert f <= pgo.TOL, (label, f)


def _slice_of_sentinels(t, dev, extra=2):
    """`t` (fp32, any device) as a channel slice of a larger sentinel-filled device tensor: strided frames."""
    n, c, h, w = t.shape
    whole = torch.full((n, c + 2 * extra, h, w), SENTINEL, device=dev)
    whole[:, extra:extra + c] = t.to(dev)
    return whole[:, extra:extra + c]


def _off_by_one_float(t, dev):
    """`t` as a dense view that starts 4 bytes into an allocation: not 16-byte aligned."""
    buf = torch.full((t.numel() + 1,), SENTINEL, device=dev)
    view = buf[1:].view(t.shape)
    view.copy_(t.to(dev))
    assert view.data_ptr() % 16 == 4
    return view


def _gathered_moments(shards):
    return torch.stack([ops.batch_norm_moments(s) for s in shards])


# ------------------------------------------------------------------------------------------------------------ the merge
def test_merged_moments_under_cancellation(dev):
    """test_batch_norm_stats_cancellation's tensor (mean 100, deviation 1e-2) as shards of 2 + 1 + 1 frames, dense and as a channel
    slice: the merged statistics keep batch_norm_stats's bounds, and the calls repeat their bits."""
    g = torch.Generator().manual_seed(3)
    x = (100.0 + 1e-2 * torch.randn(4, 6, 33, 35, generator=g, dtype=torch.float64)).float()
    m64 = x.double().mean(dim=(0, 2, 3))
    v64 = x.double().var(dim=(0, 2, 3), unbiased=False)
    w64 = x.double().var(dim=(0, 2, 3), unbiased=True)
    for label, view in (("dense", x.to(dev)), ("channel slice", _slice_of_sentinels(x, dev))):
        shards = bso.split(view, (2, 1, 1))
        gathered = _gathered_moments(shards)
        assert gathered.dtype == torch.float64 and tuple(gathered.shape) == (3, 13)
        assert gathered[:, 0].tolist() == [2.0 * 33 * 35, 33.0 * 35, 33.0 * 35]
        mean, var, unbiased = ops.batch_norm_moments_merge(gathered)
        em = float(((mean.double().cpu() - m64).abs() / m64).max())
        ev = float(((var.double().cpu() - v64).abs() / v64).max())
        ew = float(((unbiased.double().cpu() - w64).abs() / w64).max())
        print(f"merged moments, {label}: mean {em:.2e}, variance {ev:.2e}, unbiased variance {ew:.2e} relative")
        assert em <= 1e-7 and ev <= 1e-6 and ew <= 1e-6
        assert torch.equal(gathered, _gathered_moments(shards))
        for a, b in zip((mean, var, unbiased), ops.batch_norm_moments_merge(gathered)):
            assert torch.equal(a, b)


def test_one_shard_merge_is_batch_norm_stats(dev):
    g = torch.Generator().manual_seed(5)
    x = (0.7 * torch.randn(3, 5, 7, 9, generator=g) + 0.3).to(dev)
    mean, var, _ = ops.batch_norm_moments_merge(_gathered_moments([x]))
    want = ops.batch_norm_stats(x)
    assert ulps(mean, want[0]) <= 1 and ulps(var, want[1]) <= 1


def test_refusals(dev):
    x = torch.zeros(2, 3, 4, 5, device=dev)
    with pytest.raises(KbnError, match="empty"):
        ops.batch_norm_moments(x[:0])
    with pytest.raises(KbnError):
        ops.batch_norm_moments_merge(torch.zeros(2, 6, device=dev, dtype=torch.float64))      # no 2 C + 1
    with pytest.raises(KbnError, match="float64"):
        ops.batch_norm_moments_merge(torch.zeros(2, 7, device=dev))
    with pytest.raises(KbnError, match="empty"):
        ops.batch_norm_act_sync(x[:0], torch.ones(3, device=dev), torch.zeros(3, device=dev), kb.dist.BatchNormGroup(0, 1))
    gathered = _gathered_moments([x + 1.0])
    ones, zeros = torch.ones(3, device=dev), torch.zeros(3, device=dev)
    sums = ops.batch_norm_act_backward_sums(x, x, ones, zeros, zeros, ones).unsqueeze(0)
    with pytest.raises(KbnError, match="rank"):
        ops.batch_norm_act_backward_sync(x, x, ones, zeros, zeros, ones, sums, gathered, 1)


# ------------------------------------------------------------------------------------------------------------ the backward
VIEWS = {"dense": lambda t, dev: t.to(dev), "strided": _slice_of_sentinels, "unaligned": _off_by_one_float}


def _sharded_backward(c, d, sizes, slope, view, dev):
    """Forward and backward shard by shard through the four operators -> (y, grad_u, grad_gamma, grad_beta) of the whole batch
    after the n_r / n weights, and the merged (mean, var)."""
    us = [VIEWS[view](t, dev) for t in bso.split(d["u"], sizes)]
    gys = [VIEWS[view](t.float(), dev) for t in bso.shard_cotangents(c["grad_y"], sizes)]
    gathered = _gathered_moments(us)
    mean, var, _ = ops.batch_norm_moments_merge(gathered)
    ys = [ops.batch_norm_act(u, d["gamma"], d["beta"], mean, var, pgo.EPS, slope, True) for u in us]
    sums = torch.stack([ops.batch_norm_act_backward_sums(u, gy, d["gamma"], d["beta"], mean, var, pgo.EPS, slope) for u, gy in zip(us, gys)])
    grad_us = [ops.batch_norm_act_backward_sync(u, gy, d["gamma"], d["beta"], mean, var, sums, gathered, r, pgo.EPS, slope)
               for r, (u, gy) in enumerate(zip(us, gys))]
    k = c["u"].shape[1]
    gu, gg, gb = bso.reassemble(grad_us, [s[k:] for s in sums], [s[:k] for s in sums], sizes)
    return torch.cat(ys), gu, gg, gb, mean, var


@pytest.mark.parametrize("view", list(VIEWS))
@pytest.mark.parametrize("sizes", [(2, 1), (1, 1, 1)], ids=lambda s: "+".join(str(v) for v in s))
@pytest.mark.parametrize("slope", [None, 0.0, 0.2])
def test_sharded_backward_against_the_whole_batchs_autograd(dev, slope, sizes, view):
    c = cases.bn_case(slope, True)
    assert tuple(c["u"].shape) == (3, 5, 7, 9)
    d = {k: v.float().to(dev) for k, v in c.items()}
    y, gu, gg, gb, mean, var = _sharded_backward(c, d, sizes, slope, view, dev)
    assert po.gate_fraction(y, c["y"], po.layer_floor(c["y"])) <= 1.0
    label = f"slope {slope} shards {sizes} {view}"
    _close(f"{label} grad_u", gu, c["grad_u"])
    _close(f"{label} grad_gamma", gg, c["grad_gamma"])
    _close(f"{label} grad_beta", gb, c["grad_beta"])
    again = _sharded_backward(c, d, sizes, slope, view, dev)
    for a, b in zip((y, gu, gg, gb, mean, var), again):
        assert torch.equal(a, b), "the synchronised backward must repeat its bits"


@pytest.mark.parametrize("slope", [None, 0.2])
def test_one_shard_backward_is_batch_norm_act_backward(dev, slope):
    c = cases.bn_case(slope, True)
    d = {k: v.float().to(dev) for k, v in c.items()}
    mean, var = ops.batch_norm_stats(d["u"])
    want = ops.batch_norm_act_backward(d["u"], d["grad_y"], d["gamma"], d["beta"], mean, var, pgo.EPS, slope, True)
    sums = ops.batch_norm_act_backward_sums(d["u"], d["grad_y"], d["gamma"], d["beta"], mean, var, pgo.EPS, slope)
    got = ops.batch_norm_act_backward_sync(d["u"], d["grad_y"], d["gamma"], d["beta"], mean, var, sums.unsqueeze(0),
                                           _gathered_moments([d["u"]]), 0, pgo.EPS, slope)
    assert ulps(got, want[0]) <= 2
    assert torch.equal(sums[5:].float(), want[1]) and torch.equal(sums[:5].float(), want[2])


# ------------------------------------------------------------------------------------------------------------ through autograd
@pytest.mark.parametrize("slope", [None, 0.2])
def test_the_autograd_node_on_a_one_rank_group(dev, slope):
    """batch_norm_act_sync with a group that runs no collective against batch_norm_stats + batch_norm_act(batch=True)."""
    assert not torch.distributed.is_initialized()
    group = kb.dist.BatchNormGroup(0, 1)
    c = cases.bn_case(slope, True)
    d = {k: v.float().to(dev) for k, v in c.items()}
    mean, var = ops.batch_norm_stats(d["u"])
    ref = [d[k].clone().requires_grad_(True) for k in ("u", "gamma", "beta")]
    want = ops.batch_norm_act(ref[0], ref[1], ref[2], mean, var, pgo.EPS, slope, True)
    want.backward(d["grad_y"])
    leaves = [d[k].clone().requires_grad_(True) for k in ("u", "gamma", "beta")]
    y, m, v, unbiased = ops.batch_norm_act_sync(leaves[0], leaves[1], leaves[2], group, pgo.EPS, slope, return_stats=True)
    assert y.grad_fn is not None and not m.requires_grad and not v.requires_grad and not unbiased.requires_grad
    assert ulps(m, mean) <= 1 and ulps(v, var) <= 1
    count = c["u"].numel() // c["u"].shape[1]
    assert pgo.fraction(unbiased, c["u"].var(dim=(0, 2, 3), unbiased=True)) <= 1e-6 and count == 3 * 7 * 9
    assert po.gate_fraction(y, c["y"], po.layer_floor(c["y"])) <= 1.0
    y.backward(d["grad_y"])
    for name, leaf, r in zip(("grad_u", "grad_gamma", "grad_beta"), leaves, ref):
        _close(f"batch_norm_act_sync slope {slope} {name}", leaf.grad, c[name])
        assert pgo.fraction(leaf.grad, r.grad) <= 1e-6, name      # the two paths agree far inside the gate
    with torch.no_grad():
        quiet = ops.batch_norm_act_sync(leaves[0], leaves[1], leaves[2], group, pgo.EPS, slope)
    assert quiet.grad_fn is None and torch.equal(quiet, y)


def _launch_names(m, image0, image1):
    ops.PROFILE = []
    try:
        m.forward(image0, image1)
        return [record[0] for record in ops.PROFILE]
    finally:
        ops.PROFILE = None


def test_a_model_in_sync_mode_passes_its_batch_mode_gate(dev):
    """PoseNetModel on narrow_n3_batch with sync_batch_norm(one-rank group): the existing model test's comparison with the fp64
    oracle, its running statistics included.  Without the call the model launches what it launched before."""
    c = cases.MODEL["narrow_n3_batch"]
    image0, image1, enc, dec, cot = cases.inputs(c)
    m = model_test._model(dev, c, enc, dec, "batch")
    d0, d1 = image0.to(dev), image1.to(dev)
    with torch.no_grad():
        off = _launch_names(m, d0, d1)
        assert m.sync_batch_norm(kb.dist.BatchNormGroup(0, 1)) is m
        on = _launch_names(m, d0, d1)
    assert off.count("bn_stats") == 7 and not any(name.startswith("bn_moments") for name in off)
    assert on.count("bn_moments") == 7 and on.count("bn_moments_merge") == 7 and "bn_stats" not in on and len(on) == len(off) + 7
    m = model_test._model(dev, c, enc, dec, "batch").sync_batch_norm(kb.dist.BatchNormGroup(0, 1))
    pose, dof, layers = m.forward(d0, d1, return_all=True)
    (pose * cot.float().to(dev)).sum().backward()
    got = model_test._grads(m, dof)
    masks = [(t > 0).cpu() for t in layers]
    want = pgo.gradients(image0, image1, enc, dec, cot, batch_norm="batch", masks=masks)
    print(f"sync mode, one rank: {pgo.kink_check(masks, want['pre'])} activations on the other side of the kink than in fp64")
    model_test._compare("narrow_n3_batch in sync mode", got, want)
    model_test._running("narrow_n3_batch in sync mode", m, want, enc, "batch")
    m.set_batch_norm("running")
    with torch.no_grad():
        assert not any(name.startswith("bn_moments") for name in _launch_names(m, d0, d1))      # no effect outside 'batch' mode
