"""CPU: the algebra of synchronised BatchNorm (tests/bn_sync_oracle.py) against fp64 autograd of the whole batch, proof that the
gates of the GPU tests see what the feature is for and what it could get wrong, and the host-side pieces.

1. The oracle's shard-wise forward and backward, reassembled with GradientAverager's n_r / n weights, equal fp64 autograd of
   the whole batch to 1e-12 of |b| + rms(b).
2. Power: per-shard statistics -- data-parallel training WITHOUT the feature -- miss the pose network's gate by more than 10 x on
   every trainable parameter, and three planted mistakes each miss it by more than 10 x on a named tensor.
3. kb.dist.every_rank_has_frames against shard_bounds; the header, the binding and the build list carry the new names.

    python -m pytest tests/test_bn_sync_cpu.py -q -s
"""
import os
import re

import pytest
import torch

import kbnet_amd as kb

import bn_sync_oracle as bso
import posenet_grad_cases as cases
import posenet_grad_oracle as pgo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = 1e-12
SPLITS = [(3, 1, 1), (2, 1), (1, 1)]
ENTRY_POINTS = ("kbn_bn_moments_forward", "kbn_bn_moments_merge", "kbn_bn_act_backward_sums", "kbn_bn_act_backward_sync_apply")


def _sharded(c, sizes, slope, **mistakes):
    us = bso.split(c["u"], sizes)
    gys = bso.shard_cotangents(c["grad_y"], sizes)
    return bso.reassemble(*bso.backward(us, gys, c["gamma"], c["beta"], pgo.EPS, slope, **mistakes), sizes)


@pytest.mark.parametrize("sizes", SPLITS, ids=lambda s: "+".join(str(v) for v in s))
@pytest.mark.parametrize("slope", [None, 0.0, 0.2])
def test_the_sharded_algebra_is_the_whole_batchs_autograd(slope, sizes):
    c = cases.bn_case(slope, True, n=sum(sizes))
    us = bso.split(c["u"], sizes)
    ys, M, mean, var, unbiased = bso.forward(us, c["gamma"], c["beta"], pgo.EPS, slope)
    n, _, h, w = c["u"].shape
    assert M == n * h * w
    figures = {"y": pgo.fraction(torch.cat(ys), c["y"]),
               "mean": pgo.fraction(mean, c["u"].mean(dim=(0, 2, 3))),
               "var": pgo.fraction(var, c["u"].var(dim=(0, 2, 3), unbiased=False)),
               "unbiased var": pgo.fraction(unbiased, c["u"].var(dim=(0, 2, 3), unbiased=True))}
    for name, got in zip(("grad_u", "grad_gamma", "grad_beta"), _sharded(c, sizes, slope)):
        figures[name] = pgo.fraction(got, c[name])
    print(f"slope {slope} shards {sizes}: " + ", ".join(f"{k} {v:.1e}" for k, v in figures.items()))
    for k, v in figures.items():
        assert v <= EXACT, (k, v)


@pytest.mark.parametrize("name,sizes", [("narrow_n3_batch", (2, 1)), ("posenet_grad_train", (1, 1))])
def test_per_shard_statistics_miss_the_networks_gate_on_every_parameter(name, sizes):
    """What the ranks compute WITHOUT synchronised BatchNorm: each shard differentiated on its own statistics, the gradients
    summed (the loss is a sum over frames).  Every trainable parameter is far outside the gate the two-rank GPU test applies."""
    c = cases.MODEL[name]
    image0, image1, enc, dec, cot = cases.inputs(c)
    whole = pgo.gradients(image0, image1, enc, dec, cot, batch_norm="batch")
    keys = [k for k in whole if k.startswith(("enc::", "dec::"))]
    assert len(keys) == 22
    summed, lo = None, 0
    for s in sizes:
        part = pgo.gradients(image0[lo:lo + s], image1[lo:lo + s], enc, dec, cot[lo:lo + s], batch_norm="batch")
        summed = {k: part[k] if summed is None else summed[k] + part[k] for k in keys}
        lo += s
    figures = {k: pgo.fraction(summed[k], whole[k]) for k in keys}
    low, high = min(figures, key=figures.get), max(figures, key=figures.get)
    print(f"{name} as {sizes}: per-shard statistics leave {figures[low]:.2f} ({low}) to {figures[high]:.2f} ({high}) of |b| + rms(b); "
          f"gate {pgo.TOL:.0e}")
    for k, v in figures.items():
        assert v > 10 * pgo.TOL, (k, v)


@pytest.mark.parametrize("sizes", [(3, 1, 1), (2, 1)], ids=lambda s: "+".join(str(v) for v in s))
@pytest.mark.parametrize("mistake", ["global_divisor", "unweighted"])
def test_planted_backward_mistakes_leave_the_gate(mistake, sizes):
    """On ragged shards: M in place of the rank's own count under the two sums, and S = sum s_r without the c_r / M weights.  Both
    show in grad_u."""
    c = cases.bn_case(0.2, True, n=sum(sizes))
    assert pgo.fraction(_sharded(c, sizes, 0.2)[0], c["grad_u"]) <= EXACT
    f = pgo.fraction(_sharded(c, sizes, 0.2, **{mistake: True})[0], c["grad_u"])
    print(f"{mistake} on shards {sizes}: grad_u at {f:.2e} of |b| + rms(b) (gate {pgo.TOL:.0e})")
    assert f > 10 * pgo.TOL


def test_planted_biased_running_variance_leaves_the_gate():
    """Two ranks, one frame of 1 x 2 each: M = 4, the unbiased variance is 4 / 3 of the biased one.  Shows in running_var."""
    c = cases.bn_case(0.2, True, n=2, h=1, w=2)
    us = bso.split(c["u"], (1, 1))
    u = c["u"]
    want_mean = (1 - bso.MOMENTUM) * c["mean"] + bso.MOMENTUM * u.mean(dim=(0, 2, 3))
    want_var = (1 - bso.MOMENTUM) * c["var"] + bso.MOMENTUM * u.var(dim=(0, 2, 3), unbiased=True)
    mean, var = bso.running_update(c["mean"], c["var"], us)
    assert pgo.fraction(mean, want_mean) <= EXACT and pgo.fraction(var, want_var) <= EXACT
    _, wrong = bso.running_update(c["mean"], c["var"], us, biased_running_var=True)
    f = pgo.fraction(wrong, want_var)
    print(f"biased running variance at M = 4: running_var at {f:.2e} of |b| + rms(b) (gate {pgo.TOL:.0e})")
    assert f > 10 * pgo.TOL


def test_every_rank_has_frames_is_shard_bounds():
    for world in range(1, 9):
        for n in range(0, 21):
            bounds = [kb.dist.shard_bounds(n, r, world) for r in range(world)]
            assert kb.dist.every_rank_has_frames(n, world) == all(hi > lo for lo, hi in bounds), (n, world)


def test_group_arguments():
    KbnError = kb._lib.KbnError
    g = kb.dist.BatchNormGroup(0, 1)
    assert (g.rank, g.world, g.collective) == (0, 1, False)
    assert kb.dist.BatchNormGroup(0, 1, reduce_single=True).collective is False      # no process group: nothing to run them on
    for rank, world in ((1, 1), (-1, 2), (0, 0)):
        with pytest.raises(KbnError):
            kb.dist.BatchNormGroup(rank, world)
    with pytest.raises(KbnError, match="process group"):
        kb.dist.BatchNormGroup(0, 2)
    with pytest.raises(KbnError, match="float64"):
        g.gather(torch.zeros(3, dtype=torch.float64))      # a CPU vector: no CPU fallback


def test_sync_batch_norm_reaches_every_layer_and_keeps_the_refusals():
    KbnError = kb._lib.KbnError
    cpu = torch.device("cpu")
    g = kb.dist.BatchNormGroup(0, 1)
    m = kb.modules.PoseNetModel(device=cpu, n_filters=pgo.FILTERS)
    assert m.sync_batch_norm(g) is m
    assert all(layer.sync_group is g for layer in m.encoder.layers())
    assert m.sync_batch_norm(None) is m and all(layer.sync_group is None for layer in m.encoder.layers())
    with pytest.raises(KbnError, match="BatchNormGroup"):
        m.sync_batch_norm("all")
    r = kb.posenet_resnet.ResNetPoseNetModel(n_layer=18, device=cpu, n_filters=[8, 8, 16, 16, 32], decoder_filters=[16, 16], trainable=True)
    assert r.sync_batch_norm(g) is r
    layers = [l for net in r.modules() for l in net.modules() if isinstance(l, kb.posenet.PoseConv2d)]
    assert len(layers) == 1 + 3 * 8 + 2 and all(l.sync_group is g for l in layers)
    frozen = kb.posenet_resnet.ResNetPoseNetModel(n_layer=18, device=cpu, n_filters=[8, 8, 16, 16, 32], decoder_filters=[16, 16])
    with pytest.raises(KbnError, match="trainable"):
        frozen.sync_batch_norm(g)


def test_the_new_entry_points_are_declared_bound_and_built():
    header = open(os.path.join(ROOT, "include", "kbnet_hip.h")).read()
    declared = set(re.findall(r"\b(kbn_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    for name in ENTRY_POINTS:
        assert name in declared and name in kb._lib.SIGNATURES, name
    assert "bn_sync.hip" in kb._build.SOURCES
    source = open(os.path.join(os.path.dirname(kb._build.__file__), "csrc", "bn_sync.hip")).read()
    for name in ENTRY_POINTS:
        assert f'extern "C" int {name}(' in source, name
