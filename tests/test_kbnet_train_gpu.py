"""GPU: KBNetModel(trainable=True) with gradients on, against the reference's own autograd (tests/golden/kbnet_grad_*.npz) and the
fp64 oracle (tests/kbnet_grad_oracle.py).

Gate: |a - b| <= TOL |b| + TOL rms(b) per parameter gradient (kbnet_grad_oracle.TOL); the depth at the forward's 1e-4 rule.  Against
the goldens the comparison is direct.  Against the oracle the fp64 network is differentiated on the activation branches the device took
(read from `return_inner`), after kink_check has shown that the ones that differ from fp64 are a handful AT the kink.

    python -m pytest tests -m gpu -q
"""
import pytest
import torch

import kbnet_amd as kb
KbnError = kb._lib.KbnError

import kbnet_grad_cases as cases
import kbnet_grad_oracle as kgo
import resnet_pose_grad_cases as rcases
from oracle import kbnet_oracle as orc

pytestmark = pytest.mark.gpu
STEP = 1e-6      # the learning rate of the SGD step below: on the CPU oracle it moves the depth by 8 %, hundreds of times the forward's gate


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need a visible MI355X (run with -m gpu on a GPU box)")
    kb._lib.load()   # a missing extension is an error on a GPU box, never a skip
    return torch.device("cuda:0")


def _model(dev, c, sds, trainable=True):
    m = kb.modules.KBNetModel.from_config(c["cfg"], dev, trainable=trainable)
    m.load_state_dicts(*sds)
    return m


def _named(m):
    for grp, mod in zip(kgo.GROUPS, m.modules()):
        for k, p in mod.named_parameters():
            yield f"{grp}::{k}", p


def _grads(m, c):
    """Every parameter's .grad; the ones no forward touched must have none."""
    got, unused = {}, cases.untouched(c)
    for key, p in _named(m):
        if key in unused:
            assert p.grad is None, key
        else:
            assert p.grad is not None, key
            got[key] = p.grad
    assert all(k in dict(_named(m)) for k in unused)
    return got


def _compare(label, got, want, tol=None):
    tol = kgo.TOL if tol is None else tol
    keys = kgo.gradient_keys(want)
    assert sorted(keys) == sorted(got), label
    figures = {k: kgo.fraction(got[k], want[k]) for k in keys}
    worst = max(figures, key=figures.get)
    print(f"{label}: worst {figures[worst]:.2e} at {worst} (gate {tol:.0e}); " + ", ".join(f"{k.split('::')[1].split('.conv')[0]} {v:.1e}" for k, v in figures.items()))
    for k, v in figures.items():
        assert torch.isfinite(got[k]).all() and float(got[k].abs().max()) > 0, (label, k)
        assert v <= tol, (label, k, v)


def _depth_close(depth, want):
    err = float(((depth.detach().double().cpu() - want).abs() / want.abs()).max())
    assert err < 1e-4, err


def _run(dev, c):
    args = cases.inputs(c)
    m = _model(dev, c, args[4:7])
    depth, inner = m.forward(*[t.to(dev) for t in args[:4]], return_inner=True)
    assert depth.grad_fn is not None and depth.dtype == torch.float32 and tuple(depth.shape) == (c["n"], 1, c["h"], c["w"])
    assert list(inner) == kgo.activation_names(c["cfg"].resolutions_backprojection, c["cfg"].n_convolution_sparse_to_dense_pool)
    (depth * args[7].float().to(dev)).sum().backward()
    return m, _grads(m, c), depth, inner, args


def test_the_kitti_preset_has_34_activations():
    assert len(kgo.activation_names(kb.kitti_config().resolutions_backprojection)) == 34


@pytest.mark.parametrize("name", list(cases.GOLDEN))
def test_narrow_model_against_the_references_autograd(dev, name):
    c = cases.GOLDEN[name]
    gold = cases.golden(name)
    _, got, depth, _, _ = _run(dev, c)
    assert sorted(set(kgo.parameter_keys(*cases.inputs(c)[4:7])) - set(kgo.gradient_keys(gold))) == sorted(cases.untouched(c))
    _depth_close(depth, gold["depth"])
    _compare(name, got, gold)


@pytest.mark.parametrize("name", list(cases.MODEL))
def test_model_against_the_fp64_oracle(dev, name):
    c = cases.MODEL[name]
    _, got, depth, inner, args = _run(dev, c)
    masks = kgo.masks_of(inner)
    want = kgo.gradients(*args, c["cfg"], masks=masks)
    kinks = kgo.check_kinks(masks, want["pre"])
    print(f"{name}: {kinks} activations on the other side of the kink than in fp64")
    _depth_close(depth, want["depth"])
    _compare(name, got, want)


def test_frame_order_leaves_the_gradients_inside_the_gate(dev):
    """Five frames in another order (no frame keeps its place), the cotangent with them: every parameter gradient is a sum over the
    frames in another order, so it stays within the gate of the SAME oracle result.  The input side moves with its frame: the
    gradient with respect to the logits (a hook on the depth mapping's node), against cot * d depth / d logits of the oracle's fp64
    logits -- the first data gradient of the backward pass, one row per pixel."""
    c = cases.MODEL["tiny_n5"]
    args = cases.inputs(c)
    n = c["n"]
    perm = torch.roll(torch.arange(n), 2)
    inv = torch.argsort(perm)
    assert not bool((perm == torch.arange(n)).any())
    m = _model(dev, c, args[4:7])
    depth, inner = m.forward(*[t[perm].to(dev) for t in args[:4]], return_inner=True)
    seen = []
    depth.grad_fn.register_hook(lambda grad_inputs, grad_outputs: seen.append(grad_inputs[0].detach().clone()))
    (depth * args[7][perm].float().to(dev)).sum().backward()
    got = _grads(m, c)
    masks = kgo.masks_of({k: t.detach().cpu()[inv] for k, t in inner.items()})
    want = kgo.gradients(*args, c["cfg"], masks=masks)
    kgo.check_kinks(masks, want["pre"])
    _depth_close(depth.detach().cpu()[inv], want["depth"])
    _compare("tiny_n5, frames permuted", got, want)
    assert len(seen) == 1 and tuple(seen[0].shape) == (n, 1, c["h"], c["w"])
    dmin = c["cfg"].min_predict_depth
    s = torch.sigmoid(want["logits"])
    grad_logits = -args[7] * want["depth"] ** 2 / dmin * s * (1 - s)
    f = kgo.fraction(seen[0].cpu()[inv], grad_logits)
    print(f"tiny_n5, frames permuted: the logits' gradient at {f:.2e} of |b| + rms(b) (gate {kgo.TOL:.0e})")
    assert f <= kgo.TOL


def test_trainable_without_gradients_is_the_default_models_fused_forward(dev):
    c = cases.MODEL["full_width"]
    args = cases.inputs(c)
    frames = [t.to(dev) for t in args[:4]]
    ops = kb.ops

    def counted(model):
        ops.PROFILE = []
        try:
            out = model.forward(*frames)
            return out, len(ops.PROFILE)
        finally:
            ops.PROFILE = None

    want, launches = counted(_model(dev, c, args[4:7], trainable=False))
    m = _model(dev, c, args[4:7])
    with torch.no_grad():
        quiet, n_quiet = counted(m)
    assert quiet.grad_fn is None and torch.equal(quiet, want) and n_quiet == launches
    assert m.requires_grad_(False) is m
    frozen, n_frozen = counted(m)
    assert frozen.grad_fn is None and torch.equal(frozen, want) and n_frozen == launches
    out = torch.empty_like(want)
    assert m.forward(*frames, out=out) is out and torch.equal(out, want)
    m.requires_grad_(True)
    recorded = m.forward(*frames)
    assert recorded.grad_fn is not None
    _depth_close(recorded, want.double().cpu())
    assert len(m.parameters()) == len(_model(dev, c, args[4:7], trainable=False).parameters())
    with pytest.raises(KbnError, match="inference only"):
        m.train()
    assert all(mod.training is False for top in m.modules() for mod in top.modules())


def test_refusals(dev):
    c = cases.MODEL["tiny"]
    args = cases.inputs(c)
    frames = [t.to(dev) for t in args[:4]]
    m = _model(dev, c, args[4:7])
    for i, name in enumerate(("image", "sparse_depth", "validity_map_depth", "intrinsics")):
        bad = list(frames)
        bad[i] = bad[i].clone().requires_grad_(True)
        with pytest.raises(KbnError, match=name):
            m.forward(*bad)
    with pytest.raises(KbnError, match="out="):
        m.forward(*frames, out=torch.empty((1, 1, c["h"], c["w"]), device=dev))
    with pytest.raises(KbnError, match="return_logits"):
        m.forward(*frames, return_logits=True)
    with torch.no_grad():
        with pytest.raises(KbnError, match="return_inner"):
            m.forward(*frames, return_inner=True)
    plain = _model(dev, c, args[4:7], trainable=False)
    with pytest.raises(KbnError, match="trainable=True"):
        plain.requires_grad_(True)
    with pytest.raises(KbnError, match="return_inner"):
        plain.forward(*frames, return_inner=True)
    assert plain.forward(*frames).grad_fn is None      # grad mode on, parameters that require grad: still the fused forward


def test_gradients_reach_the_depth_parameters_through_compute_loss(dev):
    """The reference's training step (src/kbnet.py:392-453) up to the optimizer: depth forward, two pose forwards, compute_loss,
    loss.backward().  The depth network's gradients are the fp64 oracle's chain fed with the d loss / d depth the HIP loss backward
    delivered; bar: the loss backward's own 1e-3."""
    c = cases.MODEL["full_width"]
    _, _, _, _, s2d, enc, dec, _ = cases.inputs(c)
    i0, i1, i2, _, sparse, validity, k, _, _ = kb.synthetic.make_triplet(1, c["h"], c["w"], "kitti", seed=12)
    m = _model(dev, c, (s2d, enc, dec))
    rc = rcases.MODEL["full_18_running"]
    _, _, penc, pdec, _ = rcases.inputs(rc)
    pose_model = kb.posenet_resnet.ResNetPoseNetModel(n_layer=18, device=dev, trainable=True)
    pose_model.load_state_dicts(penc, pdec)
    pose_model.requires_grad_(True)
    d0, d1, d2 = i0.to(dev), i1.to(dev), i2.to(dev)
    depth, inner = m.forward(d0, sparse.to(dev), validity.to(dev), k.to(dev), return_inner=True)
    depth.retain_grad()
    pose01, pose02 = pose_model.forward(d0, d1), pose_model.forward(d0, d2)
    loss, _ = m.compute_loss(d0, d1, d2, depth, sparse.to(dev), validity.to(dev), k.to(dev), pose01, pose02)
    loss.backward()
    assert depth.grad is not None and float(depth.grad.abs().max()) > 0
    assert all(p.grad is not None for p in pose_model.encoder.conv1.parameters())
    got = _grads(m, c)
    masks = kgo.masks_of(inner)
    want = kgo.gradients(i0, sparse, validity, k, s2d, enc, dec, depth.grad.double().cpu(), c["cfg"], masks=masks)
    kgo.check_kinks(masks, want["pre"])
    _compare("through compute_loss", got, want, tol=1e-3)


def test_an_optimizer_step_reaches_the_next_forward(dev):
    """One SGD step changes every used weight in place; the next forward (recorded and fused) runs on the new weights: the packed
    blobs follow the parameters' versions.  Each matches the oracle on the updated weights."""
    c = cases.GOLDEN["kbnet_grad_kitti_odd"]
    args = cases.inputs(c)
    cfg = c["cfg"]
    frames = [t.to(dev) for t in args[:4]]
    m = _model(dev, c, args[4:7])
    opt = torch.optim.SGD(m.parameters(), lr=STEP)
    before = m.forward(*frames)
    (before * args[7].float().to(dev)).sum().backward()
    opt.step()
    opt.zero_grad()
    sds = [{k: v.detach().cpu() for k, v in mod.state_dict().items()} for mod in m.modules()]
    unused = cases.untouched(c)
    for grp, new, old in zip(kgo.GROUPS, sds, args[4:7]):
        for k in new:
            assert torch.equal(new[k], old[k]) == (f"{grp}::{k}" in unused), k
    ref = orc.kbnet_forward(*args[:4], *sds, cfg.min_pools, cfg.max_pools, cfg.min_predict_depth, cfg.max_predict_depth,
                            cfg.resolutions_backprojection, orc.activation_slope(cfg.activation_func)).double()
    moved = float(((before.detach().double().cpu() - ref).abs() / ref.abs()).max())
    assert moved > 1e-2, moved             # the step moved the depth far outside the forward's gate
    recorded = m.forward(*frames)
    with torch.no_grad():
        fused = m.forward(*frames)
    assert recorded.grad_fn is not None and fused.grad_fn is None
    _depth_close(recorded, ref)
    _depth_close(fused, ref)
