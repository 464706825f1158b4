"""GPU: ops.augment (csrc/augment.hip) and kb.transforms.Transforms against the NumPy oracle (tests/transforms_oracle.py) at the
cases of tests/transforms_cases.py -- bit for bit, but the Gaussian noise, which is held to transforms_oracle.GAUSS_GATE against
the fp64 evaluation of the same draws (tests/test_transforms_cpu.py measures the gate; tests/test_transforms_power_cpu.py shows that
these comparisons see the mistakes worth making) -- and one training iteration fed through transforms.train_inputs.

    python -m pytest tests/test_transforms_gpu.py -m gpu -q
"""
import numpy as np
import pytest
import torch

import kbnet_amd as kb
import posenet_grad_oracle as pgo
import transforms_cases as tc
import transforms_oracle as to

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need a visible MI355X (run with -m gpu on a GPU box)")
    kb._lib.load()   # a missing extension is an error on a GPU box, never a skip
    return torch.device("cuda:0")


def _put(x, dev, left=None):
    """x on the device: dense, or (left given) as a view `left` elements into the rows of a base tensor whose rows are 8 longer,
    filled with NaN around it."""
    t = torch.from_numpy(np.ascontiguousarray(x))
    if left is None:
        return t.to(dev)
    n, c, h, w = t.shape
    base = torch.full((n, c, h, w + 8), float("nan"), device=dev)
    view = base[..., left:left + w]
    view.copy_(t)
    assert not view.is_contiguous() and view.storage_offset() == left
    return view


def _run(case, dev, **override):
    """ops.augment on the case: (images, ranges, validity) as lists of NumPy arrays.  Asserts what holds for every call: new dense
    outputs at addresses of their own, inputs unchanged."""
    ins = [[_put(x, dev, case["left"]) for x in case[key]] for key in ("images", "ranges", "validity")]
    before = [[t.clone() for t in lst] for lst in ins]
    densities = None if case["densities"] is None else torch.from_numpy(case["densities"]).to(dev)
    outs = kb.ops.augment(*ins, case["flags"], densities, **dict(case["options"], **override))
    torch.cuda.synchronize()
    held = {t.data_ptr() for lst in ins for t in lst}
    for lst, olst, blst in zip(ins, outs, before):
        assert len(lst) == len(olst)
        for t, o, b in zip(lst, olst, blst):
            assert o.shape == t.shape and o.is_contiguous() and o.dtype == torch.float32 and o.data_ptr() not in held
            assert torch.equal(t.view(torch.int32) if t.is_contiguous() else t.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return [[o.cpu().numpy() for o in lst] for lst in outs]


def _check(case, dev):
    want = tc.expected(case)
    got = _run(case, dev)
    found = tc.mismatches(case, got, want=want)
    assert found == [], (case["name"], found)
    return got, want


# -------------------------------------------------------------------------------------------------------------- nothing to do
@pytest.mark.parametrize("rng", [[0, 1], [-1, 1], [0, 255]], ids=["0_1", "m1_1", "0_255"])
def test_nothing_to_do(dev, rng):
    """p = 0, and all-zero flags: the images are ops.preprocess's normalised images bit for bit ([0, 255]: bit-equal copies at fresh
    addresses), the maps bit-equal copies, every input unchanged."""
    g = np.random.default_rng(21)
    image = torch.from_numpy(g.integers(0, 256, size=(3, 3, 19, 44)).astype(np.float32)).to(dev)
    sparse = torch.from_numpy(tc._depth(g, 3, 1, 19, 44, 0.2)).to(dev)
    validity = (sparse > 0).float()
    keep = [t.clone() for t in (image, sparse, validity)]
    want_image = kb.ops.preprocess(image, sparse, normalized_image_range=rng)[0]
    t = kb.transforms.Transforms(normalized_image_range=rng, random_flip_type=["horizontal", "vertical"], random_remove_points=[0.6, 0.7],
                                 random_noise_type="uniform", random_noise_spread=0.5, seed=1)
    np.random.seed(0)
    [a], [b], [c] = t.transform([image], [sparse], [validity], random_transform_probability=0.0)
    [a2], [b2], [c2] = kb.ops.augment([image], [sparse], [validity], [0, 0, 0], None, normalized_image_range=rng)
    torch.cuda.synchronize()
    ints = lambda x: x.view(torch.int32)
    for got_image, got_sparse, got_validity in ((a, b, c), (a2, b2, c2)):
        assert torch.equal(ints(got_image), ints(want_image))
        assert torch.equal(ints(got_sparse), ints(sparse)) and torch.equal(ints(got_validity), ints(validity))
        assert len({x.data_ptr() for x in (got_image, got_sparse, got_validity, image, sparse, validity)}) == 6
    if rng == [0, 255]:
        assert torch.equal(ints(a), ints(image))
    for x, k in zip((image, sparse, validity), keep):
        assert torch.equal(ints(x), ints(k))
    # the single list when only one is not empty, as the reference returns it
    only = t.transform([image, image], random_transform_probability=0.0)
    assert isinstance(only, list) and len(only) == 2 and torch.equal(only[1], want_image)


# ---------------------------------------------------------------------------------------------------------------------- flips
@pytest.mark.parametrize("case", tc.flip_cases(), ids=lambda c: c["name"].replace(" ", "_"))
def test_flips(dev, case):
    _check(case, dev)


# -------------------------------------------------------------------------------------------------------------------- removal
@pytest.mark.parametrize("case", [tc.removal_edge_case(), tc.removal_edge_case(True), tc.removal_kitti_case(), tc.removal_dense_case(),
                                  tc.removal_two_channel_case()], ids=lambda c: c["name"].replace(" ", "_"))
def test_removal(dev, case):
    """The removed set is the oracle's and has k elements, frame by frame and map by map; and the call that produced it never
    waited for the device (torch's sync debug mode raises on a synchronising call)."""
    got, want = _check(case, dev)
    for i, src in enumerate(case["ranges"]):
        for b, f in enumerate(case["flags"]):
            info = want[3][i][b]
            out = to.flip(got[1][i][b], f)          # a flip is its own inverse: back to source coordinates
            removed = (src[b] > 0) & (out == 0)
            assert np.array_equal(removed, info["removed"]) and int(removed.sum()) == info["k"], (case["name"], i, b)
            assert np.array_equal(out[~removed].view(np.uint32), src[b][~removed].view(np.uint32))
            if f & to.REMOVE:
                assert info["k"] == to.removal_count(case["densities"][b], int((src[b] > 0).sum()))
    ins = [[_put(x, dev) for x in case[key]] for key in ("images", "ranges", "validity")]
    densities = torch.from_numpy(case["densities"]).to(dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        outs = kb.ops.augment(*ins, case["flags"], densities, **case["options"])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert tc.mismatches(case, [[o.cpu().numpy() for o in lst] for lst in outs], want=want) == []


def test_tie_at_the_boundary(dev):
    """Two equal keys with the cut between them: the element with the smaller index goes, the other stays."""
    case, r = tc.tie_case()
    key, e = to.removal_keys((1, 192, 640), 0, 0, tc.TIE_SEED, 0)
    order = np.lexsort((e, key))
    assert key[order][r] == key[order][r + 1] and to.removal_count(case["densities"][0], key.size) == r + 1      # the premise, in fp32
    got, want = _check(case, dev)
    out = got[1][0].reshape(-1)
    assert int((out == 0).sum()) == r + 1 and out[e[order][r]] == 0 and out[e[order][r + 1]] != 0
    assert np.array_equal(out == 0, want[3][0][0]["removed"].reshape(-1))


# ---------------------------------------------------------------------------------------------------------------------- noise
@pytest.mark.parametrize("noise_type", ["uniform", "gaussian"])
def test_noise(dev, noise_type):
    """Uniform: bit-equal.  Gaussian: within the gate of the fp64 oracle.  Noise only where the value after removal was positive,
    removed points stay 0, two range maps (of equal data) get different draws."""
    case = tc.noise_case(noise_type)
    got, want = _check(case, dev)
    spread = case["options"]["noise_spread"]
    if noise_type == "gaussian":
        w64 = tc.expected(case, dtype=np.float64)
        worst = max(float(np.abs(g.astype(np.float64) - w).max()) for g, w in zip(got[1], w64[1])) / spread
        print(f"gaussian: device {worst:.3e} x spread from the fp64 oracle, gate {to.GAUSS_GATE:.1e}")
    for i, src in enumerate(case["ranges"]):
        for b, f in enumerate(case["flags"]):
            out = to.flip(got[1][i][b], f)
            removed = want[3][i][b]["removed"]
            alive = (src[b] > 0) & ~removed
            assert not out[removed].any(), (i, b)
            if f & to.NOISE:
                assert not out[~alive].any(), (i, b)                # zeros, negatives and removed points are 0 after the mask
                assert (out[alive] != src[b][alive]).all() and float(np.abs(out[alive] - src[b][alive]).max()) <= spread * (0.5 if noise_type == "uniform" else 6.0)
            else:
                assert np.array_equal(out[~removed], src[b][~removed])
    assert np.array_equal(case["ranges"][0], case["ranges"][1]) and not np.array_equal(got[1][0], got[1][1])


# ---------------------------------------------------------------------------------------------------------------- determinism
def test_determinism(dev):
    case = tc.noise_case("uniform")
    first, again, later = _run(case, dev), _run(case, dev), _run(case, dev, call=case["options"]["call"] + 1)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for x, y in zip(first, again) for a, b in zip(x, y))
    assert not np.array_equal(first[1][0], later[1][0])
    assert tc.mismatches(case, later, want=tc.expected(case, call=case["options"]["call"] + 1)) == []
    other_seed = _run(case, dev, seed=case["options"]["seed"] + 1)
    assert not np.array_equal(first[1][0], other_seed[1][0])
    # two Transforms objects with one seed agree call for call (the decisions and densities are fixed from outside)
    kwargs = dict(normalized_image_range=[0, 1], random_flip_type=["horizontal"], random_remove_points=[0.6, 0.7], random_noise_type="gaussian",
                  random_noise_spread=0.1)
    one, two = kb.transforms.Transforms(seed=42, **kwargs), kb.transforms.Transforms(seed=42, **kwargs)
    x = _put(case["ranges"][0], dev)
    results = []
    for t in (one, two):
        per_call = []
        for call in range(3):
            np.random.seed(9)
            torch.manual_seed(9)
            per_call.append(t.transform([], [x], [], random_transform_probability=1.0))
        assert t.calls == 3
        results.append(per_call)
    torch.manual_seed(9)
    densities = (0.7 - 0.6) * torch.rand(4, device=dev) + 0.6
    np.random.seed(9)
    flags = one.draw(4, 1.0)
    assert any(f & to.REMOVE for f in flags) and any(f & to.NOISE for f in flags)
    for call in range(3):
        assert isinstance(results[0][call], list) and torch.equal(results[0][call][0].view(torch.int32), results[1][call][0].view(torch.int32))
        [direct] = kb.ops.augment([], [x], [], flags, densities, noise_type="gaussian", noise_spread=0.1, seed=42, call=call)[1]
        assert torch.equal(direct.view(torch.int32), results[0][call][0].view(torch.int32))
    assert not torch.equal(results[0][0][0], results[0][1][0])


# ----------------------------------------------------------------------------------------------------- one training iteration
def test_one_training_iteration_through_train_inputs(dev):
    """Reference src/kbnet.py:396-453 over this package: train_inputs, KBNetModel(trainable).forward, two pose forwards, compute_loss,
    backward, kb.optim.Adam.step -- on the narrow KITTI configuration at 2 x 3 x 32 x 64."""
    cfg = kb.kitti_config().narrow()
    depth_model = kb.modules.KBNetModel.from_config(cfg, dev, trainable=True)
    depth_model.load_state_dicts(*kb.synthetic.make_state_dicts(cfg, seed=0, gain=1.3))
    pose_model = kb.modules.PoseNetModel(device=dev, n_filters=pgo.FILTERS)
    pose_model.load_state_dicts(*kb.synthetic.make_posenet_weights(pgo.FILTERS, seed=5))
    pose_model.requires_grad_(True).set_batch_norm("running")
    i0, i1, i2, _, sparse, _, k, _, _ = kb.synthetic.make_triplet(2, 32, 64, "kitti", seed=31)
    image0, image1, image2 = ((255.0 * i).to(dev) for i in (i0, i1, i2))
    sparse, k = sparse.to(dev), k.to(dev)
    transforms = kb.transforms.Transforms(normalized_image_range=[0, 1], random_flip_type=["none"], random_remove_points=[0.60, 0.70],
                                          random_noise_type="none", random_noise_spread=-1, seed=3)       # the KITTI script's options
    np.random.seed(1)
    torch.manual_seed(1)
    flags = transforms.draw(2, 1.0)
    assert any(f & to.REMOVE for f in flags)
    np.random.seed(1)
    a0, a1, a2, a_sparse, filtered_sparse, filtered_validity = kb.transforms.train_inputs(transforms, image0, image1, image2, sparse, 1.0)
    assert 0 < int((a_sparse > 0).sum()) < int((sparse > 0).sum()) and float(a0.max()) <= 1.0
    _, want_validity, want_filtered = kb.ops.preprocess(None, sparse)
    assert torch.equal(filtered_sparse, want_filtered) and torch.equal(filtered_validity, want_validity)
    params = depth_model.parameters() + pose_model.parameters()
    opt = kb.optim.Adam([{"params": depth_model.parameters(), "weight_decay": 1e-4}, {"params": pose_model.parameters(), "weight_decay": 1e-4}], lr=1e-4)
    old = [p.detach().clone() for p in params]
    out = depth_model.forward(a0, a_sparse, filtered_validity, k)
    pose01, pose02 = pose_model.forward(a0, a1), pose_model.forward(a0, a2)
    loss, _ = depth_model.compute_loss(a0, a1, a2, out, filtered_sparse, filtered_validity, k, pose01, pose02)
    opt.zero_grad()
    loss.backward()
    opt.step()
    assert bool(torch.isfinite(loss.detach()))
    with_grad = [p for p in params if p.grad is not None]
    assert len(with_grad) >= len(params) - 2 and all(bool(torch.isfinite(p.grad).all()) for p in with_grad)
    assert any(not torch.equal(p.detach(), o) for p, o in zip(params, old))
    assert all(bool(torch.isfinite(p.detach()).all()) for p in params)
