"""GPU: ops.adam_step (csrc/adam.hip) as an operator against the fp64 formula, kb.optim.Adam over step sequences against the fp64
oracle at the gates tests/test_adam_cpu.py measures, the version contract behind the packed-weight caches, one real training step
against torch.optim.Adam on bit-equal gradients, and resume through save_model / restore_model.

Operator bound: adam_oracle.one_step derives, from the roundings of the formula in its stated order, what an fp32 evaluation may
differ from the fp64 one by, per element, for p, m and v.  Sequence gates: adam_oracle.TOL_P / TOL_M / TOL_V.

    python -m pytest tests/test_adam_gpu.py -m gpu -q
"""
import pytest
import torch

import kbnet_amd as kb
import adam_oracle as ao
import kbnet_grad_cases as cases
import kbnet_grad_oracle as kgo
import resnet_pose_grad_cases as rcases
from oracle import kbnet_oracle as orc

KbnError = kb._lib.KbnError
pytestmark = pytest.mark.gpu
CAP, PASS = kb.ops.ADAM_TABLE_CAPACITY, kb.ops.ADAM_PASS_ELEMENTS
HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
UNUSED = "enc::calibrated_backprojection4.conv_image.conv_block.0.conv.weight"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need a visible MI355X (run with -m gpu on a GPU box)")
    kb._lib.load()   # a missing extension is an error on a GPU box, never a skip
    return torch.device("cuda:0")


def _tensors(sizes, seed, scale=1.0):
    """(p, g, m, v) lists, CPU fp32: states as a few steps of history would leave them (v >= 0)."""
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda n: torch.randn(n, generator=gen, dtype=torch.float64)
    p = [(0.1 * rnd(n)).float() for n in sizes]
    g = [(scale * rnd(n)).float() for n in sizes]
    m = [(0.3 * scale * rnd(n)).float() for n in sizes]
    v = [(0.1 * scale * scale * rnd(n) ** 2).float() for n in sizes]
    return p, g, m, v


def _check(got, inputs, t, lr, betas, eps, wd, label):
    """One tensor's device result against the fp64 formula, element by element, at one_step's bound."""
    want_p, want_m, want_v, dp, dm, dv = ao.one_step(*inputs, t, lr, betas, eps, wd)
    worst = {}
    for name, a, b, d in (("p", got[0], want_p, dp), ("m", got[1], want_m, dm), ("v", got[2], want_v, dv)):
        a = a.detach().double().cpu().reshape(-1)
        b, d = b.reshape(-1), d.reshape(-1)
        assert bool(torch.isfinite(a).all()), (label, name)
        err = (a - b).abs()
        worst[name] = float((err / d.clamp_min(1e-300)).max()) if err.numel() else 0.0
        assert bool((err <= d).all()), (label, name, worst[name])
    return worst


def _on(dev, tensors):
    return [t.to(dev) for t in tensors]


@pytest.mark.parametrize("wd", [0.0, 1e-4])
def test_operator_against_the_fp64_formula(dev, wd):
    """Sizes around the vector width and the block, one tensor longer than one pass of the widest grid (PASS = 512 blocks x 256
    threads x 4: its stride loop runs twice), a view one element into its storage (misaligned: the scalar path), an empty tensor."""
    sizes = [1, 3, 4, 5, 1023, 1024, 1025, 40003, PASS + 4099, 0]
    p, g, m, v = _tensors(sizes, seed=3)
    dp, dg, dm, dv = (_on(dev, x) for x in (p, g, m, v))
    # the misaligned case: all four are views at a storage offset of one element
    op, og, om, ov = _tensors([1027], seed=4)
    views = [torch.cat([torch.zeros(1), x[0]]).to(dev)[1:] for x in (op, og, om, ov)]
    assert all(x.data_ptr() % 16 == 4 and x.is_contiguous() for x in views)
    assert all(x.data_ptr() % 16 == 0 for x in dp[:-1])
    p.append(op[0]); g.append(og[0]); m.append(om[0]); v.append(ov[0])
    dp.append(views[0]); dg.append(views[1]); dm.append(views[2]); dv.append(views[3])
    versions = [x._version for x in dp]
    kb.ops.adam_step(dp, dg, dm, dv, [7] * len(dp), weight_decay=wd, **HYPER)
    worst = {}
    for i in range(len(dp)):
        w = _check((dp[i], dm[i], dv[i]), (p[i], g[i], m[i], v[i]), 7, HYPER["lr"], HYPER["betas"], HYPER["eps"], wd, f"tensor {i}")
        worst = {k: max(worst.get(k, 0.0), x) for k, x in w.items()}
        assert torch.equal(dg[i].cpu(), g[i])                                   # the gradient is read only
        assert (dp[i]._version > versions[i]) == (p[i].numel() > 0)
        if p[i].numel():
            assert not torch.equal(dp[i].cpu(), p[i])
    print(f"wd {wd}: worst error / bound: p {worst['p']:.2f}, m {worst['m']:.2f}, v {worst['v']:.2f}")


def test_entry_point_skips_an_empty_record_inside_a_table(dev):
    p, g, m, v = _tensors([9, 9], seed=5)
    dp, dg, dm, dv = (_on(dev, x) for x in (p, g, m, v))
    rec = (kb._lib.AdamTensor * 3)()
    for r, i in ((rec[0], 0), (rec[2], 1)):
        r.param, r.grad, r.exp_avg, r.exp_avg_sq, r.numel = dp[i].data_ptr(), dg[i].data_ptr(), dm[i].data_ptr(), dv[i].data_ptr(), 9
        r.weight_decay, r.one_minus_beta1, r.beta2, r.one_minus_beta2, r.eps = 0.0, 0.1, 0.999, 0.001, 1e-8
        r.step_size, r.bc2_sqrt = 1e-3 / (1 - 0.9 ** 2), (1 - 0.999 ** 2) ** 0.5
    lib = kb._lib.load()
    assert rec[1].numel == 0 and not rec[1].param
    assert lib.kbn_adam_step(rec, 3, torch.cuda.current_stream().cuda_stream) == 0
    for i in range(2):
        _check((dp[i], dm[i], dv[i]), (p[i], g[i], m[i], v[i]), 2, 1e-3, (0.9, 0.999), 1e-8, 0.0, f"record {i}")
    rec[1].numel = -1
    assert lib.kbn_adam_step(rec, 3, None) == kb._lib.KBN_ERR_INVALID_ARGUMENT
    rec[1].numel = 4                                                            # null pointers with elements to process
    assert lib.kbn_adam_step(rec, 3, None) == kb._lib.KBN_ERR_INVALID_ARGUMENT
    assert lib.kbn_adam_step(rec, 0, None) == kb._lib.KBN_ERR_INVALID_ARGUMENT
    assert lib.kbn_adam_step(None, 3, None) == kb._lib.KBN_ERR_INVALID_ARGUMENT


def test_a_list_longer_than_the_table_takes_the_ceiling_of_launches(dev):
    """3 x capacity + 1 tensors of 5 to 70 elements: every one is updated exactly once (a second update would leave the bound by
    orders of magnitude), in four launches -- one ops.PROFILE record each, or one entry-point call without the profile."""
    count = 3 * CAP + 1
    sizes = [5 + (13 * i) % 66 for i in range(count)]
    assert min(sizes) == 5 and max(sizes) == 70
    p, g, m, v = _tensors(sizes, seed=6)
    runs = []
    for profiled in (True, False):
        dp, dg, dm, dv = (_on(dev, x) for x in (p, g, m, v))
        kb.ops.PROFILE = [] if profiled else None
        try:
            kb.ops.adam_step(dp, dg, dm, dv, [2] * count, weight_decay=1e-4, **HYPER)
            records = kb.ops.PROFILE
        finally:
            kb.ops.PROFILE = None
        if profiled:
            assert len(records) == -(-count // CAP) == 4
            assert [r[0] for r in records] == ["adam_step"] * 4
            assert [r[4] for r in records] == [28.0 * sum(sizes[i:i + CAP]) for i in range(0, count, CAP)]
        for i in range(count):
            _check((dp[i], dm[i], dv[i]), (p[i], g[i], m[i], v[i]), 2, HYPER["lr"], HYPER["betas"], HYPER["eps"], 1e-4, f"tensor {i}")
        runs.append([x.cpu() for x in dp + dm + dv])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_groups_and_step_counts_of_their_own_in_one_call(dev):
    sizes = [130, 7, 2050, 64]
    p, g, m, v = _tensors(sizes, seed=8)
    dp, dg, dm, dv = (_on(dev, x) for x in (p, g, m, v))
    lrs, wds, steps = [1e-3, 1e-3, 2.5e-4, 2.5e-4], [1e-4, 1e-4, 1e-2, 1e-2], [3, 17, 3, 17]
    betas, epss = [(0.9, 0.999)] * 2 + [(0.8, 0.99)] * 2, [1e-8, 1e-8, 1e-6, 1e-6]
    kb.ops.PROFILE = []
    try:
        kb.ops.adam_step(dp, dg, dm, dv, steps, lr=lrs, betas=betas, eps=epss, weight_decay=wds)
        assert len(kb.ops.PROFILE) == 1
    finally:
        kb.ops.PROFILE = None
    for i in range(4):
        _check((dp[i], dm[i], dv[i]), (p[i], g[i], m[i], v[i]), steps[i], lrs[i], betas[i], epss[i], wds[i], f"tensor {i}")
    # the same through the optimizer: two groups, state loaded at steps 3 - 1 and 17 - 1
    params = [torch.nn.Parameter(x.to(dev)) for x in p]
    opt = kb.optim.Adam([{"params": params[:2], "lr": lrs[0], "weight_decay": wds[0]},
                         {"params": params[2:], "lr": lrs[2], "weight_decay": wds[2], "betas": betas[2], "eps": epss[2]}])
    for i, x in enumerate(params):
        x.grad = g[i].to(dev)
        opt.state[x].update(step=torch.tensor(float(steps[i] - 1)), exp_avg=m[i].to(dev), exp_avg_sq=v[i].to(dev))
    opt.step()
    for i, x in enumerate(params):
        s = opt.state[x]
        assert float(s["step"]) == steps[i] and not s["step"].is_cuda
        assert torch.equal(x.detach(), dp[i]) and torch.equal(s["exp_avg"], dm[i]) and torch.equal(s["exp_avg_sq"], dv[i])


def test_refused_tensors(dev):
    p, g, m, v = (_on(dev, x) for x in _tensors([12], seed=9))
    kw = dict(weight_decay=0.0, **HYPER)
    wide = torch.zeros(12, 2, device=dev)
    with pytest.raises(KbnError, match="dense"):
        kb.ops.adam_step([wide[:, 0]], g, m, v, [1], **kw)
    with pytest.raises(KbnError, match="dense"):
        kb.ops.adam_step(p, g, [wide[:, 0]], v, [1], **kw)
    with pytest.raises(KbnError, match="float32"):
        kb.ops.adam_step([p[0].double()], g, m, v, [1], **kw)
    with pytest.raises(KbnError, match="shape"):
        kb.ops.adam_step(p, [g[0][:5]], m, v, [1], **kw)
    with pytest.raises(KbnError, match="steps"):
        kb.ops.adam_step(p, g, m, v, [0], **kw)
    with pytest.raises(KbnError, match="CPU fallback"):
        kb.ops.adam_step(p, [g[0].cpu()], m, v, [1], **kw)
    # a gradient that is not dense is copied, and gives the dense gradient's bits
    q = [x.clone() for x in (p[0], m[0], v[0])]
    strided = torch.stack([g[0], g[0] + 1], dim=1)[:, 0]
    assert not strided.is_contiguous()
    kb.ops.adam_step([q[0]], [strided], [q[1]], [q[2]], [1], **kw)
    kb.ops.adam_step(p, g, m, v, [1], **kw)
    assert torch.equal(q[0], p[0]) and torch.equal(q[1], m[0]) and torch.equal(q[2], v[0])


def test_guards_non_finite_gradients_and_bits(dev):
    """p, g, m and v are views inside larger buffers filled with a sentinel: the sentinels are intact afterwards.  A NaN and a
    +Inf gradient element change only their own elements.  A second run, and a run on a side stream, give the same bits."""
    sizes = [1, 5, 1025, 4099, 40003]
    SENT, PAD = -7.25, 37         # 37 floats: views that are not 16-byte aligned; a second set at PAD 36 is aligned
    cpu = _tensors(sizes, seed=10)

    def run(pad, poison, stream=None):
        bufs, views = [], []
        for lst in cpu:
            bl, vl = [], []
            for x in lst:
                b = torch.full((x.numel() + 2 * pad,), SENT, device=dev)
                b[pad:pad + x.numel()] = x.to(dev)
                bl.append(b)
                vl.append(b[pad:pad + x.numel()])
            bufs.append(bl)
            views.append(vl)
        if poison:
            views[1][3][11] = float("nan")
            views[1][3][12] = float("inf")
            views[1][4][40002] = float("nan")
        torch.cuda.synchronize()
        if stream is None:
            kb.ops.adam_step(*views, [4] * len(sizes), weight_decay=1e-4, **HYPER)
        else:
            with torch.cuda.stream(stream):
                kb.ops.adam_step(*views, [4] * len(sizes), weight_decay=1e-4, **HYPER)
            stream.synchronize()
        torch.cuda.synchronize()
        for bl, vl in zip(bufs, views):
            for b, x in zip(bl, vl):
                assert bool((b[:pad] == SENT).all()) and bool((b[pad + x.numel():] == SENT).all())
        return [[x.cpu() for x in views[k]] for k in (0, 2, 3)]

    for pad in (PAD, 36):
        clean = run(pad, False)
        again = run(pad, False)
        side = run(pad, False, torch.cuda.Stream(device=dev))
        for a, b, c in zip(clean, again, side):
            assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(a, b, c))
        bad = run(pad, True)
        for name, a, b in zip("pmv", clean, bad):
            for i in range(len(sizes)):
                hit = {3: [11, 12], 4: [40002]}.get(i, [])
                keep = torch.ones(sizes[i], dtype=torch.bool)
                for j in hit:
                    keep[j] = False
                    assert not bool(torch.isfinite(b[i][j])), (name, i, j)
                assert torch.equal(a[i][keep], b[i][keep]), (name, i)
        # +Inf: m = Inf, v = Inf, and p = p - step_size Inf / Inf = NaN; NaN: all three NaN
        assert torch.isnan(bad[0][3][11]) and torch.isnan(bad[1][3][11]) and torch.isnan(bad[2][3][11])
        assert torch.isinf(bad[1][3][12]) and torch.isinf(bad[2][3][12]) and torch.isnan(bad[0][3][12])
    aligned = _check([x[4] for x in run(36, False)], [x[4] for x in cpu], 4, HYPER["lr"], HYPER["betas"], HYPER["eps"], 1e-4, "aligned")
    scalar = _check([x[4] for x in run(PAD, False)], [x[4] for x in cpu], 4, HYPER["lr"], HYPER["betas"], HYPER["eps"], 1e-4, "scalar")
    print(f"worst error / bound: 16-byte path {aligned}, scalar path {scalar}")


@pytest.mark.parametrize("name", list(ao.CASES))
def test_sequences_against_the_fp64_oracle_at_the_cpu_gates(dev, name):
    p0, grads, groups = ao.case(name)
    got = ao.run_optimizer(lambda g: kb.optim.Adam(g), p0, grads, groups, device=dev)
    want = ao.case_reference(name)
    lr_sum = sum(ao.lr_schedule())
    fp, fm, fv = ao.p_fraction(got["p"][0], want["p"][0], lr_sum), ao.fraction(got["m"][0], want["m"][0]), ao.fraction(got["v"][0], want["v"][0])
    print(f"{name}: p {fp:.2e} of sum lr (gate {ao.TOL_P:.0e}), m {fm:.2e} (gate {ao.TOL_M:.0e}), v {fv:.2e} (gate {ao.TOL_V:.0e})")
    assert got["step"] == [ao.STEPS]
    assert fp <= ao.TOL_P and fm <= ao.TOL_M and fv <= ao.TOL_V


# ------------------------------------------------------------------------------------------ models
def _depth_model(dev, c, sds, trainable=True):
    m = kb.modules.KBNetModel.from_config(c["cfg"], dev, trainable=trainable)
    m.load_state_dicts(*sds)
    return m


def _named(m):
    for grp, mod in zip(kgo.GROUPS, m.modules()):
        for k, p in mod.named_parameters():
            yield f"{grp}::{k}", p


def _depth_close(depth, want):
    err = float(((depth.detach().double().cpu() - want).abs() / want.abs()).max())
    assert err < 1e-4, err


def test_the_step_bumps_versions_and_reaches_every_later_forward(dev):
    """Modelled on test_an_optimizer_step_reaches_the_next_forward (tests/test_kbnet_train_gpu.py), with kb.optim.Adam: the kernel
    writes through raw pointers, and what tells the packed-weight caches is the version bump of ops.adam_step."""
    c = cases.GOLDEN["kbnet_grad_kitti_odd"]
    assert (c["n"], c["h"], c["w"]) == (2, 45, 77)
    args = cases.inputs(c)
    cfg = c["cfg"]
    frames = [t.to(dev) for t in args[:4]]
    m = _depth_model(dev, c, args[4:7])
    m.requires_grad_(False)
    replay = m.capture(*frames, tune=False)                   # an inference graph, captured BEFORE the step
    captured = replay(*frames).clone()
    m.requires_grad_(True)
    opt = kb.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-4)
    before = m.forward(*frames)
    _depth_close(before, captured.double().cpu())
    (before * args[7].float().to(dev)).sum().backward()
    versions = {k: p._version for k, p in _named(m)}
    old = {k: p.detach().clone() for k, p in _named(m)}
    opt.step()
    opt.zero_grad()
    assert cases.untouched(c) == [UNUSED]
    for k, p in _named(m):
        if k == UNUSED:
            assert torch.equal(p.detach(), old[k]) and p not in opt.state and p._version == versions[k], k
        else:
            assert p._version > versions[k] and not torch.equal(p.detach(), old[k]), k
            assert float(opt.state[p]["step"]) == 1
    sds = [{k: v.detach().cpu() for k, v in mod.state_dict().items()} for mod in m.modules()]
    ref = orc.kbnet_forward(*args[:4], *sds, cfg.min_pools, cfg.max_pools, cfg.min_predict_depth, cfg.max_predict_depth,
                            cfg.resolutions_backprojection, orc.activation_slope(cfg.activation_func)).double()
    moved = float(((before.detach().double().cpu() - ref).abs() / ref.abs()).max())
    assert moved > 1e-3, moved             # the step moved the depth far outside the forward's gate
    recorded = m.forward(*frames)
    with torch.no_grad():
        fused = m.forward(*frames)
    assert recorded.grad_fn is not None and fused.grad_fn is None
    _depth_close(recorded, ref)
    _depth_close(fused, ref)
    fresh = _depth_model(dev, c, sds)
    fresh_recorded = fresh.forward(*frames)
    with torch.no_grad():
        fresh_fused = fresh.forward(*frames)
    assert fresh_recorded.grad_fn is not None
    assert torch.equal(recorded.detach(), fresh_recorded.detach()) and torch.equal(fused, fresh_fused)
    m.requires_grad_(False)
    assert torch.equal(replay(*frames), fresh_fused)          # the graph re-packed what the step changed


RC = rcases.GOLDEN["resnet_pose_grad_18_train"]             # narrow ResNet-18, 2 x 130 x 136: the last BatchNorm sees > 1 value a channel
DC = cases.GOLDEN["kbnet_grad_kitti_odd"]
WD_DEPTH, WD_POSE, LR = 1e-4, 1e-3, 1e-4


def _models(dev):
    depth = _depth_model(dev, DC, cases.inputs(DC)[4:7])
    _, _, enc, dec, _ = rcases.inputs(RC)
    pose = kb.posenet_resnet.ResNetPoseNetModel(n_layer=18, device=dev, n_filters=RC["filters"], decoder_filters=RC["decoder_filters"],
                                                trainable=True)
    pose.load_state_dicts(enc, dec)
    pose.requires_grad_(True).set_batch_norm("batch")
    return depth, pose


def _groups(depth, pose):
    return [{"params": depth.parameters(), "weight_decay": WD_DEPTH}, {"params": pose.parameters(), "weight_decay": WD_POSE}]


_DATA = {}


def _data(dev):
    if not _DATA:
        i0, i1, i2, _, sparse, validity, k, _, _ = kb.synthetic.make_triplet(RC["n"], RC["h"], RC["w"], "kitti", seed=21)
        _DATA["d"] = [t.to(dev) for t in (i0, i1, i2, sparse, validity, k)]
    return _DATA["d"]


def _train_step(dev, depth, pose, opt):
    """The reference's training step (src/kbnet.py:392-453)."""
    i0, i1, i2, sparse, validity, k = _data(dev)
    out = depth.forward(i0, sparse, validity, k)
    pose01, pose02 = pose.forward(i0, i1), pose.forward(i0, i2)
    loss, _ = depth.compute_loss(i0, i1, i2, out, sparse, validity, k, pose01, pose02)
    opt.zero_grad()
    loss.backward()
    opt.step()
    return float(loss.detach())


def _all_params(depth, pose):
    return depth.parameters() + pose.parameters()


def _buffers(depth, pose):
    return [v for top in list(depth.modules()) + list(pose.modules()) for v in top.state_dict().values()]


def test_one_training_step_against_torchs_adam_on_the_same_gradients(dev):
    """Twin models, one compute_loss step each, two groups with their own weight decay: the gradients are bit-equal (the package is
    deterministic), so the two optimizers differ by their own rounding alone.  Both lie within one_step's bound of the fp64
    formula, hence within twice the bound of each other.  One step only: a longer trajectory through the network is
    ill-conditioned in elements whose gradient is near zero."""
    ours_d, ours_p = _models(dev)
    ref_d, ref_p = _models(dev)
    ours = kb.optim.Adam(_groups(ours_d, ours_p), lr=LR)
    ref = torch.optim.Adam(_groups(ref_d, ref_p), lr=LR, foreach=False)
    start = [p.detach().clone() for p in _all_params(ours_d, ours_p)]
    kb.ops.PROFILE = []
    try:
        la = _train_step(dev, ours_d, ours_p, ours)
        launches = sum(1 for r in kb.ops.PROFILE if r[0] == "adam_step")
    finally:
        kb.ops.PROFILE = None
    lb = _train_step(dev, ref_d, ref_p, ref)
    assert la == lb
    a, b = _all_params(ours_d, ours_p), _all_params(ref_d, ref_p)
    used = [i for i, p in enumerate(a) if p.grad is not None]
    assert len(used) < len(a) and launches == -(-len(used) // CAP)
    n_depth = len(ours_d.parameters())
    worst = 0.0
    for i, (x, y, x0) in enumerate(zip(a, b, start)):
        if x.grad is None:
            assert y.grad is None and torch.equal(x.detach(), y.detach()) and torch.equal(x.detach(), x0) and x not in ours.state
            continue
        assert torch.equal(x.grad, y.grad), i
        wd = WD_DEPTH if i < n_depth else WD_POSE
        zero = torch.zeros_like(x0)
        _, _, _, dp, dm, dv = ao.one_step(x0, x.grad, zero, zero, 1, LR, (0.9, 0.999), 1e-8, wd)
        sa, sb = ours.state[x], ref.state[y]
        assert float(sa["step"]) == float(sb["step"]) == 1
        for u, w, d in ((x.detach(), y.detach(), dp), (sa["exp_avg"], sb["exp_avg"], dm), (sa["exp_avg_sq"], sb["exp_avg_sq"], dv)):
            err = (u.double().cpu() - w.double().cpu()).abs()
            assert bool((err <= 2 * d).all()), i
            worst = max(worst, float((err / (2 * d).clamp_min(1e-300)).max()))
        assert not torch.equal(x.detach(), x0)
    print(f"ours vs torch.optim.Adam after one step: worst |a - b| / (2 x bound) {worst:.2f}, {len(used)} tensors in {launches} launches")


def _state_of(opt, params):
    return [(opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) if p in opt.state else None for p in params]


def test_resume_through_save_model_and_restore_model(dev, tmp_path):
    """3 steps, save_model(path, step, optimizer) on both models, restore_model(path, optimizer) into fresh models and a fresh
    kb.optim.Adam, 2 more steps: the bits of 5 uninterrupted steps.

    The same resume into torch.optim.Adam.  Its first resumed step runs on bit-equal gradients (asserted), so there p, m and v
    are held to all three sequence gates.  After the second step p is held to its gate, TOL_P x the lr of the two resumed steps:
    moments restarted from zero, or a step count restarted from 1, move p by the order of lr itself.  m and v after the second step
    are printed, not asserted: its gradients come from parameters that already differ in their last bit, and the network carries
    that to 3.0e-5 (m) and 1.3e-5 (v) of |b| + rms(b) on the MI355X -- the ill-conditioning of a trajectory through the network, which a
    gate would have to be widened for until it hid mistakes of the optimizer's."""
    depth, pose = _models(dev)
    opt = kb.optim.Adam(_groups(depth, pose), lr=LR)
    paths = str(tmp_path / "depth.pth"), str(tmp_path / "pose.pth")
    for step in range(5):
        if step == 3:
            depth.save_model(paths[0], step, opt)
            pose.save_model(paths[1], step, opt)
        _train_step(dev, depth, pose, opt)
        if step == 3:
            after4 = [p.detach().clone() for p in _all_params(depth, pose)], _state_of(opt, _all_params(depth, pose)), \
                [None if p.grad is None else p.grad.clone() for p in _all_params(depth, pose)]
    want = [p.detach() for p in _all_params(depth, pose)]
    for cls, kwargs in ((kb.optim.Adam, {}), (torch.optim.Adam, {"foreach": False})):
        d2, p2 = _models(dev)
        for p in _all_params(d2, p2):
            p.data.add_(1.0)                                   # restore_model has to bring the weights back
        opt2 = cls(_groups(d2, p2), lr=1.0, **kwargs)
        assert d2.restore_model(paths[0], opt2) == (3, opt2)
        assert p2.restore_model(paths[1], opt2) == (3, opt2)
        assert opt2.param_groups[0]["lr"] == LR and [g["weight_decay"] for g in opt2.param_groups] == [WD_DEPTH, WD_POSE]
        assert all(float(s["step"]) == 3 for s in opt2.state.values()) and len(opt2.state) == len(opt.state)
        params2 = _all_params(d2, p2)
        _train_step(dev, d2, p2, opt2)
        if cls is torch.optim.Adam:
            fp, fm, fv = [], [], []
            for x, p4, s4, g4 in zip(params2, *after4):
                assert (x.grad is None) == (g4 is None) and (g4 is None or torch.equal(x.grad, g4))
                fp.append(ao.p_fraction(x.detach(), p4, LR))
                if s4 is not None:
                    fm.append(ao.fraction(opt2.state[x]["exp_avg"], s4[0]))
                    fv.append(ao.fraction(opt2.state[x]["exp_avg_sq"], s4[1]))
            print(f"resume into torch.optim.Adam, first step (same gradients): p {max(fp):.2e} of lr (gate {ao.TOL_P:.0e}), m {max(fm):.2e} "
                  f"(gate {ao.TOL_M:.0e}), v {max(fv):.2e} (gate {ao.TOL_V:.0e})")
            assert max(fp) <= ao.TOL_P and max(fm) <= ao.TOL_M and max(fv) <= ao.TOL_V
        _train_step(dev, d2, p2, opt2)
        got = [p.detach() for p in params2]
        pairs = [(a, b) for a, b in zip(params2, _all_params(depth, pose)) if b in opt.state]
        if cls is kb.optim.Adam:
            assert all(torch.equal(a, b) for a, b in zip(got, want))
            assert all(torch.equal(a, b) for a, b in zip(_buffers(d2, p2), _buffers(depth, pose)))
            assert all(torch.equal(opt2.state[a][k], opt.state[b][k]) for a, b in pairs for k in ("exp_avg", "exp_avg_sq"))
            assert all(float(opt2.state[a]["step"]) == 5 for a, _ in pairs)
        else:
            fp = max(ao.p_fraction(a, b, 2 * LR) for a, b in zip(got, want))
            fm = max(ao.fraction(opt2.state[a]["exp_avg"], opt.state[b]["exp_avg"]) for a, b in pairs)
            fv = max(ao.fraction(opt2.state[a]["exp_avg_sq"], opt.state[b]["exp_avg_sq"]) for a, b in pairs)
            print(f"resume into torch.optim.Adam, second step: p {fp:.2e} of the resumed lr (gate {ao.TOL_P:.0e}); through the network's "
                  f"gradients: m {fm:.2e}, v {fv:.2e}")
            assert fp <= ao.TOL_P
