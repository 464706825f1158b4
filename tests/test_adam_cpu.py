"""CPU: the Adam oracle against the reference's optimizer class, the gates measured where they come from, the power of the gates, and
the host logic of kb.optim.Adam and restore_model(path, optimizer) -- no GPU needed (the step itself is tests/test_adam_gpu.py).

    python -m pytest tests/test_adam_cpu.py -q
"""
import copy
import math
import os
import re

import pytest
import torch

import kbnet_amd as kb
import adam_oracle as ao

KbnError = kb._lib.KbnError
HERE = os.path.dirname(os.path.abspath(__file__))
CKPT = os.path.join(HERE, "golden", "ckpt_kitti_narrow.pth")


def _torch_adam(groups):
    return torch.optim.Adam(groups, foreach=False)


def _mixed_sequence(dtype=torch.float32, steps=8):
    """Three parameters in two groups (their own weight decay and lr schedule); the second has no gradient on steps 2, 3 and 6, the
    third never has one."""
    gen = torch.Generator().manual_seed(7)
    p0 = [torch.randn(n, generator=gen, dtype=torch.float64).to(dtype) * 0.1 for n in (1001, 77, 5)]
    grads = []
    for t in range(steps):
        grads.append([torch.randn(1001, generator=gen, dtype=torch.float64).to(dtype),
                      None if t in (2, 3, 6) else torch.randn(77, generator=gen, dtype=torch.float64).to(dtype), None])
    groups = [{"params": [0], "lr": [1e-3] * 4 + [5e-4] * (steps - 4), "weight_decay": 1e-4},
              {"params": [1, 2], "lr": [2e-3] * 4 + [1e-3] * (steps - 4), "weight_decay": 1e-2, "betas": (0.8, 0.99), "eps": 1e-6}]
    return p0, grads, groups


def test_the_fp64_oracle_is_torchs_adam():
    """adam_oracle.adam in fp64 = torch.optim.Adam(foreach=False) in fp64 on the CPU, the class reference src/kbnet.py:360 constructs,
    to 1e-15 of each tensor's largest element: gradient sequence, lr change, two groups, a parameter without a gradient on some
    steps and one that never has one."""
    p0, grads, groups = _mixed_sequence(torch.float64)
    ours = ao.adam(p0, grads, groups, torch.float64)
    ref = ao.run_optimizer(_torch_adam, p0, grads, groups, dtype=torch.float64)
    assert ours["step"] == ref["step"] == [8, 5, 0]
    assert ours["m"][2] is None and ref["m"][2] is None and torch.equal(ours["p"][2], p0[2])
    for key in ("p", "m", "v"):
        for a, b in zip(ours[key][:2], ref[key][:2]):
            assert float((a - b).abs().max()) <= 1e-15 * float(b.abs().max()), key
    for name in ao.CASES:
        p0, grads, groups = ao.case(name)
        ref = ao.run_optimizer(_torch_adam, p0, grads, groups, dtype=torch.float64)
        want = ao.case_reference(name)
        for key in ("p", "m", "v"):
            assert float((want[key][0] - ref[key][0]).abs().max()) <= 1e-15 * float(ref[key][0].abs().max()), (name, key)


def _round_up_one_digit(x):
    e = math.floor(math.log10(x))
    return math.ceil(x / 10 ** e - 1e-9) * 10 ** e


def test_the_gates_are_three_times_torchs_own_fp32_distance():
    """The rule of DESIGN section 8e: torch's fp32 Adam (CPU, foreach=False) against the fp64 run on the same fp32 gradients, the worst of
    the four cases, x 3, rounded up to one digit -- printed, and the constants of adam_oracle asserted to be that: no smaller than
    3 x the distance and less than the factor 2 above it that rounding up one digit can add."""
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for name in ao.CASES:
        p0, grads, groups = ao.case(name)
        assert len(grads) == 20 and p0[0].numel() == 40003
        kind = ao.CASES[name][0]
        g = torch.stack([s[0] for s in grads])
        if kind == "scaled":
            assert bool((g[:, ::7] == 0).all()) and float(g.abs().max()) > 100
        nz = g[g != 0].double()
        assert float((1e-3 * nz * nz).min()) > 1.2e-38 * 1e3     # (1 - beta2) g^2 well inside the normal range
        got = ao.run_optimizer(_torch_adam, p0, grads, groups)
        want = ao.case_reference(name)
        lr_sum = sum(ao.lr_schedule())
        fig = {"p": ao.p_fraction(got["p"][0], want["p"][0], lr_sum), "m": ao.fraction(got["m"][0], want["m"][0]),
               "v": ao.fraction(got["v"][0], want["v"][0])}
        print(f"{name}: torch fp32 vs fp64: p {fig['p']:.2e} of sum lr, m {fig['m']:.2e}, v {fig['v']:.2e}")
        for k in worst:
            worst[k] = max(worst[k], fig[k])
    assert abs(sum(ao.lr_schedule()) - 1.5e-3) < 1e-12
    for k, const in (("p", ao.TOL_P), ("m", ao.TOL_M), ("v", ao.TOL_V)):
        rule = _round_up_one_digit(3 * worst[k])
        print(f"{k}: worst {worst[k]:.2e}, 3 x rounded up {rule:.0e}, constant {const:.0e}")
        assert 3 * worst[k] <= const <= 2 * 3 * worst[k], (k, worst[k], rule, const)    # (rounding up to one digit at most doubles)


def _power_sequence():
    """The mixed sequence at the gate cases' scale: 20 steps, the scaled gradients (small elements are where weight decay and eps
    act), two groups with their own decay, lr halved after step 10, the second parameter without a gradient on five steps."""
    gen = torch.Generator().manual_seed(11)
    n = 4001
    p0 = [(0.1 * torch.randn(n, generator=gen, dtype=torch.float64)).float() for _ in range(2)]
    grads = [[ao.gradient("scaled", n, gen), None if t in (1, 2, 3, 8, 9) else ao.gradient("scaled", n, gen)] for t in range(20)]
    groups = [{"params": [0], "lr": ao.lr_schedule(), "weight_decay": 1e-4}, {"params": [1], "lr": ao.lr_schedule(), "weight_decay": 1e-2}]
    return p0, grads, groups


_POWER = {}


def _power_reference():
    if not _POWER:
        p0, grads, groups = _power_sequence()
        _POWER["args"] = (p0, grads, groups)
        _POWER["want"] = ao.adam(p0, grads, groups, torch.float64)
    return _POWER["args"], _POWER["want"]


# the quantity each planted mistake must push out of its gate by more than 10 x, and the parameter it shows on
@pytest.mark.parametrize("mistake, quantity, index", [
    ("no_bias_correction2", "p", 0), ("eps_inside_sqrt", "p", 0), ("decoupled_weight_decay", "p", 0), ("group0_weight_decay", "p", 1),
    ("step_without_gradient", "p", 1), ("m_from_raw_gradient", "p", 0), ("lr_change_ignored", "p", 0)])
def test_a_planted_mistake_leaves_the_gate_by_ten_times(mistake, quantity, index):
    (p0, grads, groups), want = _power_reference()
    got = ao.adam(p0, grads, groups, torch.float64, mistake=mistake)
    lr_sum = sum(ao.lr_schedule())
    fig = {"p": ao.p_fraction(got["p"][index], want["p"][index], lr_sum) / ao.TOL_P,
           "m": ao.fraction(got["m"][index], want["m"][index]) / ao.TOL_M,
           "v": ao.fraction(got["v"][index], want["v"][index]) / ao.TOL_V}
    print(f"{mistake}: parameter {index}: p at {fig['p']:.1f} x its gate, m {fig['m']:.1f} x, v {fig['v']:.1f} x")
    assert fig[quantity] > 10, (mistake, fig)
    clean = ao.adam(p0, grads, groups, torch.float64)
    assert all(torch.equal(a, b) for a, b in zip(clean["p"], want["p"]))     # the reference is left unchanged, and reproducible


# ---------------------------------------------------------------------------------------------- host logic
def _params(n=2, device="cpu"):
    return [torch.nn.Parameter(torch.randn(4, 3, device=device)) for _ in range(n)]


@pytest.mark.parametrize("option, value", [("amsgrad", True), ("maximize", True), ("capturable", True), ("differentiable", True),
                                           ("decoupled_weight_decay", True), ("foreach", True), ("fused", True)])
def test_refused_options_raise_with_their_name(option, value):
    with pytest.raises(ValueError, match=option):
        kb.optim.Adam(_params(), **{option: value})
    with pytest.raises(ValueError, match=option):                      # in a group of its own
        kb.optim.Adam([{"params": _params(1)}, {"params": _params(1), option: value}])
    opt = kb.optim.Adam(_params())                                      # arriving later, as through load_state_dict
    opt.param_groups[0][option] = value
    with pytest.raises(ValueError, match=option):
        opt.step()
    sd = torch.optim.Adam(_params()).state_dict()
    sd["param_groups"][0][option] = value
    opt = kb.optim.Adam(_params())
    opt.load_state_dict(sd)
    with pytest.raises(ValueError, match=option):
        opt.step()


def test_a_tensor_lr_and_a_closure_are_refused():
    with pytest.raises(ValueError, match="tensor lr"):
        kb.optim.Adam(_params(), lr=torch.tensor(1e-3))
    opt = kb.optim.Adam(_params())
    opt.param_groups[0]["lr"] = torch.tensor(1e-3)
    with pytest.raises(ValueError, match="tensor lr"):
        opt.step()
    with pytest.raises(ValueError, match="closure"):
        kb.optim.Adam(_params()).step(lambda: 0.0)
    for bad in ({"lr": -1.0}, {"eps": -1.0}, {"betas": (1.0, 0.9)}, {"weight_decay": -1.0}):
        with pytest.raises(ValueError):
            kb.optim.Adam(_params(), **bad)


def test_cpu_parameters_raise_on_step():
    params = _params()
    opt = kb.optim.Adam(params)
    opt.step()                                   # no gradients: nothing to do, no state
    assert len(opt.state) == 0
    for p in params:
        p.grad = torch.ones_like(p)
    before = [p.detach().clone() for p in params]
    with pytest.raises(KbnError, match="no CPU fallback"):
        opt.step()
    assert all(torch.equal(a, b) for a, b in zip(before, params))
    assert all(float(opt.state[p]["step"]) == 0 for p in params if p in opt.state)
    with pytest.raises(KbnError):
        kb.ops.adam_step(params, [p.grad for p in params], [torch.zeros_like(p) for p in params], [torch.zeros_like(p) for p in params],
                         [1, 1], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0)
    with pytest.raises(KbnError, match="one length"):
        kb.ops.adam_step(params, [], [], [], [], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0)


def test_keys_are_torchs_in_torchs_order():
    ours, theirs = kb.optim.Adam(_params(), lr=3e-4, weight_decay=1e-4), torch.optim.Adam(_params(), lr=3e-4, weight_decay=1e-4)
    assert list(ours.defaults) == list(theirs.defaults) and ours.defaults == theirs.defaults
    assert [list(g) for g in ours.param_groups] == [list(g) for g in theirs.param_groups]
    a, b = ours.state_dict(), theirs.state_dict()
    assert set(a) == set(b) and [set(g) for g in a["param_groups"]] == [set(g) for g in b["param_groups"]]
    assert kb.optim.Adam is kb.optim.Adam.__mro__[0] and issubclass(kb.optim.Adam, torch.optim.Optimizer)
    # the reference's construction: two groups with their own weight decay, lr written through param_groups
    opt = kb.optim.Adam([{"params": _params(1), "weight_decay": 0.0}, {"params": _params(1), "weight_decay": 1e-4}], lr=1e-4)
    for g in opt.param_groups:
        g["lr"] = 5e-5
    assert [g["weight_decay"] for g in opt.param_groups] == [0.0, 1e-4] and all(g["lr"] == 5e-5 for g in opt.param_groups)


def _stepped_torch_adam(params, steps=3):
    opt = torch.optim.Adam([{"params": params[:1], "weight_decay": 1e-4}, {"params": params[1:], "weight_decay": 0.0}], lr=1e-4)
    for _ in range(steps):
        for p in params:
            p.grad = torch.randn_like(p)
        opt.step()
    return opt


def test_state_dicts_load_both_ways():
    torch.manual_seed(0)
    params = _params(3)
    theirs = _stepped_torch_adam(params)
    ours = kb.optim.Adam([{"params": params[:1]}, {"params": params[1:]}])
    ours.load_state_dict(theirs.state_dict())
    assert [g["weight_decay"] for g in ours.param_groups] == [1e-4, 0.0] and ours.param_groups[0]["lr"] == 1e-4
    for p in params:
        s, t = ours.state[p], theirs.state[p]
        assert set(s) == set(t) == {"step", "exp_avg", "exp_avg_sq"}
        assert float(s["step"]) == 3 and s["step"].dtype == torch.float32 and not s["step"].is_cuda
        assert torch.equal(s["exp_avg"], t["exp_avg"]) and torch.equal(s["exp_avg_sq"], t["exp_avg_sq"])
    back = torch.optim.Adam([{"params": params[:1]}, {"params": params[1:]}])
    back.load_state_dict(ours.state_dict())
    for p in params:
        assert torch.equal(back.state[p]["exp_avg_sq"], theirs.state[p]["exp_avg_sq"]) and float(back.state[p]["step"]) == 3
    for p in params:
        p.grad = torch.randn_like(p)
    back.step()                                   # torch steps on the state that went through ours
    assert all(float(back.state[p]["step"]) == 4 for p in params)
    # a state dict of an older torch: step as a Python number, the newer group keys missing
    old = copy.deepcopy(theirs.state_dict())     # (state_dict() hands out the live per-parameter dicts)
    for s in old["state"].values():
        s["step"] = int(s["step"])
    for g in old["param_groups"]:
        for k in ("maximize", "foreach", "capturable", "differentiable", "fused", "decoupled_weight_decay"):
            del g[k]
    ours = kb.optim.Adam([{"params": params[:1]}, {"params": params[1:]}])
    ours.load_state_dict(old)
    # (load_state_dict keeps tensors that need no cast, so `back`'s step above advanced the shared state to 4)
    assert all(torch.is_tensor(ours.state[p]["step"]) and float(ours.state[p]["step"]) == float(theirs.state[p]["step"]) == 4 for p in params)
    assert [set(g) for g in ours.param_groups] == [set(g) for g in theirs.param_groups]


def _narrow_kitti(device=torch.device("cpu")):
    return kb.modules.KBNetModel.from_config(kb.kitti_config().narrow(), device)


def test_both_optimizers_load_the_shipped_checkpoints_optimizer_state():
    state = torch.load(CKPT, map_location="cpu")["optimizer_state_dict"]
    assert state and len(state["param_groups"]) == 1
    for cls in (kb.optim.Adam, torch.optim.Adam):
        model = _narrow_kitti()
        params = model.parameters()
        assert len(params) == len(state["param_groups"][0]["params"])
        opt = cls(params, lr=1.0)
        opt.load_state_dict(state)
        assert opt.param_groups[0]["lr"] == state["param_groups"][0]["lr"] != 1.0
        assert len(opt.state) == len(state["state"])
        step, opt2 = model.restore_model(CKPT, cls(params, lr=1.0))
        assert opt2.param_groups[0]["lr"] == state["param_groups"][0]["lr"]
        assert step == torch.load(CKPT, map_location="cpu")["train_step"]


def _pose(device=torch.device("cpu")):
    return kb.posenet_resnet.ResNetPoseNetModel(n_layer=18, device=device, n_filters=[8, 8, 16, 16, 32], decoder_filters=[16, 16])


@pytest.mark.parametrize("kind", ["depth", "pose"])
def test_restore_model_brings_the_optimizer_back(kind, tmp_path):
    torch.manual_seed(1)
    make = _narrow_kitti if kind == "depth" else _pose
    model = make()
    params = [p for p in model.parameters()]
    for p in params:
        p.requires_grad_(True)
    saved = _stepped_torch_adam(params)
    path = str(tmp_path / "model.pth")
    model.save_model(path, 12, saved)
    fresh = make()
    fparams = fresh.parameters()
    opt = torch.optim.Adam([{"params": fparams[:1]}, {"params": fparams[1:]}], lr=1.0)
    step, returned = fresh.restore_model(path, opt)
    assert step == 12 and returned is opt
    assert opt.param_groups[0]["lr"] == 1e-4 and opt.param_groups[0]["weight_decay"] == 1e-4
    for p, q in zip(params, fparams):
        assert torch.equal(p.detach(), q.detach())
        assert float(opt.state[q]["step"]) == 3
        assert torch.equal(opt.state[q]["exp_avg"], saved.state[p]["exp_avg"])
        assert torch.equal(opt.state[q]["exp_avg_sq"], saved.state[p]["exp_avg_sq"])
    ours = kb.optim.Adam([{"params": fparams[:1]}, {"params": fparams[1:]}], lr=1.0)
    fresh.restore_model(path, ours)
    assert all(torch.equal(ours.state[q]["exp_avg"], saved.state[p]["exp_avg"]) for p, q in zip(params, fparams))
    assert fresh.restore_model(path) == (12, None)            # without an optimizer: as before
    # an empty dict (save_model without an optimizer) leaves the optimizer alone
    empty = str(tmp_path / "empty.pth")
    model.save_model(empty, 5)
    assert torch.load(empty, map_location="cpu")["optimizer_state_dict"] == {}
    before = {q: {k: v.clone() for k, v in opt.state[q].items()} for q in fparams}
    step, returned = fresh.restore_model(empty, opt)
    assert step == 5 and returned is opt and opt.param_groups[0]["lr"] == 1e-4
    assert all(torch.equal(opt.state[q][k], v) for q in fparams for k, v in before[q].items())
    # a dict that does not fit raises: the reference's silent `except: pass` is not copied
    wrong = torch.optim.Adam(fparams[:2], lr=1.0)
    with pytest.raises(ValueError):
        fresh.restore_model(path, wrong)


def test_binding_constants_are_the_headers():
    header = open(os.path.join(os.path.dirname(HERE), "include", "kbnet_hip.h")).read()
    for name in ("KBN_ADAM_TABLE_CAPACITY", "KBN_ADAM_PASS_ELEMENTS"):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == getattr(kb._lib, name)
    assert kb.ops.ADAM_TABLE_CAPACITY == kb._lib.KBN_ADAM_TABLE_CAPACITY and kb.ops.ADAM_PASS_ELEMENTS == kb._lib.KBN_ADAM_PASS_ELEMENTS
    import ctypes
    assert ctypes.sizeof(kb._lib.AdamTensor) == kb.ops._ADAM_RECORD.size == 72      # the wrapper packs records with struct, field by field
