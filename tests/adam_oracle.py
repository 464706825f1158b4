"""Adam as the reference trains with it (torch.optim.Adam: L2 weight decay, no amsgrad; reference src/kbnet.py:360-369), restated in
plain tensor arithmetic of any dtype -- the fp64 run is what csrc/adam.hip and kb.optim.Adam are tested against -- with the gates,
their cases, and the planted mistakes that show the gates can see (tests/test_adam_cpu.py).

Per element and step, for a parameter that has a gradient at that step (one that has none is left alone, its step count too):
    t  = t + 1
    g' = g + wd * p                      (skipped when wd == 0)
    m  = m + (1 - beta1) * (g' - m)
    v  = beta2 * v + (1 - beta2) * g' * g'
    p  = p - step_size * m / (sqrt(v) / bc2_sqrt + eps),   step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t)

GATES (the section 8e rule: 3 x the distance of torch's own fp32 Adam on the CPU, foreach=False, from the fp64
run on the same fp32 gradients, worst of the four CASES, rounded up to one digit; test_adam_cpu measures and asserts them):
    m, v   |a - b| <= TOL (|b| + rms(b)) per tensor, elementwise
    p      max |a - b| <= TOL_P * sum_t lr_t: the error against the most any element can move (|m| / sqrt(v) is of order 1), so a
           dropped or doubled step is of order 1 / T on that scale
"""
import math

import torch

TOL_M = 1e-6
TOL_V = 2e-6
TOL_P = 3e-4

MISTAKES = ("no_bias_correction2", "eps_inside_sqrt", "decoupled_weight_decay", "group0_weight_decay", "step_without_gradient",
            "m_from_raw_gradient", "lr_change_ignored")


def lr_at(group, t):
    """The group's learning rate at (0-based) step t: `lr` is a number or one number per step."""
    lr = group["lr"]
    return float(lr[t]) if isinstance(lr, (list, tuple)) else float(lr)


def adam(p, grads_sequence, groups, dtype, mistake=None):
    """p: list of tensors.  grads_sequence[t][i]: the gradient of p[i] at step t, or None.  groups: dicts with 'params' (indices
    into p), 'lr' (a number, or one per step: the schedule writes it into param_groups between steps), 'weight_decay' and
    optionally 'betas', 'eps'.  Returns {'p', 'm', 'v', 'step'}: lists over the parameters (m, v None and step 0 for one that never
    had a gradient).  `mistake`: one of MISTAKES, planted for the power tests."""
    assert mistake is None or mistake in MISTAKES, mistake
    p = [x.detach().to(dtype).clone() for x in p]
    m, v, step = [None] * len(p), [None] * len(p), [0] * len(p)
    for t, grads in enumerate(grads_sequence):
        for group in groups:
            beta1, beta2 = group.get("betas", (0.9, 0.999))
            eps = group.get("eps", 1e-8)
            wd = groups[0]["weight_decay"] if mistake == "group0_weight_decay" else group["weight_decay"]
            lr = lr_at(group, 0 if mistake == "lr_change_ignored" else t)
            for i in group["params"]:
                if grads[i] is None:
                    if mistake == "step_without_gradient":
                        step[i] += 1
                    continue
                g_raw = grads[i].to(dtype)
                if m[i] is None:
                    m[i], v[i] = torch.zeros_like(p[i]), torch.zeros_like(p[i])
                step[i] += 1
                g = g_raw
                if wd != 0:
                    if mistake == "decoupled_weight_decay":
                        p[i] = p[i] * (1 - lr * wd)
                    else:
                        g = g_raw + wd * p[i]
                m[i] = m[i] + (1 - beta1) * ((g_raw if mistake == "m_from_raw_gradient" else g) - m[i])
                v[i] = beta2 * v[i] + (1 - beta2) * g * g
                step_size = lr / (1 - beta1 ** step[i])
                bc2_sqrt = 1.0 if mistake == "no_bias_correction2" else math.sqrt(1 - beta2 ** step[i])
                if mistake == "eps_inside_sqrt":
                    denom = torch.sqrt(v[i] / bc2_sqrt ** 2 + eps)
                else:
                    denom = torch.sqrt(v[i]) / bc2_sqrt + eps
                p[i] = p[i] - step_size * m[i] / denom
    return {"p": p, "m": m, "v": v, "step": step}


U = 2.0 ** -24    # fp32 unit roundoff


def one_step(p, g, m, v, t, lr, betas, eps, wd):
    """One step of the formula in fp64 on fp32 inputs, with a bound on what an fp32 evaluation in the stated order may differ by
    (fused multiply-adds only remove roundings): (p', m', v', dp, dm, dv), all fp64 CPU tensors.  Every scalar (wd, 1 - beta1,
    beta2, 1 - beta2, step_size, bc2_sqrt, eps) reaches the kernel rounded to fp32: one relative U each.  With G = |g| + wd |p|:
        g' = fl(g + fl(wd p))                  3 roundings on terms <= G                 dg <= 3 U G        (0 without decay)
        m' = fl(m + fl(c1 fl(g' - m)))         c1 dg + 3 U c1 (G + |m|) + U |m'|         dm <= 8 U (|m| + c1 (G + |m|))
        v' = fl(fl(b2 v) + fl(fl(c2 g') g'))   2 U b2 v + 3 U c2 G^2 + 2 c2 G dg + U v'  dv <= 10 U (b2 v + c2 G^2)
        s  = fl(sqrt(v'))                      |sqrt a - sqrt b| <= min(|a - b| / sqrt b, sqrt |a - b|), + U s
        d  = fl(fl(s / bc2) + eps)             ds / bc2 + 2 U s / bc2 + U eps + U d      dd <= ds / bc2 + 3 U d
        u  = fl(fl(step_size m') / d)          3 U |u| + step_size dm / d + |u| dd / (d - dd)
        p' = fl(p - u)                         du + U |p'|
    second-order terms are covered by the factor 1.01 on the whole."""
    p, g, m, v = (x.detach().double().cpu() for x in (p, g, m, v))
    beta1, beta2 = betas
    c1, c2 = 1 - beta1, 1 - beta2
    gp = g + wd * p if wd != 0 else g
    G = g.abs() + wd * p.abs()
    dg = 3 * U * G if wd != 0 else torch.zeros_like(G)
    m2 = m + c1 * (gp - m)
    dm = 8 * U * (m.abs() + c1 * (G + m.abs()))
    v2 = beta2 * v + c2 * gp * gp
    dv = 10 * U * (beta2 * v + c2 * G * G)
    step_size = lr / (1 - beta1 ** t)
    bc2_sqrt = math.sqrt(1 - beta2 ** t)
    s = torch.sqrt(v2)
    ds = torch.minimum(dv / s.clamp_min(1e-300), dv.sqrt()) + U * (s + dv.sqrt())
    d = s / bc2_sqrt + eps
    dd = ds / bc2_sqrt + 3 * U * d
    upd = step_size * m2 / d
    du = 3 * U * upd.abs() + step_size * dm / d + upd.abs() * dd / (d - dd).clamp_min(1e-300)
    p2 = p - upd
    dp = du + U * p2.abs()
    return p2, m2, v2, 1.01 * dp, 1.01 * dm, 1.01 * dv


def fraction(a, b):
    """max |a - b| / (|b| + rms(b)): the m, v gate's left side (0 for an all-zero pair)."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    scale = b.abs() + b.pow(2).mean().sqrt()
    err = (a - b).abs()
    if not bool(torch.isfinite(err).all()):
        return float("inf")
    return float((err / scale.clamp_min(1e-300)).max()) if err.numel() else 0.0


def p_fraction(a, b, lr_sum):
    """max |a - b| / sum_t lr_t: the p gate's left side."""
    err = (a.detach().double().cpu() - b.detach().double().cpu()).abs()
    if not bool(torch.isfinite(err).all()):
        return float("inf")
    return float(err.max()) / lr_sum if err.numel() else 0.0


# ---- the gate cases: 20 steps, 40 003 elements, p0 ~ 0.1 N(0, 1), lr 1e-4 halved after step 10
STEPS, NUMEL, LR = 20, 40003, 1e-4
CASES = {"normal_wd0": ("normal", 0.0), "normal_wd1e-4": ("normal", 1e-4), "scaled_wd0": ("scaled", 0.0), "scaled_wd1e-4": ("scaled", 1e-4)}


def lr_schedule(steps=STEPS, lr=LR):
    return [lr if t < steps // 2 else lr / 2 for t in range(steps)]


def gradient(kind, numel, gen):
    """'normal': N(0, 1).  'scaled': N(0, 1) * 10^U(-12, 3) with every seventh element exactly zero.  |N| is kept above 0.01, so that
    (1 - beta2) g^2 >= 1e-31 stays a normal fp32 number: the gates do not rest on how denormals are handled."""
    n = torch.randn(numel, generator=gen, dtype=torch.float64)
    n = torch.where(n.abs() < 0.01, torch.where(n < 0, -0.01, 0.01).double(), n)
    if kind == "scaled":
        n = n * 10 ** (torch.rand(numel, generator=gen, dtype=torch.float64) * 15 - 12)
        n[::7] = 0
    return n.float()


def case(name):
    """(p0, grads_sequence, groups) of a gate case: fp32 tensors from a fixed seed."""
    kind, wd = CASES[name]
    gen = torch.Generator().manual_seed(1000 + list(CASES).index(name))
    p0 = (0.1 * torch.randn(NUMEL, generator=gen, dtype=torch.float64)).float()
    grads = [[gradient(kind, NUMEL, gen)] for _ in range(STEPS)]
    return [p0], grads, [{"params": [0], "lr": lr_schedule(), "weight_decay": wd}]


_REFERENCE = {}


def case_reference(name):
    """The fp64 run of a gate case, computed once and shared (callers do not modify it)."""
    if name not in _REFERENCE:
        p0, grads, groups = case(name)
        _REFERENCE[name] = adam(p0, grads, groups, torch.float64)
    return _REFERENCE[name]


def run_optimizer(make, p0, grads_sequence, groups, device="cpu", dtype=torch.float32):
    """The same sequence through an optimizer class: make(param_groups) -> optimizer.  Returns what adam() returns."""
    params = [torch.nn.Parameter(x.detach().to(device=device, dtype=dtype).clone()) for x in p0]
    opt = make([{"params": [params[i] for i in g["params"]], "lr": lr_at(g, 0), "weight_decay": g["weight_decay"],
                 "betas": g.get("betas", (0.9, 0.999)), "eps": g.get("eps", 1e-8)} for g in groups])
    for t, grads in enumerate(grads_sequence):
        for g, pg in zip(groups, opt.param_groups):
            pg["lr"] = lr_at(g, t)
        for x, gr in zip(params, grads):
            x.grad = None if gr is None else gr.detach().to(device=device, dtype=dtype).clone()
        opt.step()
    state = [opt.state.get(x, {}) for x in params]
    return {"p": [x.detach() for x in params], "m": [s.get("exp_avg") for s in state], "v": [s.get("exp_avg_sq") for s in state],
            "step": [int(s["step"]) if s else 0 for s in state], "optimizer": opt, "params": params}
