"""fp64 restatement, in plain torch and WITHOUT autograd, of BatchNorm on the statistics of a batch that is spread over several
ranks (csrc/bn_sync.hip, ops.batch_norm_act_sync): the yardstick of tests/test_bn_sync_cpu.py, which holds it to fp64 autograd of
the whole batch, and of the GPU tests.

Convention (GradientAverager's): rank r holds n_r of the n frames, its loss L_r is the mean over its own frames, the global loss
is sum_r (n_r / n) L_r.  c_r = n_r H W, M = sum c_r.

    forward    record_r = (c_r, mean_r, q_r = sum (u - mean_r)^2);   merged pairwise in rank order:
               d = m_B - m_A;  m = m_A + d c_B / (c_A + c_B);  q = q_A + q_B + d^2 c_A c_B / (c_A + c_B)
               mean, var = q / M (normalises), q / (M - 1) (the running variance)
    backward   s_r = (sum g_z, sum g_z xhat) over the rank's frames;   S = sum_r (c_r / M) s_r
               grad_u = scale (g_z - (S1 + xhat S2) / c_r);   grad_gamma, grad_beta = the rank's own s_r

The keyword arguments are the MISTAKES the test plants to prove that the gate sees them; their defaults are the algebra.
"""
import torch

MOMENTUM = 0.1


def moments(u):
    """(c_r, mean_r[C], q_r[C]) of one shard, two passes."""
    n, _, h, w = u.shape
    mean = u.mean(dim=(0, 2, 3))
    q = (u - mean.view(1, -1, 1, 1)).pow(2).sum(dim=(0, 2, 3))
    return float(n * h * w), mean, q


def merge(records):
    """-> (M, mean, biased variance, unbiased variance) of the shards' records, merged in the order given."""
    cnt, m, q = records[0]
    for cb, mb, qb in records[1:]:
        tot = cnt + cb
        d = mb - m
        m = m + d * cb / tot
        q = q + qb + d * d * cnt * cb / tot
        cnt = tot
    return cnt, m, q / cnt, q / (cnt - 1.0)


def _parts(u, grad_y, gamma, beta, mean, var, eps, slope):
    """(scale, g_z, xhat) of one shard on the given statistics; z <= 0 takes the slope, as torch's leaky_relu at 0."""
    rstd = torch.rsqrt(var + eps)
    scale = (gamma * rstd).view(1, -1, 1, 1)
    xhat = (u - mean.view(1, -1, 1, 1)) * rstd.view(1, -1, 1, 1)
    z = xhat * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)
    gz = grad_y if slope is None else torch.where(z > 0, grad_y, slope * grad_y)
    return scale, gz, xhat, z


def forward(shards_u, gamma, beta, eps, slope):
    """-> (the shards' outputs, M, mean, biased variance, unbiased variance)."""
    M, mean, var, unbiased = merge([moments(u) for u in shards_u])
    ys = []
    for u in shards_u:
        _, _, _, z = _parts(u, u, gamma, beta, mean, var, eps, slope)
        ys.append(z if slope is None else torch.where(z > 0, z, slope * z))
    return ys, M, mean, var, unbiased


def backward(shards_u, shards_grad_y, gamma, beta, eps, slope, global_divisor=False, unweighted=False):
    """-> (grad_u, grad_gamma, grad_beta), a list over the shards each, in the units of the shards' own losses.
    `global_divisor`: M in place of the rank's own count c_r under the two sums.  `unweighted`: S = sum_r s_r."""
    records = [moments(u) for u in shards_u]
    M, mean, var, _ = merge(records)
    parts = [_parts(u, g, gamma, beta, mean, var, eps, slope) for u, g in zip(shards_u, shards_grad_y)]
    s1 = [gz.sum(dim=(0, 2, 3)) for _, gz, _, _ in parts]
    s2 = [(gz * xhat).sum(dim=(0, 2, 3)) for _, gz, xhat, _ in parts]
    S1, S2 = torch.zeros_like(s1[0]), torch.zeros_like(s2[0])
    for (cr, _, _), a, b in zip(records, s1, s2):
        weight = 1.0 if unweighted else cr / M
        S1, S2 = S1 + weight * a, S2 + weight * b
    grad_u = []
    for (cr, _, _), (scale, gz, xhat, _) in zip(records, parts):
        div = M if global_divisor else cr
        grad_u.append(scale * (gz - (S1.view(1, -1, 1, 1) + xhat * S2.view(1, -1, 1, 1)) / div))
    return grad_u, s2, s1


def running_update(running_mean, running_var, shards_u, biased_running_var=False):
    """The running statistics after one forward over the shards.  `biased_running_var`: q / M where q / (M - 1) belongs."""
    _, mean, var, unbiased = merge([moments(u) for u in shards_u])
    return ((1 - MOMENTUM) * running_mean + MOMENTUM * mean,
            (1 - MOMENTUM) * running_var + MOMENTUM * (var if biased_running_var else unbiased))


def split(t, sizes):
    assert sum(sizes) == t.shape[0]
    return list(torch.split(t, list(sizes), dim=0))


def shard_cotangents(grad_y, sizes):
    """The whole batch's cotangent as the shards' own: shard r's scaled n / n_r, so that sum_r (n_r / n) L_r is the whole's loss."""
    n = grad_y.shape[0]
    return [g * (n / s) for g, s in zip(split(grad_y, sizes), sizes)]


def reassemble(grad_u, grad_gamma, grad_beta, sizes):
    """What GradientAverager's n_r / n weights make of the shards' results -> (grad_u of the whole batch, grad_gamma, grad_beta)."""
    n = float(sum(sizes))
    gu = torch.cat([g * (s / n) for g, s in zip(grad_u, sizes)], dim=0)
    gg = sum(g * (s / n) for g, s in zip(grad_gamma, sizes))
    gb = sum(g * (s / n) for g, s in zip(grad_beta, sizes))
    return gu, gg, gb
