"""What the ranks of tests/test_grad_average_gpu.py run, each in a process of its own:

    python tests/grad_average_ranks.py <backend> <rank> <world> <port> <out_dir> <scenario> [<scenario> ...]

backend "gloo": every rank drives cuda:0 and the collectives go through gloo (RCCL refuses two ranks on one device); "nccl": rank
r drives cuda:r over RCCL.  A scenario that ends well prints `<scenario> OK` -- the parent looks for the marker, not at the exit
status (an RCCL teardown may abort after everything has passed) -- and the scenarios of one call run in the order given, the first
failure ending the process.  `world1_checks` is also what the in-process test calls."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kbnet_amd as kb
import kbnet_grad_cases as cases
import kbnet_grad_oracle as kgo
import resnet_pose_grad_cases as rcases

KbnError = kb._lib.KbnError
WD_DEPTH, WD_POSE, LR = 1e-4, 1e-3, 1e-4
FRAME = (32, 64)      # the whole-step scenarios' frames (tests/test_transforms_gpu.py's training iteration)
DROPPED = "dec::"     # the disagreement scenario drops the gradient of the first decoder parameter on rank 1


def depth_model(dev, c, sds=None):
    m = kb.modules.KBNetModel.from_config(c["cfg"], dev, trainable=True)
    m.load_state_dicts(*(cases.inputs(c)[4:7] if sds is None else sds))
    return m


def named(m):
    for grp, mod in zip(kgo.GROUPS, m.modules()):
        for k, p in mod.named_parameters():
            yield f"{grp}::{k}", p


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def backward_of(m, dev, c, lo=0, hi=None, scale=None):
    """sum(depth * cotangent) / scale over the frames lo..hi of case c, differentiated -> the activations `return_inner` gave."""
    args = cases.inputs(c)
    hi = c["n"] if hi is None else hi
    depth, inner = m.forward(*[t[lo:hi].to(dev) for t in args[:4]], return_inner=True)
    loss = (depth * args[7][lo:hi].float().to(dev)).sum()
    (loss if scale is None else loss / scale).backward()
    return inner


# ------------------------------------------------------------------------------------------ one rank: items 1 and 2
def world1_checks(dev, reduce_single):
    """After a backward pass of tiny_n3, average(n, n): every .grad keeps its bits and becomes a 16-byte-aligned view of the one
    buffer, the untouched parameters keep none; two kb.optim.Adam steps with the averager in the loop leave the bits of two steps
    without it.  With `reduce_single` the collectives run (a one-rank group), and broadcast_parameters leaves every bit."""
    c = cases.MODEL["tiny_n3"]
    m = depth_model(dev, c)
    pairs = list(named(m))
    assert [id(p) for _, p in pairs] == [id(p) for p in m.parameters()]
    averager = kb.dist.GradientAverager(pairs, 0, 1, reduce_single=reduce_single)
    assert averager.collective == bool(reduce_single)
    before = [p.detach().clone() for p in m.parameters()]
    versions = [p._version for p in m.parameters()]
    averager.broadcast_parameters()
    assert all(same_bits(p, b) for p, b in zip(m.parameters(), before))
    assert all(p._version == v + (1 if reduce_single else 0) for p, v in zip(m.parameters(), versions))
    assert not bool(averager.buffer.any())
    backward_of(m, dev, c)
    grads = {k: None if p.grad is None else p.grad.clone() for k, p in pairs}
    unused = cases.untouched(c)
    assert unused and sorted(k for k, g in grads.items() if g is None) == sorted(unused)
    averager.average(c["n"], c["n"])
    buf = averager.buffer
    lo, hi = buf.data_ptr(), buf.data_ptr() + 4 * buf.numel()
    seen = []
    for (k, p), off in zip(pairs, averager.offsets):
        if grads[k] is None:
            assert p.grad is None, k
            assert not bool(buf[off:off + p.numel()].any()), k      # its segment stays zero
            continue
        assert same_bits(p.grad, grads[k]), k
        assert p.grad.data_ptr() == lo + 4 * off and p.grad.data_ptr() % 16 == 0 and p.grad.is_contiguous(), k
        assert p.grad.data_ptr() + 4 * p.numel() <= hi and p.grad.shape == p.shape, k
        assert p.grad._base is buf, k
        seen.append((p.grad.data_ptr(), p.numel()))
    seen.sort()
    assert all(a + 4 * n <= b for (a, n), (b, _) in zip(seen, seen[1:]))
    # two steps with the averager in the loop, two without
    twin = depth_model(dev, c)
    opts = kb.optim.Adam(m.parameters(), lr=1e-3, weight_decay=WD_DEPTH), kb.optim.Adam(twin.parameters(), lr=1e-3, weight_decay=WD_DEPTH)
    for p in m.parameters():
        p.grad = None
    for step in range(2):
        for model, opt, avg in ((m, opts[0], averager), (twin, opts[1], None)):
            opt.zero_grad()
            backward_of(model, dev, c)
            if avg is not None:
                avg.average(c["n"], c["n"])
            opt.step()
    moved = 0
    for (k, p), q, b in zip(pairs, twin.parameters(), before):
        assert torch.equal(p.detach(), q.detach()), k
        moved += not torch.equal(p.detach(), b)
    assert moved == len(pairs) - len(unused)


# ------------------------------------------------------------------------------------------ two ranks: items 3 and 7
def oracle_scenario(dev, rank, world, out_dir):
    """tiny_n5 split 3 + 2: the rank differentiates sum(depth_r * cot_r) / n_r over its shard and calls average(n_r, 5).  Leaves
    rank<r>.pt for the parent: the reduced and the unweighted local gradients and the activations of its frames."""
    c = cases.MODEL["tiny_n5"]
    lo, hi = kb.dist.shard_bounds(c["n"], rank, world)
    m = depth_model(dev, c)
    pairs = list(named(m))
    averager = kb.dist.GradientAverager(pairs, rank, world)
    assert averager.collective
    inner = backward_of(m, dev, c, lo, hi, scale=hi - lo)
    local = {k: p.grad.clone().cpu() for k, p in pairs if p.grad is not None}
    averager.average(hi - lo, c["n"])
    reduced = {k: p.grad.cpu() for k, p in pairs if p.grad is not None}
    assert sorted(local) == sorted(reduced)
    assert all(p.grad is None or p.grad.data_ptr() == averager.buffer.data_ptr() + 4 * off for (_, p), off in zip(pairs, averager.offsets))
    torch.save({"n_local": hi - lo, "local": local, "reduced": reduced, "inner": {k: t.detach().cpu() for k, t in inner.items()}},
               os.path.join(out_dir, f"rank{rank}.pt"))


# ------------------------------------------------------------------------------------------ two ranks: item 4
def pose_model(dev, seed):
    rc = rcases.GOLDEN["resnet_pose_grad_18_eval"]
    pose = kb.posenet_resnet.ResNetPoseNetModel(n_layer=18, device=dev, n_filters=rc["filters"], decoder_filters=rc["decoder_filters"],
                                                trainable=True)
    pose.load_state_dicts(*kb.synthetic.make_resnet_pose_weights(18, rc["filters"], rc["decoder_filters"], seed=seed))
    pose.requires_grad_(True).set_batch_norm("running")
    return pose


def whole_step(dev, depth, pose, opt, averager, frames, n_global):
    """The reference's training step (src/kbnet.py:392-453) on this rank's frames (none: no forward, no backward)."""
    n_local = frames[0].shape[0]
    opt.zero_grad()
    if n_local:
        i0, i1, i2, sparse, validity, k = (t.to(dev) for t in frames)
        out = depth.forward(i0, sparse, validity, k)
        pose01, pose02 = pose.forward(i0, i1), pose.forward(i0, i2)
        loss, _ = depth.compute_loss(i0, i1, i2, out, sparse, validity, k, pose01, pose02)
        loss.backward()
    averager.average(n_local, n_global)
    opt.step()


def replicas_scenario(dev, rank, world):
    """Narrow KBNet + narrow ResNet-18 pose network ('running'), compute_loss, kb.optim.Adam with the two groups.  Rank 1 starts
    from other weights; after broadcast_parameters and two steps -- the second on a ragged global batch of 3 frames -- the packed
    parameters are equal across ranks, bit for bit, and differ from the initial ones."""
    import torch.distributed as dist
    cfg = kb.kitti_config().narrow()
    depth = kb.modules.KBNetModel.from_config(cfg, dev, trainable=True)
    depth.load_state_dicts(*kb.synthetic.make_state_dicts(cfg, seed=10 * rank, gain=1.3))
    pose = pose_model(dev, seed=5 + rank)
    params = depth.parameters() + pose.parameters()
    opt = kb.optim.Adam([{"params": depth.parameters(), "weight_decay": WD_DEPTH}, {"params": pose.parameters(), "weight_decay": WD_POSE}], lr=LR)
    averager = kb.dist.GradientAverager(params, rank, world)

    def packed():
        mine = torch.cat([p.detach().reshape(-1) for p in params])
        every = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        return every

    start = packed()
    assert not torch.equal(start[0], start[1]), "the ranks must start from different weights"
    averager.broadcast_parameters()
    sent = packed()
    assert all(same_bits(s, start[0]) for s in sent)
    for step, n_global in enumerate((4, 3)):
        i0, i1, i2, _, sparse, validity, k, _, _ = kb.synthetic.make_triplet(n_global, *FRAME, "kitti", seed=41 + step)
        lo, hi = kb.dist.shard_bounds(n_global, rank, world)
        assert hi > lo
        whole_step(dev, depth, pose, opt, averager, [t[lo:hi] for t in (i0, i1, i2, sparse, validity, k)], n_global)
    end = packed()
    assert all(torch.equal(e, end[0]) for e in end), "the replicas diverged"
    assert bool(torch.isfinite(end[0]).all()) and not torch.equal(end[0], start[0])
    changed = sum(not torch.equal(p.detach().reshape(-1), s) for p, s in zip(params, start[0].split([p.numel() for p in params])))
    with_grad = sum(p.grad is not None for p in params)
    assert changed == with_grad and len(params) // 2 < with_grad < len(params), (changed, with_grad, len(params))


# ------------------------------------------------------------------------------------------ two ranks: item 5
def empty_shard_scenario(dev, rank, world):
    """A global batch of ONE frame: rank 1 has none, calls average(0, 1) without a backward pass and steps.  Both ranks end with
    the bits a single process stepping on that frame holds (computed here, on a twin)."""
    c = cases.MODEL["tiny"]
    assert c["n"] == 1
    lo, hi = kb.dist.shard_bounds(1, rank, world)
    assert (hi - lo) == (1 if rank == 0 else 0)
    m, twin = depth_model(dev, c), depth_model(dev, c)
    opt, opt_twin = (kb.optim.Adam(x.parameters(), lr=1e-3, weight_decay=WD_DEPTH) for x in (m, twin))
    averager = kb.dist.GradientAverager(list(named(m)), rank, world)
    before = [p.detach().clone() for p in m.parameters()]
    for step in range(2):      # the second step: the agreed set is known, the rank without frames binds its views from it
        opt.zero_grad()
        if hi > lo:
            backward_of(m, dev, c, scale=1)
        kb.ops.PROFILE = []
        try:
            averager.average(hi - lo, 1)
            launches = len(kb.ops.PROFILE)
        finally:
            kb.ops.PROFILE = None
        assert (launches > 0) == (hi > lo), "a rank without frames launches no pack kernel"
        opt.step()
        opt_twin.zero_grad()
        backward_of(twin, dev, c, scale=1)
        opt_twin.step()
    moved = 0
    for (k, p), q, b in zip(named(m), twin.parameters(), before):
        assert torch.equal(p.detach(), q.detach()), (rank, k)
        moved += not torch.equal(p.detach(), b)
    assert moved == len(before) - len(cases.untouched(c))


# ------------------------------------------------------------------------------------------ two ranks: item 6
def disagreement_scenario(dev, rank, world):
    """Rank 1 loses one parameter's gradient before its first average call: BOTH ranks must raise KbnError naming it."""
    c = cases.MODEL["tiny"]
    m = depth_model(dev, c)
    pairs = list(named(m))
    averager = kb.dist.GradientAverager(pairs, rank, world)
    backward_of(m, dev, c, scale=1)
    name, p = next((k, p) for k, p in pairs if k.startswith(DROPPED) and p.grad is not None)
    if rank == 1:
        p.grad = None
    try:
        averager.average(1, 2)
    except KbnError as e:
        print(f"KBNERROR on rank {rank}: {e}", flush=True)
        assert name in str(e)
        print(f"DROPPED {name}", flush=True)
        return
    raise AssertionError("average() returned although the ranks disagree")


def main(argv):
    import torch.distributed as dist
    backend, rank, world, port, out_dir = argv[0], int(argv[1]), int(argv[2]), int(argv[3]), argv[4]
    dev = torch.device("cuda", rank if backend == "nccl" else 0)
    torch.cuda.set_device(dev)
    dist.init_process_group(backend=backend, init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        for scenario in argv[5:]:
            if scenario == "single":
                world1_checks(dev, reduce_single=True)
            elif scenario == "oracle":
                oracle_scenario(dev, rank, world, out_dir)
            elif scenario == "replicas":
                replicas_scenario(dev, rank, world)
            elif scenario == "empty":
                empty_shard_scenario(dev, rank, world)
            elif scenario == "disagree":
                disagreement_scenario(dev, rank, world)
            else:
                raise SystemExit(f"unknown scenario {scenario}")
            torch.cuda.synchronize()
            print(f"{scenario} OK", flush=True)
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1:])
