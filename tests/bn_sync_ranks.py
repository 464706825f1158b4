"""What the ranks of tests/test_bn_sync_ranks_gpu.py run, each in a process of its own:

    python tests/bn_sync_ranks.py <backend> <rank> <world> <port> <out_dir> <scenario> [<scenario> ...]

backend "gloo": every rank drives cuda:0 and the collectives go through gloo; "nccl": rank r drives cuda:r over RCCL.  A scenario
that ends well prints `<scenario> OK` (the parent looks for the marker, as in tests/grad_average_ranks.py); the first failure ends
the process.

The two networks run their three-frame 'batch' cases split 2 + 1: each rank differentiates the mean over its own frames of
sum(pose * cotangent) and calls GradientAverager.average(n_r, 3)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kbnet_amd as kb
import posenet_grad_cases as pcases
import resnet_pose_grad_cases as rcases

NETS = {"posenet": ("narrow_n3_batch", pcases), "resnet18": ("narrow_18_n3_batch", rcases)}
LR, WD = 1e-4, 1e-3


def build(net, dev, group):
    """(case, its inputs, the model in 'batch' mode with every parameter trainable, (name, parameter) pairs)."""
    name, cases = NETS[net]
    c = cases.MODEL[name]
    args = cases.inputs(c)
    if net == "posenet":
        m = kb.modules.PoseNetModel(device=dev, n_filters=c["filters"])
    else:
        m = kb.posenet_resnet.ResNetPoseNetModel(n_layer=c["n_layer"], device=dev, n_filters=c["filters"],
                                                 decoder_filters=c["decoder_filters"], trainable=True)
    m.load_state_dicts(args[2], args[3])
    m.requires_grad_(True).set_batch_norm("batch").sync_batch_norm(group)
    pairs = [(f"{grp}::{k}", p) for grp, mod in (("enc", m.encoder), ("dec", m.decoder)) for k, p in mod.named_parameters()]
    assert [id(p) for _, p in pairs] == [id(p) for p in m.parameters()]
    return c, args, m, pairs


def buffers(m):
    return {f"{grp}::{k}": v for grp, mod in (("enc", m.encoder), ("dec", m.decoder)) for k, v in mod.state_dict().items()
            if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}


def backward_of(net, m, dev, args, frames, n_local):
    """The rank's loss on the frames `frames` of the case (a mean over its own), differentiated -> (layer outputs, inner outputs)."""
    image0, image1, cot = (args[i][frames] for i in (0, 1, 4))
    if net == "posenet":
        pose, _, layers = m.forward(image0.to(dev), image1.to(dev), return_all=True)
        inner = {}
    else:
        pose, _, layers, inner = m.forward(image0.to(dev), image1.to(dev), return_all=True, return_inner=True)
    ((pose * cot.float().to(dev)).sum() / n_local).backward()
    return layers, inner


def one_pass(net, dev, rank, world, sync):
    """A fresh model, one forward and backward on this rank's shard, average(n_r, n) -> what the parent compares."""
    group = kb.dist.BatchNormGroup(rank, world) if sync else None
    c, args, m, pairs = build(net, dev, group)
    lo, hi = kb.dist.shard_bounds(c["n"], rank, world)
    averager = kb.dist.GradientAverager(pairs, rank, world)
    layers, inner = backward_of(net, m, dev, args, slice(lo, hi), hi - lo)
    averager.average(hi - lo, c["n"])
    return {"n_local": hi - lo,
            "reduced": {k: p.grad.cpu() for k, p in pairs if p.grad is not None},
            "layers": [t.detach().cpu() for t in layers],
            "inner": {k: t.detach().cpu() for k, t in inner.items()},
            "buffers": {k: v.cpu() for k, v in buffers(m).items()}}


def oracle_scenario(dev, rank, world, out_dir):
    """Leaves rank<r>.pt: for both networks the pass with synchronised BatchNorm and the pass without."""
    out = {net: {"sync": one_pass(net, dev, rank, world, True), "local": one_pass(net, dev, rank, world, False)} for net in NETS}
    torch.save(out, os.path.join(out_dir, f"rank{rank}.pt"))


def same_bits(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if not a.is_floating_point():
        return torch.equal(a, b)
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def replicas_scenario(dev, rank, world):
    """Two steps with kb.optim.Adam on shards 2 + 1 (the second on the frames in another order): every parameter and every
    BatchNorm buffer ends bit-equal on the two ranks, and has moved."""
    import torch.distributed as dist
    for net in NETS:
        c, args, m, pairs = build(net, dev, kb.dist.BatchNormGroup(rank, world))
        before = [p.detach().clone() for _, p in pairs]
        opt = kb.optim.Adam(m.parameters(), lr=LR, weight_decay=WD)
        averager = kb.dist.GradientAverager(pairs, rank, world)
        lo, hi = kb.dist.shard_bounds(c["n"], rank, world)
        for step in range(2):
            order = torch.roll(torch.arange(c["n"]), step)
            opt.zero_grad()
            backward_of(net, m, dev, args, order[lo:hi], hi - lo)
            averager.average(hi - lo, c["n"])
            opt.step()
        state = dict(pairs)
        state.update(buffers(m))
        for k, t in state.items():
            mine = t.detach().contiguous()
            every = [torch.empty_like(mine) for _ in range(world)]
            dist.all_gather(every, mine)
            assert all(same_bits(e, every[0]) for e in every), (net, k)
            if k.endswith("num_batches_tracked"):
                assert int(mine) == 1002, (net, k)
            else:
                assert bool(torch.isfinite(mine).all()), (net, k)
        moved = sum(not torch.equal(p.detach(), b) for (_, p), b in zip(pairs, before))
        assert moved == sum(p.grad is not None for _, p in pairs) and moved > len(pairs) // 2, (net, moved)


def determinism_scenario(dev, rank, world):
    """The synchronised pass twice from the same state: the same bits in every reduced gradient, activation and buffer."""
    for net in NETS:
        a, b = one_pass(net, dev, rank, world, True), one_pass(net, dev, rank, world, True)
        for k in a["reduced"]:
            assert same_bits(a["reduced"][k], b["reduced"][k]), (net, k)
        for k in a["buffers"]:
            assert same_bits(a["buffers"][k], b["buffers"][k]), (net, k)
        assert all(same_bits(x, y) for x, y in zip(a["layers"], b["layers"])), net


def main(argv):
    import torch.distributed as dist
    backend, rank, world, port, out_dir = argv[0], int(argv[1]), int(argv[2]), int(argv[3]), argv[4]
    dev = torch.device("cuda", rank if backend == "nccl" else 0)
    torch.cuda.set_device(dev)
    dist.init_process_group(backend=backend, init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        for scenario in argv[5:]:
            if scenario == "oracle":
                oracle_scenario(dev, rank, world, out_dir)
            elif scenario == "replicas":
                replicas_scenario(dev, rank, world)
            elif scenario == "determinism":
                determinism_scenario(dev, rank, world)
            else:
                raise SystemExit(f"unknown scenario {scenario}")
            torch.cuda.synchronize()
            print(f"{scenario} OK", flush=True)
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1:])
