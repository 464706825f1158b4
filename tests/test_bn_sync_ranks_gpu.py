"""GPU, two ranks: synchronised BatchNorm through real collectives (tests/bn_sync_ranks.py in child processes, the pattern of
tests/test_grad_average_gpu.py: two ranks share cuda:0 over gloo, each under a time limit, logs in files, a marker per scenario;
the same over RCCL where two devices are visible).

PoseNetModel on narrow_n3_batch and ResNetPoseNetModel(18) on narrow_18_n3_batch, shards 2 + 1.  Every rank's reduced gradient of
every parameter is held to the network's EXISTING gate (posenet_grad_oracle.TOL / resnet_pose_grad_oracle.TOL) against the fp64
oracle's gradient of the WHOLE batch / 3, on the branches the ranks took (kink_check as in the model tests); the running statistics to
the oracle's values for the whole batch.  The same run without sync_batch_norm must fail that gate: the test that fails without
the feature.

    python -m pytest tests/test_bn_sync_ranks_gpu.py -m gpu -q -s
"""
import os
import socket
import subprocess
import sys

import pytest
import torch

import kbnet_amd as kb
import bn_sync_ranks as ranks
import posenet_grad_oracle as pgo
import posenet_oracle as po
import resnet_pose_grad_oracle as rgo
import test_resnet_pose_train_gpu as resnet_test

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT = 300      # seconds a rank may take: a collective that waits for a rank that left ends here, not with the suite
SCENARIOS = ["oracle", "replicas", "determinism"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need a visible MI355X (run with -m gpu on a GPU box)")
    kb._lib.load()   # a missing extension is an error on a GPU box, never a skip
    return torch.device("cuda:0")


def run_ranks(backend, world, out_dir, scenarios):
    """Starts the ranks, each a process of its own, and waits for all of them -> [(stdout, stderr, exit status)] by rank."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    script = os.path.join(ROOT, "tests", "bn_sync_ranks.py")
    # the ranks write to files: a rank whose pipe is full would keep the other waiting in a collective
    logs = [[open(os.path.join(str(out_dir), f"rank{rank}.{name}"), "w+") for name in ("out", "err")] for rank in range(world)]
    children = [subprocess.Popen([sys.executable, script, backend, str(rank), str(world), str(port), str(out_dir)] + list(scenarios),
                                 stdout=logs[rank][0], stderr=logs[rank][1], env=env) for rank in range(world)]
    try:
        for child in children:
            try:
                child.wait(timeout=TIMEOUT)
            except subprocess.TimeoutExpired:
                pass      # ended below; its log lacks the marker
    finally:
        for child in children:
            if child.poll() is None:
                child.kill()
                child.wait()
    results = []
    for child, (out, err) in zip(children, logs):
        texts = []
        for f in (out, err):
            f.seek(0)
            texts.append(f.read())
            f.close()
        results.append((texts[0], texts[1], child.returncode))
    return results


def passed(results, scenario):
    ok = all(f"{scenario} OK" in out for out, _, _ in results)
    if not ok:
        for rank, (out, err, status) in enumerate(results):
            print(f"---- rank {rank} (exit status {status}) ----\n{out[-2000:]}\n{err[-6000:]}")
    return ok


@pytest.fixture(scope="module")
def two_ranks(dev, tmp_path_factory):
    """Two ranks on cuda:0 over gloo, started once for all scenarios."""
    out_dir = tmp_path_factory.mktemp("bn_sync")
    return out_dir, run_ranks("gloo", 2, out_dir, SCENARIOS)


def _oracle(net, got):
    """The fp64 oracle's gradients and running statistics of the WHOLE batch on the branches the synchronised ranks took ->
    (want, the gate's fraction function, its tolerance, run-key prefix)."""
    name, cases = ranks.NETS[net]
    c = cases.MODEL[name]
    args = cases.inputs(c)
    layers = [torch.cat([g["sync"]["layers"][i] for g in got], dim=0) for i in range(len(got[0]["sync"]["layers"]))]   # rank 0's frames first
    if net == "posenet":
        masks = [t > 0 for t in layers]
        want = pgo.gradients(*args, batch_norm="batch", masks=masks)
        kinks = pgo.kink_check(masks, want["pre"])
        return want, pgo.fraction, pgo.TOL, kinks, lambda k: "run::" + k.split("::", 1)[1]
    inner = {k: torch.cat([g["sync"]["inner"][k] for g in got], dim=0) for k in got[0]["sync"]["inner"]}
    masks, indices = resnet_test._branches(c, layers, inner)
    want = rgo.gradients(*args, n_layer=c["n_layer"], batch_norm="batch", masks=masks, pool_indices=indices)
    kinks = rgo.kink_check(masks, want["pre"], indices, want["pool_in"])
    return want, rgo.fraction, rgo.TOL, kinks, lambda k: "run::" + k


def against_the_oracle(out_dir, label):
    got = [torch.load(os.path.join(out_dir, f"rank{r}.pt")) for r in range(2)]
    for net in ranks.NETS:
        mine = [g[net] for g in got]
        assert [g["sync"]["n_local"] for g in mine] == [2, 1]
        want, fraction, tol, kinks, run_key = _oracle(net, mine)
        keys = sorted(k for k in want if k.startswith(("enc::", "dec::")))
        worst = 0.0
        for rank, g in enumerate(mine):
            assert sorted(g["sync"]["reduced"]) == keys, (net, rank)
            for k in keys:
                a = g["sync"]["reduced"][k]
                assert torch.isfinite(a).all() and float(a.abs().max()) > 0, (net, rank, k)
                f = fraction(a, want[k] / 3)
                worst = max(worst, f)
                assert f <= tol, (label, net, rank, k, f)
            checked = 0
            for k, a in g["sync"]["buffers"].items():
                if k.endswith("num_batches_tracked"):
                    assert int(a) == 1001, (net, rank, k)
                    continue
                b = want[run_key(k)]
                f = po.gate_fraction(a, b, po.layer_floor(b))
                assert f <= 1.0, (label, net, rank, k, f)
                checked += 1
            assert checked >= 14
        for part in ("reduced", "buffers"):
            assert all(torch.equal(mine[0]["sync"][part][k], mine[1]["sync"][part][k]) for k in mine[0]["sync"][part]), \
                f"{net}: the ranks hold different {part}"
        # the same run on per-shard statistics (sync_batch_norm(None)): what the parent commit computes on two ranks
        local = {k: max(fraction(g["local"]["reduced"][k], want[k] / 3) for g in mine) for k in keys}
        low, high = min(local, key=local.get), max(local, key=local.get)
        print(f"{label}, {net}: worst reduced gradient at {worst:.2e} of |b| + rms(b) (gate {tol:.0e}), {kinks} branches on the other side "
              f"of the kink than in fp64; WITHOUT sync_batch_norm {local[low]:.2e} ({low}) to {local[high]:.2e} ({high})")
        assert local[high] > tol, "the test cannot tell synchronised BatchNorm from per-shard statistics"
        assert any(not torch.equal(mine[0]["local"]["buffers"][k], mine[1]["local"]["buffers"][k]) for k in mine[0]["local"]["buffers"])


def test_two_ranks_against_the_fp64_oracle(two_ranks):
    out_dir, results = two_ranks
    assert passed(results, "oracle")
    against_the_oracle(out_dir, "two ranks on cuda:0 over gloo, 2 + 1 frames")


def test_replicas_stay_identical(two_ranks):
    assert passed(two_ranks[1], "replicas")


def test_a_second_run_repeats_its_bits(two_ranks):
    assert passed(two_ranks[1], "determinism")


def test_two_ranks_over_rccl(tmp_path):
    """The same scenarios with rank r on cuda:r over RCCL.  One-GPU leases skip it, with the reason in the report (-rs)."""
    n = torch.cuda.device_count() if torch.cuda.is_available() else 0
    if n < 2:
        print(f"SKIP: {n} visible GPU(s); two ranks over RCCL need two devices (the gloo tests above run the same code on one)")
        pytest.skip(f"{n} visible GPU(s): two RCCL ranks need two devices")
    kb._lib.load()
    results = run_ranks("nccl", 2, tmp_path, SCENARIOS)
    for scenario in SCENARIOS:
        assert passed(results, scenario)
    against_the_oracle(tmp_path, "two ranks on two devices over RCCL, 2 + 1 frames")
