"""GPU: kb.dist.GradientAverager, the data-parallel training step.  One rank in this process; one-rank RCCL and two-rank groups in
child processes (tests/grad_average_ranks.py), which print a marker per scenario that ended well -- an RCCL teardown abort after it
cannot end the suite.  Two ranks share cuda:0 over gloo (RCCL refuses two ranks on one device); the same comparison runs over RCCL
where two devices are visible.

The two-rank gradients are held to the depth network's existing gate against the fp64 oracle, kgo.fraction(got, want / 5) <= kgo.TOL:
the ranks differentiate per-shard means, average() weights them n_r / 5, so the reduced gradient is the global-batch mean's.

    python -m pytest tests/test_grad_average_gpu.py -m gpu -q -s
"""
import os
import socket
import subprocess
import sys

import pytest
import torch

import kbnet_amd as kb
import grad_average_ranks as ranks
import kbnet_grad_cases as cases
import kbnet_grad_oracle as kgo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT = 300      # seconds a rank may take: a collective that waits for a rank that left ends here, not with the suite


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
    script = os.path.join(ROOT, "tests", "grad_average_ranks.py")
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
    """Two ranks on cuda:0 over gloo, started once: the oracle comparison's gradients, then the replica and empty-shard scenarios."""
    out_dir = tmp_path_factory.mktemp("grad_average")
    return out_dir, run_ranks("gloo", 2, out_dir, ["oracle", "replicas", "empty"])


# ----------------------------------------------------------------------------------------------------------- one rank
def test_world_1_without_a_group(dev):
    assert not torch.distributed.is_initialized()
    ranks.world1_checks(dev, reduce_single=False)


def test_one_rank_rccl_group(dev, tmp_path):
    """The same assertions through the real collectives (reduce_single=True on a one-rank RCCL group), and broadcast_parameters
    leaves every parameter's bits."""
    results = run_ranks("nccl", 1, tmp_path, ["single"])
    assert passed(results, "single"), "the child died before the end of the body (its output is printed above)"
    if results[0][2] != 0:
        print(f"(the child's teardown exited with {results[0][2]} after the body had passed: {results[0][1][-300:]})")


# ----------------------------------------------------------------------------------------------------------- two ranks
def against_the_oracle(out_dir, label):
    """Every rank's reduced gradient of every parameter against the fp64 oracle's gradient of the WHOLE batch / 5, on the branches
    the ranks took; and the 1 / world mistake, (g_0 + g_1) / 2 of the unweighted local gradients, must fail the same gate."""
    c = cases.MODEL["tiny_n5"]
    got = [torch.load(os.path.join(out_dir, f"rank{r}.pt")) for r in range(2)]
    assert [g["n_local"] for g in got] == [3, 2]
    args = cases.inputs(c)
    masks = kgo.masks_of({k: torch.cat([g["inner"][k] for g in got], dim=0) for k in got[0]["inner"]})      # frame order: rank 0's three first
    want = kgo.gradients(*args, c["cfg"], masks=masks)
    kinks = kgo.check_kinks(masks, want["pre"])
    keys = kgo.gradient_keys(want)
    unused = cases.untouched(c)
    assert sorted(keys) == sorted(set(kgo.parameter_keys(*args[4:7])) - set(unused))
    worst = 0.0
    for rank, g in enumerate(got):
        assert sorted(g["reduced"]) == sorted(keys), rank
        for k in keys:
            assert torch.isfinite(g["reduced"][k]).all() and float(g["reduced"][k].abs().max()) > 0, (rank, k)
            f = kgo.fraction(g["reduced"][k], want[k] / 5)
            worst = max(worst, f)
            assert f <= kgo.TOL, (label, rank, k, f)
    assert all(torch.equal(got[0]["reduced"][k], got[1]["reduced"][k]) for k in keys), "the ranks hold different reduced gradients"
    # per-rank means averaged 1 / world: 1/2 against 3/5 and 2/5 of the frames' gradients
    mistaken = {k: (got[0]["local"][k] + got[1]["local"][k]) / 2 for k in keys}
    wrong = [kgo.fraction(mistaken[k], want[k] / 5) for k in keys]
    print(f"{label}: worst reduced gradient at {worst:.2e} of |b| + rms(b) (gate {kgo.TOL:.0e}), {kinks} activations on the other side "
          f"of the kink than in fp64; with 1 / world weights the worst is {max(wrong):.2e}, the best {min(wrong):.2e}")
    assert max(wrong) > kgo.TOL, "the test cannot tell n_local / n_global from 1 / world"


def test_two_ranks_against_the_fp64_oracle(two_ranks):
    out_dir, results = two_ranks
    assert passed(results, "oracle")
    against_the_oracle(out_dir, "two ranks on cuda:0 over gloo, 3 + 2 frames")


def test_replicas_stay_identical(two_ranks):
    assert passed(two_ranks[1], "replicas")


def test_a_rank_with_an_empty_shard(two_ranks):
    assert passed(two_ranks[1], "empty")


def test_disagreement_is_loud_not_a_hang(dev, tmp_path):
    results = run_ranks("gloo", 2, tmp_path, ["disagree"])      # run_ranks ends a rank that waits after TIMEOUT: a hang fails here
    assert passed(results, "disagree")
    names = set()
    for rank, (out, _, _) in enumerate(results):
        error = [line for line in out.splitlines() if line.startswith(f"KBNERROR on rank {rank}:")]
        dropped = [line.split(" ", 1)[1] for line in out.splitlines() if line.startswith("DROPPED ")]
        assert len(error) == 1 and len(dropped) == 1 and dropped[0] in error[0] and "disagree" in error[0], (rank, out)
        names.add(dropped[0])
    assert len(names) == 1 and names.pop().startswith(ranks.DROPPED)


def test_two_ranks_over_rccl(tmp_path):
    """The oracle comparison with rank r on cuda:r over RCCL.  One-GPU leases skip it, with the reason in the report (-rs)."""
    n = torch.cuda.device_count() if torch.cuda.is_available() else 0
    if n < 2:
        print(f"SKIP: {n} visible GPU(s); two ranks over RCCL need two devices (the gloo test above runs the same code on one)")
        pytest.skip(f"{n} visible GPU(s): two RCCL ranks need two devices")
    kb._lib.load()
    results = run_ranks("nccl", 2, tmp_path, ["oracle"])
    assert passed(results, "oracle")
    against_the_oracle(tmp_path, "two ranks on two devices over RCCL, 3 + 2 frames")
