"""GPU, two ranks through kb.training.launch itself: train_ranks(rank, world) against a one-process train() under the same seeds.

Two ranks share cuda:0 over gloo (launch(2, backend="gloo", devices=[0, 0])), each a fresh child process under launch's time limit,
at most two children at a time; the same over RCCL where two devices are visible.  The settings are tests/train_cases.py's: three
24 x 40 frames, batch 3 -- shards 2 + 1 -- three epochs of one step, a summary, a checkpoint and (from step 2) a validation every
step.  The one-process side records its writers' calls; the two-rank side writes event files with the default writers.

The gradient gate.  After step 1 Adam's exp_avg is (1 - beta1) (g + weight_decay p) with g the reduced gradient, and both runs
start from the same weights: per parameter the two-rank exp_avg must lie within tol |b| + tol rms(b) of the one-process exp_avg b,
tol = 2 x the network's existing gate against fp64 (kbnet_grad_oracle.TOL for the depth network, resnet_pose_grad_oracle.TOL for
the pose network) -- each run is held to that gate against the same fp64 gradient elsewhere, so the factor two is the triangle
inequality.  The same comparison for a run with sync_batch_norm=False must FAIL the pose parameters' gate: per-shard statistics
differentiate another function.  At the settings above that run cannot be made at all: rank 1's shard is ONE
24 x 40 frame, whose deepest pose maps are 1 x 1, and batch statistics of one value a channel do not exist -- the package raises
KbnError there, as torch.nn.BatchNorm2d does (the reference's DataParallel could not train this split either).  That refusal is
asserted, and the gate's power is shown where per-shard statistics exist: the four triplets of tests/golden/train_io centre-cropped
to 24 x 40, batch 4, shards 2 + 2, one step -- with synchronised BatchNorm the gate holds there too, without it the pose parameters
fail it.

    python -m pytest tests/test_train_ranks_gpu.py -m gpu -q -s
"""
import math
import os
import re
import time

import numpy as np
import pytest
import torch

import kbnet_amd as kb
from conftest import GOLDEN_DIR
import event_cases as ec
import kbnet_grad_oracle as kgo
import resnet_pose_grad_oracle as rgo
import test_train_gpu as base
import train_cases as tc
from test_train_gpu import inputs  # noqa: F401  (the fixture: path lists, checkpoints and settings in one directory)

pytestmark = pytest.mark.gpu

TIMEOUT = 300      # seconds a launch may take, as tests/test_bn_sync_ranks_gpu.py gives its ranks: a collective that waits for a rank that left ends here
LOSS_TOL = base.LOSS_TOL
ARGUMENT_NAMES = ("train_image_path", "train_sparse_depth_path", "train_intrinsics_path", "val_image_path", "val_sparse_depth_path",
                  "val_intrinsics_path", "val_ground_truth_path")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need a visible MI355X (run with -m gpu on a GPU box)")
    kb._lib.load()   # a missing extension is an error on a GPU box, never a skip
    return torch.device("cuda:0")


def _launch(inputs, out, backend="gloo", devices=(0, 0), **more):  # noqa: F811
    lists = inputs["lists"]
    arguments = dict(zip(ARGUMENT_NAMES, lists[:3] + lists))
    arguments.update(inputs["settings"], checkpoint_path=out, depth_model_restore_path=inputs["depth"],
                     pose_model_restore_path=inputs["pose"], device="cuda", workers=2)
    arguments.update(more)
    base._seed()      # the children start from the caller's random state
    started = time.time()
    results, logged, checkpoints = kb.training.launch(2, backend=backend, devices=list(devices), timeout=TIMEOUT, **arguments)
    return {"out": out, "results": results, "logged": logged, "checkpoints": checkpoints, "seconds": time.time() - started}


@pytest.fixture(scope="module")
def one_process(dev, inputs, tmp_path_factory):  # noqa: F811
    """train() in this process with recording writers."""
    out = str(tmp_path_factory.mktemp("ranks_one") / "trained")
    writers = []

    def factory(log_dir):
        writers.append(tc.RecordingWriter(log_dir))
        return writers[-1]

    started = time.time()
    results, logged, checkpoints = base._train(inputs, out, summary_writer_factory=factory)
    return {"out": out, "results": results, "logged": logged, "checkpoints": checkpoints, "writers": writers, "seconds": time.time() - started}


@pytest.fixture(scope="module")
def two_ranks(dev, inputs, tmp_path_factory):  # noqa: F811
    return _launch(inputs, str(tmp_path_factory.mktemp("ranks_two") / "trained"))


@pytest.fixture(scope="module")
def four_frames(dev, inputs, tmp_path_factory):  # noqa: F811
    """One step on the four triplets of golden/train_io (24 x 40, 26 x 44, 25 x 43, 24 x 40) centre-cropped to 24 x 40, batch 4: one
    process, two ranks (2 + 2 frames), and two ranks with sync_batch_norm=False -- the reference's DataParallel behaviour, every
    rank's BatchNorm layers normalising with the statistics of its own shard."""
    root = tmp_path_factory.mktemp("ranks_four")
    io = os.path.join(GOLDEN_DIR, "train_io")
    lists = []
    for name, pattern in (("image.txt", "triplet_{}.png"), ("sparse_depth.txt", "depth_{}.png"), ("intrinsics.txt", "k_{}.npy")):
        lists.append(str(root / name))
        with open(lists[-1], "w") as f:
            f.write("\n".join(os.path.join(io, pattern.format(i)) for i in range(4)) + "\n")
    # the validation lists are the training lists (the sparse depth as ground truth): read, and never used -- no step reaches 100
    four = dict(inputs, lists=lists + [lists[1]], settings=dict(inputs["settings"], n_batch=4, learning_rates=[1e-4], learning_schedule=[1],
                                                                 n_summary=100, validation_start_step=100))
    results, logged, checkpoints = base._train(four, str(root / "one"))
    one = {"out": str(root / "one"), "results": results, "logged": logged}
    return {"one": one, "two": _launch(four, str(root / "two")), "local": _launch(four, str(root / "local"), sync_batch_norm=False)}


def _lines(run):
    with open(os.path.join(run["out"], "results.txt")) as f:
        return f.read().splitlines()


# ------------------------------------------------------------------------------------------------ what is written, and by whom
def test_results_text_line_for_line(one_process, two_ranks):
    got, want = _lines(two_ranks), _lines(one_process)
    assert len(got) == len(want), ("\n".join(got), "\n".join(want))
    steps = numbers = 0
    for i, (g, w) in enumerate(zip(got, want)):
        if w.startswith(("checkpoint_path=", "event_path=")):
            key = w.split("=")[0] + "="
            assert g.startswith(key + two_ranks["out"]) and w.startswith(key + one_process["out"]), (g, w)
        elif re.match(base.STEP, w):
            assert re.match(base.STEP, g) and re.match(base.STEP, g).group(1) == re.match(base.STEP, w).group(1), (g, w)
            steps += 1
        elif re.match(base.NUMBERS, w):
            assert re.match(base.NUMBERS, g), (g, w)
            if want[i - 2] == "Validation results:":
                assert re.match(base.NUMBERS, g).group(1) == re.match(base.NUMBERS, w).group(1), (g, w)
            numbers += 1
        else:
            assert g == w, (i, g, w)      # the path lists, every setting, device=cuda, n_train_step=3
    assert steps == 3 and numbers == 4
    assert "device=cuda" in got and "n_sample=3  n_epoch=3  n_step=3" in got


def test_rank_0_writes_everything_once(two_ranks):
    out = two_ranks["out"]
    assert sorted(os.listdir(out)) == sorted(
        ["results.txt", "events-train", "events-val", "launch-arguments.pkl", "launch-results.pkl"]
        + [f"{model}_model-{step}.pth" for model in ("depth", "pose") for step in (1, 2, 3)]
        + [f"rank{rank}.{kind}" for rank in range(2) for kind in ("out", "err", "digest")])
    for which in ("train", "val"):
        assert len(os.listdir(os.path.join(out, "events-" + which))) == 1
    with open(os.path.join(out, "rank0.out")) as f:
        first = f.read()
    with open(os.path.join(out, "rank1.out")) as f:
        second = f.read()
    assert "Begin training..." in first and len(re.findall(r"(?m)^Step=", first)) == 3
    assert "Begin training..." not in second and "Step=" not in second and "n_batch=" not in second
    assert sorted(two_ranks["checkpoints"]) == sorted(os.path.join(out, n) for n in os.listdir(out) if n.endswith(".pth"))


@pytest.mark.parametrize("which", ["train", "val"])
def test_event_files_hold_the_one_process_calls(one_process, two_ranks, which):
    directory = os.path.join(two_ranks["out"], "events-" + which)
    [name] = os.listdir(directory)
    events = ec.read_events(os.path.join(directory, name))
    kinds = {"add_scalar": "scalar", "add_histogram": "histo", "add_image": "image"}
    writer = one_process["writers"][0 if which == "train" else 1]
    assert [(e["kind"], e["tag"], e["step"]) for e in events[1:]] == [(kinds[m], t, s) for m, t, s in writer.calls]
    assert len(writer.calls) == (45 if which == "train" else 16)
    if which == "train":      # the panels are the global batch's: three columns, not rank 0's two
        panels = [e["value"] for e in events[1:] if e["kind"] == "image"]
        widths = {p[1] for p in panels}
        assert len(panels) == 6 and len(widths) == 1 and widths.pop() > 3 * tc.N_WIDTH


def test_checkpoint_steps_and_learning_rates(one_process, two_ranks):
    for name in sorted(os.path.basename(p) for p in one_process["checkpoints"]):
        a = torch.load(os.path.join(two_ranks["out"], name), map_location="cpu")
        b = torch.load(os.path.join(one_process["out"], name), map_location="cpu")
        assert int(a["train_step"]) == int(b["train_step"]), name
        lrs = lambda c: [float(g["lr"]) for g in c["optimizer_state_dict"]["param_groups"]]
        assert lrs(a) == lrs(b) and len(lrs(a)) == 2, name
        assert sorted(a["optimizer_state_dict"]["state"]) == sorted(b["optimizer_state_dict"]["state"]), name
    assert two_ranks["results"]["train_step"] == one_process["results"]["train_step"] == 3
    assert two_ranks["results"]["best_results"]["step"] in (2, 3)


# ------------------------------------------------------------------------------------------------ numbers
def test_the_logged_loss_is_the_global_batchs(one_process, two_ranks):
    """Step 1, before any update: within 1e-4 relative of the one-process loss, the bar of tests/test_loss_gpu.py.  Steps 2 and 3
    are printed, not gated (Adam's first steps are ill-conditioned: DESIGN section 8o)."""
    got, want = [v for _, v in two_ranks["logged"]], [v for _, v in one_process["logged"]]
    assert [s for s, _ in two_ranks["logged"]] == [s for s, _ in one_process["logged"]] == [1, 2, 3]
    for step, (g, w) in enumerate(zip(got, want), 1):
        print(f"step {step}: two ranks log {g!r}, one process {w!r}, relative distance {abs(g - w) / abs(w):.3e}")
    print(f"three steps with summaries, validation and checkpoints: one process {one_process['seconds']:.1f} s, two ranks on one GPU over gloo "
          f"(process start included) {two_ranks['seconds']:.1f} s")
    assert abs(got[0] - want[0]) <= LOSS_TOL * abs(want[0])
    assert all(math.isfinite(g) for g in got)


def _first_moments(run):
    """Adam's exp_avg after step 1, by parameter index, and the number of depth parameters (the first group)."""
    state = torch.load(os.path.join(run["out"], "depth_model-1.pth"), map_location="cpu")["optimizer_state_dict"]
    n_depth = len(state["param_groups"][0]["params"])
    assert len(state["param_groups"]) == 2 and all(int(s["step"]) == 1 for s in state["state"].values())
    return {int(i): s["exp_avg"].double() for i, s in state["state"].items()}, n_depth


def _gate_fractions(run, reference):
    """Per parameter max |a - b| / (tol |b| + tol rms(b)): at most 1 passes.  -> (worst of the depth network, worst of the pose
    network, the parameters beyond the gate)."""
    got, n_depth = _first_moments(run)
    want, n_depth_want = _first_moments(reference)
    assert sorted(got) == sorted(want) and n_depth == n_depth_want and n_depth > 30 and len(want) - n_depth > 50
    worst, beyond = {"depth": 0.0, "pose": 0.0}, []
    for i, b in want.items():
        net, tol = ("depth", 2 * kgo.TOL) if i < n_depth else ("pose", 2 * rgo.TOL)
        a = got[i]
        assert a.shape == b.shape and torch.isfinite(a).all() and float(b.abs().max()) > 0, i
        bound = tol * b.abs() + tol * b.pow(2).mean().sqrt()
        fraction = float(((a - b).abs() / bound).max())
        worst[net] = max(worst[net], fraction)
        if not fraction <= 1.0:
            beyond.append((net, i, fraction))
    return worst["depth"], worst["pose"], beyond


def test_reduced_gradient_is_the_one_process_gradient(one_process, two_ranks):
    depth, pose, beyond = _gate_fractions(two_ranks, one_process)
    print(f"exp_avg after step 1, two ranks (2 + 1 frames) against one process: worst parameter at {depth:.3f} of the gate for the depth network "
          f"(tol {2 * kgo.TOL:.1e}), {pose:.3f} for the pose network (tol {2 * rgo.TOL:.1e})")
    assert not beyond, beyond[:10]


def test_a_shard_of_one_small_frame_has_no_statistics_of_its_own(dev, inputs, tmp_path):  # noqa: F811
    """sync_batch_norm=False on the 2 + 1 split of 24 x 40 frames: rank 1 cannot normalise its one frame's 1 x 1 maps, launch ends
    rank 0 and raises with rank 1's message.  Synchronised BatchNorm is what makes this split trainable at all."""
    started = time.time()
    with pytest.raises(kb._lib.KbnError, match=r"(?s)rank 1 of 2 exited with status 1.*one value per channel"):
        _launch(inputs, str(tmp_path / "trained"), sync_batch_norm=False)
    assert time.time() - started < TIMEOUT / 2      # the first failure ended the run, not the time limit
    assert not [n for n in os.listdir(str(tmp_path / "trained")) if n.endswith((".pth", ".digest"))]


def test_without_synchronised_batch_norm_the_gate_fails(four_frames):
    """The power of the gate above, on 2 + 2 frames: with synchronised BatchNorm it holds, per-shard statistics push pose parameters
    beyond it."""
    depth, pose, beyond = _gate_fractions(four_frames["two"], four_frames["one"])
    print(f"2 + 2 frames, synchronised: worst parameter at {depth:.3f} of the gate for the depth network, {pose:.3f} for the pose network")
    assert not beyond, beyond[:10]
    got, want = four_frames["two"]["logged"][0][1], four_frames["one"]["logged"][0][1]
    assert abs(got - want) <= LOSS_TOL * abs(want)
    depth, pose, beyond = _gate_fractions(four_frames["local"], four_frames["one"])
    print(f"2 + 2 frames, sync_batch_norm=False: worst parameter at {depth:.3f} of the gate for the depth network, {pose:.1f} for the pose network; "
          f"{sum(1 for net, _, _ in beyond if net == 'pose')} pose parameters beyond it (the depth network's gradient follows: it runs through the poses)")
    assert any(net == "pose" for net, _, _ in beyond), "the gate cannot tell synchronised BatchNorm from per-shard statistics"


def _digests(run):
    values = []
    for rank in range(2):
        with open(os.path.join(run["out"], f"rank{rank}.digest")) as f:
            values.append(f.read().strip())
    return values


def test_replicas_end_bit_identical(two_ranks, four_frames):
    """Each rank's digest of its final parameters, BatchNorm buffers and optimizer state."""
    a, b = _digests(two_ranks)
    assert len(a) == 64 and a == b == two_ranks["results"]["digest"]
    c, d = _digests(four_frames["two"])
    assert c == d and c != a
    e, f = _digests(four_frames["local"])
    assert e != f      # per-rank running statistics: the digest sees them


# ------------------------------------------------------------------------------------------------ a batch with fewer frames than ranks
def test_a_batch_of_one_frame_is_skipped_on_both_ranks(dev, inputs, tmp_path):  # noqa: F811
    """3 samples, batch 2: batches of 2 and 1 frames an epoch; the second gives rank 1 nothing and is no step."""
    run = _launch(inputs, str(tmp_path / "trained"), n_batch=2, validation_start_step=100)
    assert run["results"]["train_step"] == 3 and [s for s, _ in run["logged"]] == [1, 2, 3]
    lines = _lines(run)
    steps = [re.match(base.STEP, line).group(1) for line in lines if re.match(base.STEP, line)]
    assert steps == ["1", "2", "3"] and "n_sample=3  n_epoch=3  n_step=3" in lines      # one process counts 6
    assert sorted(n for n in os.listdir(run["out"]) if n.endswith(".pth")) == sorted(
        f"{model}_model-{step}.pth" for model in ("depth", "pose") for step in (1, 2, 3))
    a, b = _digests(run)
    assert a == b


# ------------------------------------------------------------------------------------------------ RCCL
def test_two_ranks_over_rccl(one_process, inputs, tmp_path):  # noqa: F811
    """The same comparison with rank r on cuda:r over RCCL.  One-GPU leases skip it, with the reason in the report (-rs)."""
    n = torch.cuda.device_count() if torch.cuda.is_available() else 0
    if n < 2:
        print(f"SKIP: {n} visible GPU(s); two ranks over RCCL need two devices (the gloo tests above run the same code on one)")
        pytest.skip(f"{n} visible GPU(s): two RCCL ranks need two devices")
    run = _launch(inputs, str(tmp_path / "trained"), backend="nccl", devices=(0, 1))
    got, want = [v for _, v in run["logged"]], [v for _, v in one_process["logged"]]
    assert abs(got[0] - want[0]) <= LOSS_TOL * abs(want[0])
    depth, pose, beyond = _gate_fractions(run, one_process)
    print(f"RCCL: worst parameter at {depth:.3f} of the gate for the depth network, {pose:.3f} for the pose network")
    assert not beyond, beyond[:10]
    a, b = _digests(run)
    assert a == b
    assert _lines(run)[:5] == _lines(one_process)[:5] and run["results"]["train_step"] == 3
