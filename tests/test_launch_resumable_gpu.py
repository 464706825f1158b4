"""GPU, two ranks: kb.training.launch_resumable, stopped three times and continued, against ONE uninterrupted kb.training.launch
under the same seeds -- bit for bit.

    python -m pytest tests/test_launch_resumable_gpu.py -m gpu -q -s

Two children share cuda:0 over gloo (devices=[0, 0]), never more than two at a time, each launch under a time limit of 300 s.  The
run is the one of tests/test_train_resumable_gpu.py, whose list, settings and comparisons are imported: 12 listed samples, batch 2
(shards 1 + 1), a free 24 x 40 crop, both flips, point removal, gaussian noise, two epochs of six steps with the rates [1e-4, 5e-5],
a checkpoint, a summary and a validation every four steps, default writers.  The sessions, every generator of the launcher re-seeded
with other values before each (the children start from the launcher's random state):

    1   max_steps=1: stops after step 1, mid-epoch, the plans of the batches in flight stored;
    2   max_steps=5: stops after step 6, the epoch's last batch; the rate change lands on step 7;
    3   no limit; a thread of the test waits for train_state-8.pth and then sends SIGTERM to this process -- the launcher, which
        sends it on.  The session must return finished=False at a step s with 8 < s < 12; a run that ended first FAILS the test
        (the signal came too late), it never passes without a stop.  The equalities hold for any such s;
    4   no limit, to step 12;
    5   a fifth call returns at once and moves no mtime; a sixth with sync_batch_norm=False raises KbnError naming it.

Proof of power: the directory as it stands after session 1, continued to the end with (a) the state's NumPy generator state
replaced, (b) the crop origins of the state's stored loader plans drawn again -- each must end in another depth_model-12.pth than
the uninterrupted run's.  Seven two-rank launches in all."""
import os
import re
import shutil
import signal
import threading
import time

import numpy as np
import pytest
import torch

import kbnet_amd as kb
import test_train_resumable_gpu as one
from test_train_gpu import inputs  # noqa: F401  (the fixture `case` is built from)
from test_train_resumable_gpu import case  # noqa: F401  (the fixture: the run's lists and settings)

pytestmark = pytest.mark.gpu

KbnError = kb._lib.KbnError
training = kb.training
TIMEOUT = 300      # seconds a launch may take: a collective that waits for a rank that left ends here
N_STEP, GRID = one.N_STEP, one.GRID


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    kb._lib.load()
    return torch.device("cuda:0")


def _arguments(case, out, **more):  # noqa: F811
    arguments = dict(zip(training.PATH_ARGUMENTS, case["positional"]))
    arguments.update(case["settings"], checkpoint_path=out, depth_model_restore_path=case["depth"], pose_model_restore_path=case["pose"],
                     device="cuda", workers=2)
    arguments.update(more)
    return arguments


def _launch(function, case, out, seed, **more):  # noqa: F811
    one._seed(seed)      # the children start from the caller's random state
    return function(2, backend="gloo", devices=[0, 0], timeout=TIMEOUT, **_arguments(case, out, **more))


def _digests(out):
    values = []
    for rank in range(2):
        with open(os.path.join(out, f"rank{rank}.digest")) as f:
            values.append(f.read().strip())
    return values


@pytest.fixture(scope="module")
def yardstick(dev, case, tmp_path_factory):  # noqa: F811
    """The uninterrupted run: kb.training.launch, existing code."""
    out = str(tmp_path_factory.mktemp("launch_resumable_yardstick") / "trained")
    started = time.time()
    results, logged, checkpoints = _launch(training.launch, case, out, 0)
    return {"out": out, "results": results, "logged": logged, "checkpoints": checkpoints, "seconds": time.time() - started}


@pytest.fixture(scope="module")
def sessions(dev, case, tmp_path_factory):  # noqa: F811
    root = tmp_path_factory.mktemp("launch_resumable_sessions")
    out = str(root / "trained")
    returned, listings, digests = [], [], []

    def session(seed, **more):
        returned.append(_launch(training.launch_resumable, case, out, seed, **more))
        listings.append(sorted(one._listing(out)))
        digests.append(_digests(out))

    session(0, max_steps=1)
    shutil.copytree(out, str(root / "after_1"))
    session(101, max_steps=5)

    # the third session: SIGTERM to the launcher once the state of step 8 lies in place
    late, sent, stop_watching = [], [], threading.Event()
    fallback = signal.signal(signal.SIGTERM, lambda number, frame: late.append(number))      # one that arrives after the return ends nobody
    handler = signal.getsignal(signal.SIGTERM)

    def watch():
        path = os.path.join(out, "train_state-8.pth")
        while not stop_watching.is_set():
            if os.path.exists(path):
                sent.append(time.time())
                os.kill(os.getpid(), signal.SIGTERM)
                return
            time.sleep(0.002)

    watcher = threading.Thread(target=watch)
    try:
        watcher.start()
        session(202)
        back = time.time()
    finally:
        stop_watching.set()
        watcher.join()
        handler_after = signal.getsignal(signal.SIGTERM)
        signal.signal(signal.SIGTERM, fallback)

    session(303)

    before = one._listing(out)
    fifth = _launch(training.launch_resumable, case, out, 404)
    after_fifth = one._listing(out)
    refused = None
    try:
        _launch(training.launch_resumable, case, out, 505, sync_batch_norm=False)
    except KbnError as e:
        refused = str(e)
    return {"out": out, "returned": returned, "listings": listings, "digests": digests, "fifth": fifth, "before_fifth": before,
            "after_fifth": after_fifth, "refused": refused, "after_refused": one._listing(out), "after_1": str(root / "after_1"),
            "late": late, "sent": sent, "stop_seconds": (back - sent[0]) if sent else None, "handlers": (handler, handler_after)}


# ------------------------------------------------------------------------------------------------ the sessions themselves
def test_sessions_stop_where_they_should(sessions, yardstick):
    steps = [(r[0]["train_step"], r[0]["finished"], r[0]["resumed_from"]) for r in sessions["returned"]]
    third = steps[2][0]
    assert sessions["sent"], "train_state-8.pth never appeared while the third session ran"
    assert not sessions["late"] and steps[2][1] is False, f"the signal came too late: the third session returned {steps[2]} before it arrived"
    assert 8 < third < 12, steps
    assert steps == [(1, False, None), (6, False, 1), (third, False, 6), (12, True, third)]
    assert sessions["handlers"][0] == sessions["handlers"][1]      # the caller's SIGTERM handler is back
    print(f"the third session stopped after step {third}; from the signal to the launcher's return {sessions['stop_seconds'] * 1e3:.0f} ms "
          f"(two ranks on one GPU over gloo, the launcher's 50 ms poll and the children's exit included); the uninterrupted launch took "
          f"{yardstick['seconds']:.1f} s")
    assert yardstick["results"]["train_step"] == N_STEP and [s for s, _ in yardstick["logged"]] == list(GRID)
    names = [[os.path.basename(p) for p in r[2]] for r in sessions["returned"]]
    stop = [f"depth_model-{third}.pth", f"pose_model-{third}.pth"]
    assert names == [["depth_model-1.pth", "pose_model-1.pth"],
                     ["depth_model-4.pth", "pose_model-4.pth", "depth_model-6.pth", "pose_model-6.pth"],
                     ["depth_model-8.pth", "pose_model-8.pth"] + stop, ["depth_model-12.pth", "pose_model-12.pth"]]


def test_replicas_are_bit_identical_after_every_session(sessions, yardstick):
    assert len(sessions["digests"]) == 4
    for (a, b), returned in zip(sessions["digests"], sessions["returned"]):
        assert len(a) == 64 and a == b == returned[0]["digest"]
    assert len({a for a, _ in sessions["digests"]}) == 4
    assert sessions["digests"][-1] == _digests(yardstick["out"])      # and the run ends where the uninterrupted one does


def test_rank_0_alone_writes_and_states_are_pruned(sessions):
    third = sessions["returned"][2][0]["train_step"]
    pth = lambda listing: [n for n in listing if n.endswith(".pth")]
    models = lambda steps: [f"{m}_model-{s}.pth" for m in ("depth", "pose") for s in steps]
    states = lambda steps: [f"train_state-{s}.pth" for s in steps]
    first, second, third_listing, fourth = (pth(listing) for listing in sessions["listings"])
    assert first == sorted(models([1]) + states([1]))
    assert second == sorted(models([4, 6]) + states([4, 6]))
    assert third_listing == sorted(models([4, 8, third]) + states([8, third]))      # keep_states=2
    assert fourth == sorted(models([4, 8, third, 12]) + states([third, 12]))      # a stop's checkpoints stay as long as its state
    assert len([n for n in fourth if n.startswith("train_state-")]) == 2      # exactly keep_states states
    last = sessions["listings"][-1]
    assert not [n for n in last if n.endswith(".part")]
    # every file is one rank 0 or the launcher writes, or one of the ranks' own three
    known = {"results.txt", "launch-arguments.pkl", "launch-results.pkl"} | {f"rank{r}.{kind}" for r in range(2) for kind in ("out", "err", "digest")}
    assert [n for n in last if n not in known and not n.endswith(".pth") and not n.startswith(("events-train" + os.sep, "events-val" + os.sep))] == []
    for which in ("events-train", "events-val"):
        assert len([n for n in last if n.startswith(which + os.sep)]) == 4      # a file a session: rank 0's alone
    with open(os.path.join(sessions["out"], "rank0.out")) as f:
        first_rank = f.read().splitlines()
    with open(os.path.join(sessions["out"], "rank1.out")) as f:
        second_rank = f.read().splitlines()
    marks = ["==== launch_resumable: a session from the start ===="] + [f"==== launch_resumable: a session after step {s} ====" for s in (1, 6, third)]
    assert [line for line in first_rank if line.startswith("====")] == marks      # appended to, a line a session
    assert [line for line in second_rank if line.startswith("====")] == marks
    # rank 1 keeps no log: what it prints is the backend's and validate()'s console lines
    assert not [line for line in second_rank if line.startswith(("Begin training", "Resuming training", "Step=", "Skipping ", "n_batch="))]
    assert sum(1 for line in first_rank if line.startswith("Resuming training")) == 3 and first_rank.count("Begin training...") == 1


def test_a_fifth_call_returns_at_once_and_a_sixth_is_refused(sessions):
    results, logged, checkpoints = sessions["fifth"]
    last = sessions["returned"][-1]
    assert results["finished"] is True and results["train_step"] == N_STEP and results["resumed_from"] == N_STEP
    assert results["digest"] == last[0]["digest"] and results["best_results"] == last[0]["best_results"]
    assert logged == last[1] and checkpoints == []
    assert sessions["after_fifth"] == sessions["before_fifth"]      # no new file, no mtime moved
    assert sessions["refused"] is not None and re.search(r"sync_batch_norm is False.*started with True", sessions["refused"])
    assert sessions["after_refused"] == sessions["before_fifth"]


# ------------------------------------------------------------------------------------------------ bit for bit
@pytest.mark.parametrize("step", GRID)
def test_checkpoints_equal_the_uninterrupted_runs(sessions, yardstick, step):
    for model in ("depth", "pose"):
        name = f"{model}_model-{step}.pth"
        got, want = one._checkpoint(sessions["out"], name), one._checkpoint(yardstick["out"], name)
        differing = one._differing(got, want)
        assert not differing, (name, differing[:5])
        moments = [k for k in want if k.endswith(("exp_avg", "exp_avg_sq"))]
        counts = [k for k in want if k.startswith("/optimizer_state_dict/state/") and k.endswith("/step")]
        assert len(moments) > 100 and len(counts) > 50 and all(float(want[k]) == step for k in counts)
        lrs = [want[k] for k in want if re.match(r"^/optimizer_state_dict/param_groups/\d+/lr$", k)]
        assert lrs == [1e-4 if step <= 6 else 5e-5] * 2
        if model == "pose":
            assert [k for k in want if k.endswith(("running_mean", "running_var"))] and [k for k in want if k.endswith("num_batches_tracked")]


def test_results_and_logged_losses_are_equal(sessions, yardstick):
    last = sessions["returned"][-1]
    assert last[0]["best_results"] == yardstick["results"]["best_results"] and last[0]["best_results"]["step"] in GRID
    assert last[1] == yardstick["logged"] and [s for s, _ in last[1]] == list(GRID)
    assert sessions["returned"][1][1] == yardstick["logged"][:1] and sessions["returned"][2][1] == yardstick["logged"][:2]


def test_results_txt(sessions, yardstick):
    third = sessions["returned"][2][0]["train_step"]
    got, want = one._lines(sessions["out"]), one._lines(yardstick["out"])
    assert one._masked(got) == one._masked(want) and len(one._masked(want)) == 3 * (1 + 6)
    assert [line for line in got if line.startswith("Resuming training")] == [f"Resuming training from step {s}..." for s in (1, 6, third)]
    for once in ("Training input paths:", "Validation input paths:", "Begin training...", "Training settings:"):
        assert got.count(once) == 1, once
    strip = lambda lines, out: [re.sub(one.STEP, r"\1", line).replace(out, "<out>") for line in lines]
    assert [line for line in strip(got, sessions["out"]) if not line.startswith("Resuming training")] == strip(want, yardstick["out"])


@pytest.mark.parametrize("which", ["train", "val"])
def test_events_of_all_sessions_equal_the_uninterrupted_runs(sessions, yardstick, which):
    got = one._events(os.path.join(sessions["out"], "events-" + which))
    want = one._events(os.path.join(yardstick["out"], "events-" + which))
    assert len(os.listdir(os.path.join(yardstick["out"], "events-" + which))) == 1
    assert [(e["kind"], e["tag"], e["step"]) for e in got] == [(e["kind"], e["tag"], e["step"]) for e in want]
    assert {e["step"] for e in want} == set(GRID) and {e["kind"] for e in want} == {"scalar", "histo", "image"}
    differing = [(e["tag"], e["step"]) for e, w in zip(got, want) if not one._same_value(w["kind"], e["value"], w["value"])]
    assert not differing, differing[:5]


# ------------------------------------------------------------------------------------------------ proof of power
def _continue_harmed(case, source, directory, harm):  # noqa: F811
    shutil.copytree(source, directory)
    path = os.path.join(directory, "train_state-1.pth")
    state = torch.load(path, map_location="cpu")
    harm(state)
    torch.save(state, path)
    results, _, _ = _launch(training.launch_resumable, case, directory, 777)
    assert results["finished"] and results["train_step"] == N_STEP and results["resumed_from"] == 1
    a, b = _digests(directory)
    assert a == b      # the ranks read one state alike: harmed, they still train as one
    return one._checkpoint(directory, "depth_model-12.pth")


def test_power_without_numpys_state(sessions, yardstick, case, tmp_path):  # noqa: F811
    def harm(state):
        name, keys, position, has_gauss, cached_gaussian = state["random"]["numpy"]
        other = np.random.RandomState(4321).get_state()
        state["random"]["numpy"] = (name, torch.from_numpy(other[1].astype(np.int64)), int(other[2]), int(other[3]), float(other[4]))

    got = _continue_harmed(case, sessions["after_1"], str(tmp_path / "trained"), harm)
    differing = one._differing(got, one._checkpoint(yardstick["out"], "depth_model-12.pth"))
    assert len(differing) > 50, len(differing)


def test_power_without_the_loaders_stored_plans(sessions, yardstick, case, tmp_path):  # noqa: F811
    moved = []

    def harm(state):
        """The crop origins of the batches in flight, drawn again: what a continuation without the stored plans would do."""
        plans = state["loader"]["plans"]
        assert len(plans) == 4      # batches 1-4 were planned ahead of step 1's draws; batch 5 was still to draw
        np.random.seed(99)
        for p, (frames, shape, c, dbits, cropped) in enumerate(plans):
            assert len(frames) == 2 and cropped      # the plans of whole global batches
            drawn = [(i, hh, ww) + kb.loader.draw_crop(hh, ww, shape, case["settings"]["augmentation_random_crop_type"]) for i, hh, ww, _, _ in frames]
            moved.extend(tuple(a) != tuple(b) for a, b in zip(drawn, frames))
            plans[p] = (drawn, shape, c, dbits, cropped)

    got = _continue_harmed(case, sessions["after_1"], str(tmp_path / "trained"), harm)
    assert len(moved) == 8 and sum(moved) >= 2, moved
    differing = one._differing(got, one._checkpoint(yardstick["out"], "depth_model-12.pth"))
    assert len(differing) > 50, len(differing)
