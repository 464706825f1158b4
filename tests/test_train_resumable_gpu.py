"""GPU: kb.training.train_resumable, stopped three times and continued, against ONE uninterrupted kb.training.train under the same
seeds -- bit for bit.

    python -m pytest tests/test_train_resumable_gpu.py -m gpu -q -s

The run has teeth in every generator: 12 listed samples (triplets of tests/golden/train_io in a fixed mixed order), batch 2, a free
24 x 40 crop ('horizontal', 'vertical'), two epochs of six steps with the rates [1e-4, 5e-5], augmentation probability 1 with both
flips, point removal and gaussian noise, a checkpoint, a summary and a validation every four steps.  The sessions stop after

    step 1     max_steps=1: the middle of an epoch, the loader's default prefetch of 4 has the plans of batches 1-4 drawn and batch
               5 still to draw;
    step 6     SIGTERM, raised in-process while step 6 runs: the epoch's last batch, the rate change lands on step 7;
    step 8     SIGTERM, raised in-process by the train writer's add_scalar in step 8's summary: a grid step, the regular
               checkpoint's state is the stop's (max_steps=3 stands behind it: a signal that did nothing would show as a stop at 9);
    step 12    the end.

Two things the issue's text asks for cannot be had as written, and are mended so that no less is asked.  (1) triplet_0 and
triplet_3 ARE 24 x 40: an unanchored 'horizontal' crop of that size does not exist for them (draw_crop raises NumPy's ValueError,
as the reference does), so the list takes the two triplets with room for the crop, 26 x 44 and 25 x 43, six times each; the
validation runs over those two files at their raw sizes.  (2) with n_summary=4 no writer method is called at step 6, so the
signal of the second session is raised from a wrapper around kb.transforms.train_inputs (called once a step) on that session's
fifth step; the writer whose add_scalar raises the signal -- the issue's mechanism -- stops the third session, where a summary
exists.  No process is killed.

Between the sessions every generator is re-seeded with other values: what a continuation draws comes from the state file alone.

Proof of power: the directory as it stands after the stop at step 6, continued to the end without (a) NumPy's state, (b)
Transforms.calls, and the directory after the stop at step 1 continued with (c) the loader's stored plans dropped and re-drawn --
each must end in another depth_model-12.pth than the uninterrupted run's."""
import os
import re
import shutil
import signal

import numpy as np
import pytest
import torch

import kbnet_amd as kb
from conftest import GOLDEN_DIR
import event_cases as ec
from test_train_gpu import inputs  # noqa: F401  (the fixture: the depth and pose checkpoints and the narrow KITTI settings)

pytestmark = pytest.mark.gpu

KbnError = kb._lib.KbnError
IO = os.path.join(GOLDEN_DIR, "train_io")
ORDER = [1, 2, 2, 1, 2, 1, 1, 1, 2, 2, 1, 2]      # the 26 x 44 and the 25 x 43 triplet, six times each
N_STEP, GRID = 12, (4, 8, 12)
STEP = r"^(Step=\s+\d+/12  Loss=\d+\.\d{5})  Time Elapsed=\d+\.\d{2}h  Time Remaining=\d+\.\d{2}h$"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    kb._lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def case(inputs, tmp_path_factory):  # noqa: F811
    root = tmp_path_factory.mktemp("resumable_inputs")
    lists = {}
    for name, pattern, order in (("image", "triplet_{}.png", ORDER), ("sparse_depth", "depth_{}.png", ORDER), ("intrinsics", "k_{}.npy", ORDER),
                                 ("val_image", "triplet_{}.png", [1, 2]), ("val_sparse_depth", "depth_{}.png", [1, 2]),
                                 ("val_intrinsics", "k_{}.npy", [1, 2])):
        lists[name] = str(root / (name + ".txt"))
        with open(lists[name], "w") as f:
            f.write("\n".join(os.path.join(IO, pattern.format(i)) for i in order) + "\n")
    settings = dict(inputs["settings"], n_batch=2, n_height=24, n_width=40, augmentation_random_crop_type=["horizontal", "vertical"],
                    learning_schedule=[1, 2], learning_rates=[1e-4, 5e-5], augmentation_probabilities=[1.0], augmentation_schedule=[-1],
                    augmentation_random_flip_type=["horizontal", "vertical"], augmentation_random_remove_points=[0.60, 0.70],
                    augmentation_random_noise_type="gaussian", augmentation_random_noise_spread=0.5, n_checkpoint=4, n_summary=4,
                    validation_start_step=4)
    positional = [lists["image"], lists["sparse_depth"], lists["intrinsics"], lists["val_image"], lists["val_sparse_depth"],
                  lists["val_intrinsics"], lists["val_sparse_depth"]]      # the sparse depth as ground truth
    return {"positional": positional, "settings": settings, "depth": inputs["depth"], "pose": inputs["pose"]}


def _seed(value=0):
    torch.manual_seed(value)
    np.random.seed(value)


def _call(function, case, out, **more):
    return function(*case["positional"], checkpoint_path=out, depth_model_restore_path=case["depth"], pose_model_restore_path=case["pose"],
                    device="cuda", workers=2, return_results=True, **dict(case["settings"], **more))


@pytest.fixture(scope="module")
def yardstick(dev, case, tmp_path_factory):
    """The uninterrupted run: kb.training.train, existing code."""
    out = str(tmp_path_factory.mktemp("resumable_yardstick") / "trained")
    _seed()
    results, logged, checkpoints = _call(kb.training.train, case, out)
    return {"out": out, "results": results, "logged": logged, "checkpoints": checkpoints}


class _SignallingWriter(kb.summary.EventWriter):
    """The default writer, but its add_scalar raises SIGTERM in this process when it is called for step 8."""

    def add_scalar(self, tag, scalar_value, global_step=None):
        if global_step == 8 and tag.startswith("train_"):
            signal.raise_signal(signal.SIGTERM)
        return super().add_scalar(tag, scalar_value, global_step=global_step)


def _listing(directory):
    found = {}
    for base, _, names in os.walk(directory):
        for name in names:
            path = os.path.join(base, name)
            found[os.path.relpath(path, directory)] = os.stat(path).st_mtime_ns
    return found


@pytest.fixture(scope="module")
def sessions(dev, case, tmp_path_factory):
    """The same run in four sessions and a fifth call; copies of the directory after the first and the second stop."""
    root = tmp_path_factory.mktemp("resumable_sessions")
    out = str(root / "trained")
    handler = signal.getsignal(signal.SIGTERM)
    returned, listings = [], []

    _seed()
    returned.append(_call(kb.training.train_resumable, case, out, max_steps=1))
    shutil.copytree(out, str(root / "after_1"))
    listings.append(sorted(_listing(out)))

    _seed(101)
    real, calls = kb.transforms.train_inputs, []

    def signalling_train_inputs(*args, **kwargs):
        calls.append(1)
        if len(calls) == 5:      # the session's fifth step is step 6
            signal.raise_signal(signal.SIGTERM)
        return real(*args, **kwargs)

    kb.transforms.train_inputs = signalling_train_inputs
    try:
        returned.append(_call(kb.training.train_resumable, case, out))
    finally:
        kb.transforms.train_inputs = real
    shutil.copytree(out, str(root / "after_6"))
    listings.append(sorted(_listing(out)))

    _seed(202)
    returned.append(_call(kb.training.train_resumable, case, out, max_steps=3, summary_writer_factory=_SignallingWriter))
    listings.append(sorted(_listing(out)))

    _seed(303)
    returned.append(_call(kb.training.train_resumable, case, out))
    listings.append(sorted(_listing(out)))

    before = _listing(out)
    _seed(404)
    fifth = _call(kb.training.train_resumable, case, out)
    return {"out": out, "returned": returned, "listings": listings, "fifth": fifth, "before_fifth": before, "after_fifth": _listing(out),
            "after_1": str(root / "after_1"), "after_6": str(root / "after_6"), "handlers": (handler, signal.getsignal(signal.SIGTERM)),
            "train_inputs_calls": len(calls)}


def _tensors(value, prefix=""):
    """Every tensor of a checkpoint by its path through the dicts and lists, and every other leaf."""
    if torch.is_tensor(value):
        yield prefix, value
    elif isinstance(value, dict):
        for key in value:
            yield from _tensors(value[key], f"{prefix}/{key}")
    elif isinstance(value, (list, tuple)):
        for i, item in enumerate(value):
            yield from _tensors(item, f"{prefix}/{i}")
    else:
        yield prefix, value


def _checkpoint(directory, name):
    return dict(_tensors(torch.load(os.path.join(directory, name), map_location="cpu")))


def _differing(a, b):
    assert sorted(a) == sorted(b)
    return [k for k in a if not (torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k])]


# ------------------------------------------------------------------------------------------------ the sessions themselves
def test_sessions_stop_where_they_should(sessions, yardstick):
    steps = [(r[0]["train_step"], r[0]["finished"], r[0]["resumed_from"]) for r in sessions["returned"]]
    assert steps == [(1, False, None), (6, False, 1), (8, False, 6), (12, True, 8)]
    assert sessions["train_inputs_calls"] == 5      # the step the signal arrived in was completed, and none begun after it
    assert yardstick["results"]["train_step"] == N_STEP and [s for s, _ in yardstick["logged"]] == list(GRID)
    assert sessions["handlers"][0] == sessions["handlers"][1]      # the caller's SIGTERM handler is back
    # the checkpoint paths are each session's own
    names = [[os.path.basename(p) for p in r[2]] for r in sessions["returned"]]
    assert names == [["depth_model-1.pth", "pose_model-1.pth"],
                     ["depth_model-4.pth", "pose_model-4.pth", "depth_model-6.pth", "pose_model-6.pth"],
                     ["depth_model-8.pth", "pose_model-8.pth"], ["depth_model-12.pth", "pose_model-12.pth"]]
    digests = [r[0]["digest"] for r in sessions["returned"]]
    assert all(len(d) == 64 for d in digests) and len(set(digests)) == 4


def test_states_and_stop_checkpoints_are_pruned(sessions):
    pth = lambda listing: [n for n in listing if n.endswith(".pth")]
    models = lambda steps: [f"{m}_model-{s}.pth" for m in ("depth", "pose") for s in steps]
    states = lambda steps: [f"train_state-{s}.pth" for s in steps]
    one, two, three, four = (pth(listing) for listing in sessions["listings"])
    assert one == sorted(models([1]) + states([1]))
    assert two == sorted(models([4, 6]) + states([4, 6]))            # keep_states=2: step 1 went, with its off-grid checkpoints
    assert three == sorted(models([4, 6, 8]) + states([6, 8]))       # step 4's state went, its grid checkpoints stay
    assert four == sorted(models([4, 8, 12]) + states([8, 12]))      # step 6's checkpoints went with its state
    assert not [n for n in sessions["listings"][-1] if n.endswith(".part")]
    for which in ("events-train", "events-val"):
        assert len([n for n in sessions["listings"][-1] if n.startswith(which + os.sep)]) == 4      # a file a session


def test_a_fifth_call_returns_at_once_and_touches_nothing(sessions):
    results, logged, checkpoints = sessions["fifth"]
    last = sessions["returned"][-1]
    assert results["finished"] is True and results["train_step"] == N_STEP and results["resumed_from"] == N_STEP
    assert results["digest"] == last[0]["digest"] and results["best_results"] == last[0]["best_results"]
    assert logged == last[1] and checkpoints == []
    assert sessions["after_fifth"] == sessions["before_fifth"]      # no new file, no mtime moved


# ------------------------------------------------------------------------------------------------ bit for bit
@pytest.mark.parametrize("step", GRID)
def test_checkpoints_equal_the_uninterrupted_runs(sessions, yardstick, step):
    for model in ("depth", "pose"):
        name = f"{model}_model-{step}.pth"
        got, want = _checkpoint(sessions["out"], name), _checkpoint(yardstick["out"], name)
        assert not _differing(got, want), (name, _differing(got, want)[:5])
        moments = [k for k in want if k.endswith(("exp_avg", "exp_avg_sq"))]
        counts = [k for k in want if k.startswith("/optimizer_state_dict/state/") and k.endswith("/step")]
        assert len(moments) > 100 and len(counts) > 50 and all(float(want[k]) == step for k in counts)
        lrs = [want[k] for k in want if re.match(r"^/optimizer_state_dict/param_groups/\d+/lr$", k)]
        assert lrs == [1e-4 if step <= 6 else 5e-5] * 2
        if model == "pose":
            tracked = [k for k in want if k.endswith("num_batches_tracked")]
            running = [k for k in want if k.endswith(("running_mean", "running_var"))]
            assert tracked and running and all(int(want[k]) >= step for k in tracked)


def test_results_and_logged_losses_are_equal(sessions, yardstick):
    last = sessions["returned"][-1]
    assert last[0]["best_results"] == yardstick["results"]["best_results"] and last[0]["best_results"]["step"] in GRID
    assert last[1] == yardstick["logged"] and [s for s, _ in last[1]] == list(GRID)
    assert sessions["returned"][1][1] == yardstick["logged"][:1] and sessions["returned"][2][1] == yardstick["logged"][:2]


def _lines(directory):
    with open(os.path.join(directory, "results.txt")) as f:
        return f.read().splitlines()


def _masked(lines):
    """The Step= lines without their times, and the validation blocks (five lines from each 'Validation results:' on, and the
    three of 'Best results:')."""
    out, keep = [], 0
    for line in lines:
        m = re.match(STEP, line)
        if m:
            out.append(m.group(1))
        elif line in ("Validation results:", "Best results:"):
            keep = 3
        if keep:
            out.append(line)
            keep -= 1
    return out


def test_results_txt(sessions, yardstick):
    got, want = _lines(sessions["out"]), _lines(yardstick["out"])
    assert _masked(got) == _masked(want) and len(_masked(want)) == 3 * (1 + 6)
    assert sum(1 for line in want if re.match(STEP, line)) == 3
    resuming = [line for line in got if line.startswith("Resuming training")]
    assert resuming == [f"Resuming training from step {s}..." for s in (1, 6, 8)]
    for once in ("Training input paths:", "Validation input paths:", "Begin training...", "Training settings:"):
        assert got.count(once) == 1, once
    # nothing but the three Resuming lines sets the two files apart, times and the directory's name aside
    strip = lambda lines, out: [re.sub(STEP, r"\1", line).replace(out, "<out>") for line in lines]
    assert [line for line in strip(got, sessions["out"]) if not line.startswith("Resuming training")] == strip(want, yardstick["out"])


def _events(directory):
    found = []
    for name in sorted(os.listdir(directory)):
        records = ec.read_events(os.path.join(directory, name))
        assert records[0]["file_version"] == "brain.Event:2"
        found += records[1:]
    return sorted(found, key=lambda e: e["step"])      # stable: the order inside a step is the file's


def _same_value(kind, a, b):
    if kind == "histo":
        return sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    return a == b


@pytest.mark.parametrize("which", ["train", "val"])
def test_events_of_all_sessions_equal_the_uninterrupted_runs(sessions, yardstick, which):
    got = _events(os.path.join(sessions["out"], "events-" + which))
    want = _events(os.path.join(yardstick["out"], "events-" + which))
    assert len(os.listdir(os.path.join(yardstick["out"], "events-" + which))) == 1
    assert [(e["kind"], e["tag"], e["step"]) for e in got] == [(e["kind"], e["tag"], e["step"]) for e in want]
    assert {e["step"] for e in want} == set(GRID) and {e["kind"] for e in want} == {"scalar", "histo", "image"}
    differing = [(e["tag"], e["step"]) for e, w in zip(got, want) if not _same_value(w["kind"], e["value"], w["value"])]
    assert not differing, differing[:5]


# ------------------------------------------------------------------------------------------------ proof of power
def _continue(case, directory):
    _seed(777)
    results, _, _ = _call(kb.training.train_resumable, case, os.path.join(directory))
    assert results["finished"] and results["train_step"] == N_STEP
    return _checkpoint(directory, "depth_model-12.pth")


def test_an_unharmed_copy_ends_equal_and_a_changed_argument_is_refused(sessions, yardstick, case, tmp_path):
    """The control of the three tests below: the copy of the step-6 directory, continued as it is, ends bit-equal -- the copy, the
    re-seeding and another checkpoint_path are not what makes the others differ -- here with a newer state beside it that is cut
    short: it is passed over with a log line and removed with the next state written.  And before that: a continuation with
    another setting is refused by name and writes nothing."""
    directory = str(tmp_path / "trained")
    shutil.copytree(sessions["after_6"], directory)
    before = _listing(directory)
    for changed, name in ((dict(n_batch=3), "n_batch"), (dict(learning_rates=[1e-4, 4e-5]), "learning_rates"),
                          (dict(augmentation_random_noise_spread=0.25), "augmentation_random_noise_spread")):
        with pytest.raises(KbnError, match=f"train_resumable: {name} is "):
            _call(kb.training.train_resumable, case, directory, **changed)
    assert _listing(directory) == before
    # a job killed while it wrote under the final name would leave this: a newer state that does not load, its checkpoints there
    for name in ("depth_model-7.pth", "pose_model-7.pth"):
        shutil.copy(os.path.join(directory, name.replace("-7", "-6")), os.path.join(directory, name))
    with open(os.path.join(directory, "train_state-6.pth"), "rb") as f:
        whole = f.read()
    with open(os.path.join(directory, "train_state-7.pth"), "wb") as f:
        f.write(whole[:len(whole) // 2])
    got = _continue(case, directory)
    assert not _differing(got, _checkpoint(yardstick["out"], "depth_model-12.pth"))
    lines = _lines(directory)
    skipping = [i for i, line in enumerate(lines) if line.startswith("Skipping ") and "train_state-7.pth" in line]
    assert len(skipping) == 1 and lines[skipping[0] + 1] == "Resuming training from step 6..."
    assert sorted(n for n in os.listdir(directory) if n.endswith(".pth")) == sorted(
        [f"{m}_model-{s}.pth" for m in ("depth", "pose") for s in (4, 8, 12)] + ["train_state-8.pth", "train_state-12.pth"])


def test_power_without_numpys_state(sessions, yardstick, case, tmp_path, monkeypatch):
    directory = str(tmp_path / "trained")
    shutil.copytree(sessions["after_6"], directory)
    monkeypatch.setattr(np.random, "set_state", lambda state: None)
    got = _continue(case, directory)
    differing = _differing(got, _checkpoint(yardstick["out"], "depth_model-12.pth"))
    assert len(differing) > 50, len(differing)


def test_power_without_the_transforms_call_count(sessions, yardstick, case, tmp_path, monkeypatch):
    directory = str(tmp_path / "trained")
    shutil.copytree(sessions["after_6"], directory)
    real = kb.transforms.Transforms.load_state_dict
    monkeypatch.setattr(kb.transforms.Transforms, "load_state_dict", lambda self, state: real(self, dict(state, calls=0)))
    got = _continue(case, directory)
    differing = _differing(got, _checkpoint(yardstick["out"], "depth_model-12.pth"))
    assert len(differing) > 50, len(differing)


def test_power_without_the_loaders_stored_plans(sessions, yardstick, case, tmp_path, monkeypatch):
    directory = str(tmp_path / "trained")
    shutil.copytree(sessions["after_1"], directory)
    real = kb.loader.TrainingFrameLoader.load_state_dict
    dropped = []

    def without_plans(self, state):
        real(self, state)
        dropped.append(len(self._resume["plans"]))
        self._resume["plans"] = []      # the crops of the batches in flight are drawn again, from the restored generator

    monkeypatch.setattr(kb.loader.TrainingFrameLoader, "load_state_dict", without_plans)
    got = _continue(case, directory)
    assert dropped == [4]      # batches 1-4 were planned ahead of step 1's draws; batch 5 was still to draw
    differing = _differing(got, _checkpoint(yardstick["out"], "depth_model-12.pth"))
    assert len(differing) > 50, len(differing)


# ------------------------------------------------------------------------------------------------ the loader's state on its own
def _loader(dev, **more):
    paths = [[os.path.join(IO, pattern.format(i)) for i in ORDER[:9]] for pattern in ("triplet_{}.png", "depth_{}.png", "k_{}.npy")]
    arguments = dict(shape=(24, 40), random_crop_type=["horizontal", "vertical"], batch_size=2, shuffle=True, device=dev, workers=2)
    arguments.update(more)
    return kb.loader.TrainingFrameLoader(*paths, **arguments)


def _same_batches(got, want):
    return len(got) == len(want) and all(len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b)) for a, b in zip(got, want))


@pytest.mark.parametrize("prefetch,taken", [(4, 1), (4, 3), (2, 2), (1, 4), (8, 2)])
def test_loader_state_continues_an_epoch(dev, prefetch, taken, tmp_path):
    """Nine samples, batch 2: five batches, the last short.  Between the batches the thread draws from np.random as Transforms.draw
    does; a new loader given the state and the generator's state yields the rest of the epoch, and the next epoch, bit for bit."""
    def epochs(loader, stop=None):
        out = []
        for epoch in range(2):
            for b, batch in enumerate(loader):
                out.append([t.clone() for t in batch])
                np.random.rand(3)
                if stop is not None and epoch == 0 and b + 1 == stop:
                    return out
        return out

    _seed(5)
    want = epochs(_loader(dev, prefetch=prefetch))
    assert len(want) == 10 and want[4][0].shape[0] == 1
    assert _loader(dev, prefetch=prefetch).state_dict() == {}      # before the first epoch

    _seed(5)
    first = _loader(dev, prefetch=prefetch)
    head = epochs(first, stop=taken)
    state = first.state_dict()
    generators = (np.random.get_state(), torch.get_rng_state())
    assert state["next"] == taken and len(state["plans"]) == min(prefetch, 5 - taken) and len(state["order"]) == 9
    torch.save(state, str(tmp_path / "state.pth"))      # through a file, as a training state goes
    state = torch.load(str(tmp_path / "state.pth"), map_location="cpu")

    _seed(6)
    second = _loader(dev, prefetch=prefetch)
    second.load_state_dict(state)
    np.random.set_state(generators[0])
    torch.set_rng_state(generators[1])
    tail = []
    for batch in second:
        tail.append([t.clone() for t in batch])
        np.random.rand(3)
    assert len(tail) == 5 - taken and second.state_dict() == {}      # after the epoch's last batch
    for batch in second:      # an ordinary epoch follows
        tail.append([t.clone() for t in batch])
        np.random.rand(3)
    assert _same_batches(head + tail, want)
    assert not _same_batches(want[:5], want[5:])      # the two epochs are not one epoch twice


def test_loader_refuses_a_state_that_does_not_fit(dev):
    _seed(7)
    loader = _loader(dev)
    batches = iter(loader)
    next(batches)
    state = loader.state_dict()
    for _ in batches:      # the epoch is run to its end: nothing stays in flight
        pass
    assert loader.state_dict() == {}
    other = _loader(dev)
    other.load_state_dict({})      # an epoch boundary: nothing to continue
    with pytest.raises(KbnError, match="batch size"):
        _loader(dev, batch_size=3).load_state_dict(state)
    with pytest.raises(KbnError, match="9 samples, this loader has 8 paths"):
        fewer = [[os.path.join(IO, pattern.format(i)) for i in ORDER[:8]] for pattern in ("triplet_{}.png", "depth_{}.png", "k_{}.npy")]
        kb.loader.TrainingFrameLoader(*fewer, shape=(24, 40), batch_size=2, device=dev).load_state_dict(state)
    with pytest.raises(KbnError, match="prefetch"):
        _loader(dev, prefetch=2).load_state_dict(state)
    with pytest.raises(KbnError, match="next batch"):
        other.load_state_dict(dict(state, next=5))
    with pytest.raises(KbnError, match="does not hold the samples"):
        other.load_state_dict(dict(state, order=list(reversed(state["order"]))))
    with pytest.raises(KbnError, match="sharded"):
        _loader(dev, rank=0, world=2).state_dict()
    other.load_state_dict(state)      # and the one that fits is taken
