"""kb.training.train_resumable without a GPU: its signature, which state a call continues from, what is pruned, which arguments a
continuation may change, the session's budget and signal handlers, what is refused before anything is written, and the Transforms
state."""
import inspect
import os
import signal
import sys
import threading

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kbnet_amd as kb  # noqa: E402
import run_cases as rc  # noqa: E402
import train_cases as tc  # noqa: E402

KbnError = kb._lib.KbnError
training = kb.training


# ------------------------------------------------------------------------------------------------ signature
def test_signature_is_trains_plus_four():
    one, ours = inspect.signature(training.train).parameters, inspect.signature(training.train_resumable).parameters
    positional = lambda ps: [(p.name, repr(p.default)) for p in ps.values() if p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]
    assert positional(ours) == positional(one) and len(positional(one)) == 54
    extras = {p.name: p.default for p in ours.values() if p.kind is inspect.Parameter.KEYWORD_ONLY}
    assert extras == {"workers": None, "val_batch_size": 1, "summary_writer_factory": kb.summary.EventWriter, "return_results": False,
                      "max_steps": None, "max_seconds": None, "stop_signals": (signal.SIGTERM,), "keep_states": 2}
    assert len(ours) == 54 + 8
    assert list(ours)[-4:] == ["max_steps", "max_seconds", "stop_signals", "keep_states"]
    for name in ("rank", "world", "sync_batch_norm", "session"):
        with pytest.raises(TypeError, match=name):
            training.train_resumable("a", "b", "c", None, None, None, None, **{name: 1})
    for name in ("session",):      # the loop's hook is nobody's argument
        with pytest.raises(TypeError, match=name):
            training.train_ranks("a", "b", "c", None, None, None, None, **{name: 1})
    assert "INTEGRATION.md" in training.train_resumable.__doc__ and "data-parallel" in training.train_resumable.__doc__


# ------------------------------------------------------------------------------------------------ which state
def _touch_models(directory, step, depth=True, pose=True):
    for name, wanted in ((f"depth_model-{step}.pth", depth), (f"pose_model-{step}.pth", pose)):
        if wanted:
            torch.save({"train_step": step}, os.path.join(str(directory), name))


def _state(directory, step, **more):
    torch.save(dict({"step": step, "marker": f"state {step}"}, **more), os.path.join(str(directory), f"train_state-{step}.pth"))


def test_state_selection(tmp_path):
    assert training.find_state(str(tmp_path / "absent")) == (None, [])
    assert training.find_state(str(tmp_path)) == (None, [])      # an empty directory
    for step in (4, 8, 12):
        _touch_models(tmp_path, step)
        _state(tmp_path, step)
    _touch_models(tmp_path, 100)      # checkpoints without a state, as train() leaves them, are no state
    state, skipped = training.find_state(str(tmp_path))
    assert state["marker"] == "state 12" and skipped == []      # numerically the newest, not "8" > "12"

    # a newest state file that is cut short, or empty
    _touch_models(tmp_path, 16)
    _state(tmp_path, 16)
    path = tmp_path / "train_state-16.pth"
    whole = path.read_bytes()
    path.write_bytes(whole[:len(whole) // 2])
    state, skipped = training.find_state(str(tmp_path))
    assert state["marker"] == "state 12" and len(skipped) == 1 and "train_state-16.pth" in skipped[0] and skipped[0].startswith("Skipping ")
    path.write_bytes(b"")
    assert training.find_state(str(tmp_path))[0]["marker"] == "state 12"
    path.write_bytes(whole)
    assert training.find_state(str(tmp_path))[0]["marker"] == "state 16"

    # a state whose pose checkpoint is missing, one whose depth checkpoint is, one that holds another step
    _touch_models(tmp_path, 20, pose=False)
    _state(tmp_path, 20)
    _touch_models(tmp_path, 24, depth=False)
    _state(tmp_path, 24)
    _touch_models(tmp_path, 28)
    torch.save({"step": 27}, str(tmp_path / "train_state-28.pth"))
    state, skipped = training.find_state(str(tmp_path))
    assert state["marker"] == "state 16"
    # by file name: the directory's own path may hold any digits
    named = lambda s: [step for step in (16, 20, 24, 28) if f"train_state-{step}.pth" in s]
    assert [named(s) for s in skipped] == [[28], [24], [20]] and all(s.startswith("Skipping ") for s in skipped)
    assert "no pose_model-20.pth beside it" in skipped[2] and "no depth_model-24.pth beside it" in skipped[1]
    assert "does not hold a state of that step" in skipped[0]
    # names that only look like states
    (tmp_path / "train_state-99.pth.part").write_bytes(b"x")
    (tmp_path / "train_state-x.pth").write_bytes(b"x")
    assert training.find_state(str(tmp_path))[0]["marker"] == "state 16"


def test_pruning_keeps_the_newest_states_and_every_grid_checkpoint(tmp_path):
    # n_checkpoint 4, 12 steps: stops at 1 and 6, grid states at 4 and 8
    for step in (1, 4, 6, 8):
        _touch_models(tmp_path, step)
        _state(tmp_path, step)
    listing = lambda: sorted(os.listdir(str(tmp_path)))
    removed = training.prune_states(str(tmp_path), 2, 4, 12)
    assert sorted(os.path.basename(p) for p in removed) == ["depth_model-1.pth", "pose_model-1.pth", "train_state-1.pth", "train_state-4.pth"]
    assert listing() == sorted(["depth_model-4.pth", "pose_model-4.pth", "depth_model-6.pth", "pose_model-6.pth", "train_state-6.pth",
                                "depth_model-8.pth", "pose_model-8.pth", "train_state-8.pth"])
    assert training.prune_states(str(tmp_path), 2, 4, 12) == []
    training.prune_states(str(tmp_path), 1, 4, 12)
    assert listing() == sorted(["depth_model-4.pth", "pose_model-4.pth", "depth_model-8.pth", "pose_model-8.pth", "train_state-8.pth"])
    # the last step's checkpoints stay though they are off the grid (13 steps, n_checkpoint 4)
    _touch_models(tmp_path, 13)
    _state(tmp_path, 13)
    _touch_models(tmp_path, 14)
    _state(tmp_path, 14)
    training.prune_states(str(tmp_path), 1, 4, 13)
    assert listing() == sorted(["depth_model-4.pth", "pose_model-4.pth", "depth_model-8.pth", "pose_model-8.pth",
                                "depth_model-13.pth", "pose_model-13.pth", "depth_model-14.pth", "pose_model-14.pth", "train_state-14.pth"])
    with pytest.raises(KbnError, match="keep_states"):
        training._Session(training.Budget(), 0)


def test_pruning_removes_a_state_newer_than_the_one_just_written(tmp_path):
    """keep_states=1, a state of step 6 that loads and one of step 9 that find_state passed over; the run goes on from 6 and
    writes step 8: the unreadable newer state must not be the one state that is kept."""
    for step in (6, 8, 9):
        _touch_models(tmp_path, step)
        _state(tmp_path, step)
    (tmp_path / "train_state-9.pth").write_bytes(b"cut short")
    assert training.find_state(str(tmp_path))[0]["marker"] == "state 8"
    removed = training.prune_states(str(tmp_path), 1, 4, 12, current=8)
    assert sorted(os.path.basename(p) for p in removed) == ["depth_model-6.pth", "depth_model-9.pth", "pose_model-6.pth", "pose_model-9.pth",
                                                            "train_state-6.pth", "train_state-9.pth"]
    assert sorted(os.listdir(str(tmp_path))) == ["depth_model-8.pth", "pose_model-8.pth", "train_state-8.pth"]
    state, skipped = training.find_state(str(tmp_path))
    assert state["marker"] == "state 8" and skipped == []


# ------------------------------------------------------------------------------------------------ the argument record
def _arguments(tmp_path, **changes):
    """What the loop sees of a call: every argument of train() by name."""
    bound = inspect.signature(training.train).bind("image.txt", "depth.txt", "k.txt", None, None, None, None,
                                                   **dict(tc.train_settings(kb.kitti_config().narrow()), **changes))
    bound.apply_defaults()
    return dict(bound.arguments)


def _record(tmp_path, contents=None, **changes):
    contents = contents or {"train_image_path": ["a.png", "b.png"], "train_sparse_depth_path": ["a_d.png", "b_d.png"],
                            "train_intrinsics_path": ["a.npy", "b.npy"]}
    return training.argument_record(_arguments(tmp_path, **changes), contents)


def test_argument_record(tmp_path):
    first = _record(tmp_path)
    assert list(first)[:7] == list(training.PATH_ARGUMENTS) and first["val_image_path"] is None
    assert first["train_image_path"] == ["a.png", "b.png"]      # the list's content, not the name of the file that lists it
    for name in training.UNRECORDED_ARGUMENTS:
        assert name not in first
    assert set(first) | set(training.UNRECORDED_ARGUMENTS) == set(inspect.signature(training.train).parameters)
    training.check_argument_record(first, _record(tmp_path))
    # through a file and back: what a continuation compares with
    torch.save({"arguments": first}, str(tmp_path / "state.pth"))
    loaded = torch.load(str(tmp_path / "state.pth"), map_location="cpu")["arguments"]
    training.check_argument_record(loaded, _record(tmp_path))
    # a tuple for a list, an int for a float of the same value: the same setting
    training.check_argument_record(loaded, _record(tmp_path, learning_schedule=(1, 3), w_color=0.15, n_batch=3.0))

    for name, value in (("n_batch", 2), ("learning_schedule", [2, 3]), ("learning_rates", [1e-4, 4e-5]),
                        ("augmentation_random_crop_type", ["horizontal"]), ("augmentation_probabilities", [0.5]),
                        ("augmentation_random_remove_points", [0.5, 0.7]), ("w_smoothness", 0.05), ("val_batch_size", 2),
                        ("n_checkpoint", 2)):
        with pytest.raises(KbnError, match=rf"train_resumable: {name} is "):
            training.check_argument_record(loaded, _record(tmp_path, **{name: value}))
    # the first one in train()'s order is the one named
    with pytest.raises(KbnError, match="train_resumable: n_batch is 2"):
        training.check_argument_record(loaded, _record(tmp_path, w_smoothness=0.05, n_batch=2))
    # a path list by content: another file in it, one file fewer
    changed = {"train_image_path": ["a.png", "c.png"], "train_sparse_depth_path": ["a_d.png", "b_d.png"], "train_intrinsics_path": ["a.npy", "b.npy"]}
    with pytest.raises(KbnError, match="train_resumable: train_image_path is '2 paths, not the same ones'"):
        training.check_argument_record(loaded, _record(tmp_path, contents=changed))
    shorter = dict(changed, train_sparse_depth_path=["a_d.png"], train_image_path=["a.png", "b.png"])
    with pytest.raises(KbnError, match="train_resumable: train_sparse_depth_path is '1 paths'"):
        training.check_argument_record(loaded, _record(tmp_path, contents=shorter))
    # where the files lie, what a fresh start restores and the host's threads may change
    training.check_argument_record(loaded, _record(tmp_path, checkpoint_path="elsewhere", n_thread=3, workers=5, device="gpu",
                                                   depth_model_restore_path="other.pth", pose_model_restore_path="other_pose.pth",
                                                   return_results=True, summary_writer_factory=tc.RecordingWriter))


# ------------------------------------------------------------------------------------------------ the budget
class _Clock:
    def __init__(self):
        self.now = 100.0

    def __call__(self):
        return self.now


def test_budget_counts_steps_and_seconds():
    budget = training.Budget(max_steps=3, stop_signals=())
    with budget:
        assert [budget.step_done() for _ in range(4)] == [None, None, "max_steps", "max_steps"]
    clock = _Clock()
    budget = training.Budget(max_seconds=10, stop_signals=(), clock=clock)
    clock.now = 500.0      # the seconds count from where the context is entered, not from the construction
    with budget:
        assert budget.step_done() is None
        clock.now = 509.9
        assert budget.step_done() is None
        clock.now = 510.0
        assert budget.step_done() == "max_seconds"
    unlimited = training.Budget(stop_signals=())
    with unlimited:
        assert all(unlimited.step_done() is None for _ in range(1000))
    both = training.Budget(max_steps=1, max_seconds=1e9, stop_signals=())
    with both:
        assert both.step_done() == "max_steps"


def test_budget_signal_sets_a_flag_and_the_previous_handler_returns():
    assert threading.current_thread() is threading.main_thread()
    seen = []
    previous = lambda number, frame: seen.append(number)
    before = signal.signal(signal.SIGTERM, previous)
    try:
        budget = training.Budget()
        assert budget.stop_signals == (signal.SIGTERM,)
        with budget:
            assert signal.getsignal(signal.SIGTERM) == budget._flag
            assert budget.step_done() is None
            signal.raise_signal(signal.SIGTERM)      # the process lives: this line returns
            assert budget.signalled == signal.SIGTERM and seen == []
            assert budget.step_done() == f"signal {int(signal.SIGTERM)}"
        assert signal.getsignal(signal.SIGTERM) is previous
        # put back when the body raises, too, and with more than one signal
        budget = training.Budget(stop_signals=(signal.SIGTERM, signal.SIGUSR1))
        usr1 = signal.getsignal(signal.SIGUSR1)
        with pytest.raises(RuntimeError):
            with budget:
                assert signal.getsignal(signal.SIGUSR1) == budget._flag
                raise RuntimeError("the loop failed")
        assert signal.getsignal(signal.SIGTERM) is previous and signal.getsignal(signal.SIGUSR1) == usr1
        signal.raise_signal(signal.SIGTERM)
        assert seen == [signal.SIGTERM] and budget.signalled is None
    finally:
        signal.signal(signal.SIGTERM, before)


def test_budget_installs_nothing_off_the_main_thread():
    before = signal.getsignal(signal.SIGTERM)
    out = {}

    def body():
        try:
            budget = training.Budget(max_steps=2)
            with budget:
                out["installed"] = dict(budget.installed)
                out["handler"] = signal.getsignal(signal.SIGTERM)
                out["steps"] = [budget.step_done(), budget.step_done()]
        except BaseException as e:      # noqa: BLE001  (shown by the assertion below)
            out["error"] = e

    thread = threading.Thread(target=body)
    thread.start()
    thread.join()
    assert "error" not in out, out
    assert out["installed"] == {} and out["handler"] == before and out["steps"] == [None, "max_steps"]
    assert signal.getsignal(signal.SIGTERM) == before


# ------------------------------------------------------------------------------------------------ refusals
def _write_paths(filepath, paths):
    with open(filepath, "w") as f:
        f.write("\n".join(paths) + "\n")


def test_refusals_come_before_anything_is_written(tmp_path):
    lists = [str(tmp_path / name) for name in rc.write_lists(str(tmp_path), _write_paths)]
    settings = tc.train_settings(kb.kitti_config().narrow())
    out = str(tmp_path / "trained")
    call = lambda **more: training.train_resumable(lists[0], lists[1], lists[2], lists[0], lists[1], lists[2], lists[3], checkpoint_path=out,
                                                   **dict(settings, **more))
    before = signal.getsignal(signal.SIGTERM)
    for value in (0, -1, 1.5, True):
        with pytest.raises(KbnError, match="max_steps"):
            call(max_steps=value)
    for value in (0, -2.0, float("nan")):
        with pytest.raises(KbnError, match="max_seconds"):
            call(max_seconds=value)
    for value in (0, -1, 1.5):
        with pytest.raises(KbnError, match="keep_states"):
            call(keep_states=value)
    with pytest.raises(KbnError, match="no CPU fallback"):
        call(device="cpu")
    with pytest.raises(KbnError, match="val_batch_size"):      # train()'s own refusals are this function's
        call(val_batch_size=0)
    with pytest.raises(KbnError, match="transpose"):
        call(deconv_type="transpose", device="cuda")
    assert not os.path.exists(out)
    assert signal.getsignal(signal.SIGTERM) == before      # and the handlers are the caller's again after each


# ------------------------------------------------------------------------------------------------ Transforms
def test_transforms_state_round_trip():
    torch.manual_seed(1234)
    a = kb.transforms.Transforms(random_remove_points=[0.6, 0.7])
    assert a.state_dict() == {"seed": 1234, "calls": 0}
    a.calls = 7
    torch.manual_seed(99)
    b = kb.transforms.Transforms(random_remove_points=[0.6, 0.7])
    assert b.state_dict() == {"seed": 99, "calls": 0}
    b.load_state_dict(a.state_dict())
    assert (b.seed, b.calls) == (1234, 7) and b.state_dict() == a.state_dict()
    wide = kb.transforms.Transforms(seed=0xFEDCBA9876543210)      # a key beyond 63 bits
    state = wide.state_dict()
    assert state["seed"] == 0xFEDCBA9876543210 and type(state["seed"]) is int and type(state["calls"]) is int
    b.load_state_dict(state)
    assert b.seed == 0xFEDCBA9876543210 and b.calls == 0
    for bad in ({"seed": -1, "calls": 0}, {"seed": 1, "calls": -1}, {"seed": 1 << 64, "calls": 0}):
        with pytest.raises(ValueError):
            b.load_state_dict(bad)
    with pytest.raises(KeyError):
        b.load_state_dict({"seed": 1})
    assert b.seed == 0xFEDCBA9876543210 and b.calls == 0      # a refused state changes nothing
