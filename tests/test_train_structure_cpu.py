"""The parts kb.training's loop is made of, without a GPU: the writers' context and its error rules, the holder of the two schedule
positions against scheduled() walked by hand, and the one resume point the loop and launch_resumable() share."""
import inspect
import os
import sys

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


# ------------------------------------------------------------------------------------------------ the writers
class _Writer:
    def __init__(self, path, calls, close_raises):
        self.path, self.calls, self.close_raises = path, calls, close_raises
        calls.append(("open", path))

    def close(self):
        self.calls.append(("close", self.path))
        if self.path in self.close_raises:
            raise OSError("close of " + self.path)


def _factory(calls, close_raises=()):
    return lambda path: _Writer(path, calls, close_raises)


class _BodyError(Exception):
    pass


@pytest.mark.parametrize("close_raises", [(), ("events-train",), ("events-train", "events-val")])
def test_writers_an_exception_in_the_body_closes_both_and_is_the_one_raised(close_raises):
    calls = []
    with pytest.raises(_BodyError, match="the body's"):
        with training._summary_writers(_factory(calls, close_raises), "events", True) as (train_writer, val_writer):
            assert (train_writer.path, val_writer.path) == ("events-train", "events-val")
            raise _BodyError("the body's")
    assert calls == [("open", "events-train"), ("open", "events-val"), ("close", "events-train"), ("close", "events-val")]


def test_writers_a_factory_that_fails_closes_what_was_opened():
    calls = []

    def factory(path):
        if path.endswith("-val"):
            raise _BodyError("no val writer")
        return _Writer(path, calls, ())

    with pytest.raises(_BodyError, match="no val writer"):
        with training._summary_writers(factory, "events", True):
            raise AssertionError("the body ran without its writers")
    assert calls == [("open", "events-train"), ("close", "events-train")]


def test_writers_the_normal_path_closes_train_then_val_and_close_errors_propagate():
    calls = []
    with training._summary_writers(_factory(calls), "events", True) as (train_writer, val_writer):
        calls.append("body")
    assert calls == [("open", "events-train"), ("open", "events-val"), "body", ("close", "events-train"), ("close", "events-val")]
    # the train writer's close raises: the val writer is closed all the same, and the error is the caller's
    calls = []
    with pytest.raises(OSError, match="close of events-train"):
        with training._summary_writers(_factory(calls, ("events-train",)), "events", True):
            pass
    assert calls[-2:] == [("close", "events-train"), ("close", "events-val")]
    calls = []
    with pytest.raises(OSError, match="close of events-val"):
        with training._summary_writers(_factory(calls, ("events-val",)), "events", True):
            pass
    assert calls[-2:] == [("close", "events-train"), ("close", "events-val")]


def test_writers_a_rank_that_does_not_write_never_calls_the_factory():
    def factory(path):
        raise AssertionError("summary_writer_factory called on a rank that is not rank 0")

    with training._summary_writers(factory, "events", False) as writers:
        assert writers == (None, None)
    with pytest.raises(_BodyError):
        with training._summary_writers(factory, "events", False):
            raise _BodyError()


# ------------------------------------------------------------------------------------------------ the schedules
SCHEDULES = [      # (learning_schedule, learning_rates, augmentation_schedule, augmentation_probabilities, epochs the rate moves at)
    ([1, 3], [1e-4, 5e-5], [-1], [0.0], [2]),
    ([2, 8, 20], [5e-5, 1e-4, 15e-5], [5, 12, 20], [1.0, 0.5, 0.25], [3, 9]),
    ([1, 1, 4], [1, 2, 3], [2, 2, 4], [0.9, 0.8, 0.7], [2, 3]),      # a repeated entry lags one epoch behind
    ([2, 8, 20, 30, 45, 60], [5e-5, 1e-4, 15e-5, 1e-4, 5e-5, 2e-5], [50, 55, 60], [1.00, 0.50, 0.25], [3, 9, 21, 31, 46]),
    ([1, 2], [1e-4, 5e-5], [-1, 2], [1.0, 0.5], [2]),      # -1 anywhere freezes the augmentation
]


def _by_hand(learning_schedule, learning_rates, augmentation_schedule, augmentation_probabilities, epochs):
    """scheduled() walked as the loop of before walked it -> (the four values after `epochs` epochs, the rate's moved flags)."""
    lp, lr, ap, prob, flags = 0, learning_rates[0], 0, augmentation_probabilities[0], []
    for epoch in range(1, epochs + 1):
        lp, lr, moved = training.scheduled(epoch, lp, learning_schedule, learning_rates)
        ap, prob, _ = training.scheduled(epoch, ap, augmentation_schedule, augmentation_probabilities, frozen=-1 in augmentation_schedule)
        flags.append(moved)
    return (lp, lr, ap, prob), flags


@pytest.mark.parametrize("case", SCHEDULES, ids=[str(i) for i in range(len(SCHEDULES))])
def test_schedules_advance_as_scheduled_walked_by_hand(case):
    *settings, moves = case
    last = settings[0][-1]
    fresh = training._Schedules(*settings)
    assert (fresh.learning_position, fresh.learning_rate, fresh.augmentation_position, fresh.augmentation_probability) == \
        (0, settings[1][0], 0, settings[3][0])
    for state_epoch in range(0, last + 1):      # the replay of a continuation whose state is of this epoch
        holder = training._Schedules(*settings)
        flags = [holder.advance(epoch) for epoch in range(1, state_epoch + 1)]
        want, want_flags = _by_hand(*settings, state_epoch)
        assert (holder.learning_position, holder.learning_rate, holder.augmentation_position, holder.augmentation_probability) == want
        assert flags == want_flags and all(isinstance(flag, bool) for flag in flags)
        assert [epoch + 1 for epoch, moved in enumerate(flags) if moved] == [epoch for epoch in moves if epoch <= state_epoch]
    if -1 in settings[2]:
        assert (holder.augmentation_position, holder.augmentation_probability) == (0, settings[3][0])


def test_schedules_values_test_schedule_arithmetic_expects():
    def walk(*settings):
        holder = training._Schedules(*settings)
        out = []
        for epoch in range(1, settings[0][-1] + 1):
            moved = holder.advance(epoch)
            out.append((holder.learning_rate, moved, holder.augmentation_probability))
        return out

    assert [(v, m) for v, m, _ in walk([1, 3], [1e-4, 5e-5], [-1], [0.0])] == [(1e-4, False), (5e-5, True), (5e-5, False)]
    rates = [5e-5, 1e-4, 15e-5]
    got = walk([2, 8, 20], rates, [-1], [0.0])
    assert [v for v, _, _ in got] == [rates[0]] * 2 + [rates[1]] * 6 + [rates[2]] * 12 and {p for _, _, p in got} == {0.0}
    assert [v for v, _, _ in walk([1, 1, 4], [1, 2, 3], [-1], [0.0])] == [1, 2, 3, 3]
    got = walk([60], [1e-4], [50, 55, 60], [1.0, 0.5, 0.25])
    assert [p for _, _, p in got][49:56] == [1.0, 0.5, 0.5, 0.5, 0.5, 0.5, 0.25] and not any(m for _, m, _ in got)


# ------------------------------------------------------------------------------------------------ the resume point
def _write_paths(filepath, paths):
    with open(filepath, "w") as f:
        f.write("\n".join(paths) + "\n")


def _arguments(tmp_path):
    """tests/train_cases.py's settings over three samples: batch 3, three epochs -- three steps."""
    lists = [str(tmp_path / name) for name in rc.write_lists(str(tmp_path), _write_paths)]
    arguments = dict(zip(training.PATH_ARGUMENTS, lists[:3] + lists))
    arguments.update(tc.train_settings(kb.kitti_config().narrow()), checkpoint_path=str(tmp_path / "trained"), device="cuda")
    return arguments


def _bound(arguments, **more):
    bound = inspect.signature(training.train_ranks).bind(**dict(arguments, **more))
    bound.apply_defaults()
    return dict(bound.arguments)


def test_resume_point_is_finished_exactly_from_the_last_step_on(tmp_path):
    arguments = _arguments(tmp_path)
    for world, n_batch in ((1, 3), (2, 3), (1, 2), (2, 2)):
        given = _bound(arguments, world=world, n_batch=n_batch)
        n_sample = len(kb.loader.read_paths(arguments["train_image_path"]))
        last = training.n_train_steps(n_sample, n_batch, given["learning_schedule"], world=world)
        assert n_sample == 3 and last == {(1, 3): 3, (2, 3): 3, (1, 2): 6, (2, 2): 3}[(world, n_batch)]
        record, steps, finished = training._resume_point(given, world, None)
        assert steps == last and finished is False
        contents = {name: kb.loader.read_paths(arguments[name]) for name in training.PATH_ARGUMENTS}
        assert record == training.argument_record(given, contents) and record["world"] == world
        for step in range(0, last + 3):
            state = {"step": step, "arguments": record}
            assert training._resume_point(given, world, state) == (record, last, step >= last), (world, n_batch, step)
            # the lists the loop has read already are the ones used
            assert training._resume_point(given, world, state, contents) == (record, last, step >= last)


def test_resume_point_refuses_a_changed_argument_by_name(tmp_path):
    arguments = _arguments(tmp_path)
    record, last, _ = training._resume_point(_bound(arguments, world=2), 2, None)
    for step in (1, last, last + 1):      # also after the end
        state = {"step": step, "arguments": record}
        for changed, name in ((dict(n_batch=2), "n_batch"), (dict(sync_batch_norm=False), "sync_batch_norm"),
                              (dict(learning_rates=[1e-4, 4e-5]), "learning_rates"), (dict(world=1), "world")):
            given = _bound(arguments, **dict(dict(world=2), **changed))
            with pytest.raises(KbnError, match=f"train_resumable: {name} is "):
                training._resume_point(given, given["world"], state)
        # another list of the same length is another run's; what may change between sessions is not looked at
        other = str(tmp_path / "other_images.txt")
        _write_paths(other, list(reversed(kb.loader.read_paths(arguments["train_image_path"]))))
        with pytest.raises(KbnError, match="train_resumable: train_image_path is '3 paths, not the same ones'"):
            training._resume_point(_bound(arguments, world=2, train_image_path=other), 2, state)
        moved = _bound(arguments, world=2, rank=1, checkpoint_path="elsewhere", n_thread=3, workers=1, depth_model_restore_path="d.pth")
        assert training._resume_point(moved, 2, state) == (record, last, step >= last)
    # validation off: the four validation lists are not read, and the record holds None for them
    off = _bound(dict(arguments, val_ground_truth_path=None, val_image_path=str(tmp_path / "no such list")), world=2)
    assert [training._resume_point(off, 2, None)[0][name] for name in training.PATH_ARGUMENTS[3:]] == [None] * 4


def _hand_made_state(tmp_path, record, step):
    out = tmp_path / "trained"
    out.mkdir(exist_ok=True)
    for name in (f"depth_model-{step}.pth", f"pose_model-{step}.pth"):
        torch.save({"train_step": step}, str(out / name))
    state = {"step": step, "arguments": record, "best_results": {"step": 2, "mae": 1.5, "rmse": 2.5, "imae": 0.5, "irmse": 0.75},
             "logged": [(1, 0.5), (2, 0.25), (3, 0.125)][:step], "digest": "d" * 64, "loader": {}, "epoch": step, "batch": 1}
    torch.save(state, str(out / f"train_state-{step}.pth"))
    return state


def test_launch_resumable_asks_the_loops_resume_point(tmp_path, monkeypatch):
    arguments = _arguments(tmp_path)
    real, asked = training._resume_point, []
    record, _, _ = real(_bound(arguments, world=2), 2, None)

    def recording(given, world, state, *more):
        asked.append((given, world, state, more))
        return real(given, world, state, *more)

    class Started(Exception):
        pass

    def popen(*a, **k):
        raise Started()

    monkeypatch.setattr(training, "_resume_point", recording)
    monkeypatch.setattr(training.subprocess, "Popen", popen)
    # no state: nothing to ask about, the ranks are started
    with pytest.raises(Started):
        training.launch_resumable(2, backend="gloo", devices=[0, 0], **arguments)
    assert asked == []
    # a state of step 2 of 3: asked, not finished, the ranks are started
    state = _hand_made_state(tmp_path, record, 2)
    with pytest.raises(Started):
        training.launch_resumable(2, backend="gloo", devices=[0, 0], **arguments)
    assert len(asked) == 1
    given, world, seen, more = asked.pop()
    assert world == 2 and seen["step"] == 2 and seen["arguments"] == state["arguments"] and more == ()
    assert given == _bound(arguments, rank=0, world=2)      # the bound arguments, defaults and all
    # a state of the last step: asked, finished, nothing started
    _hand_made_state(tmp_path, record, 3)
    results, logged, checkpoints = training.launch_resumable(2, backend="gloo", devices=[0, 0], **arguments)
    assert results["finished"] is True and results["train_step"] == 3 and checkpoints == []
    assert [(world, seen["step"]) for _, world, seen, _ in asked] == [(2, 3)]
    # its answer is the launcher's: a resume point that says "not finished" has the ranks started
    monkeypatch.setattr(training, "_resume_point", lambda given, world, state, *more: (None, 3, False))
    with pytest.raises(Started):
        training.launch_resumable(2, backend="gloo", devices=[0, 0], **arguments)
    # and its refusal too
    monkeypatch.setattr(training, "_resume_point", recording)
    with pytest.raises(KbnError, match="train_resumable: n_batch is 2"):
        training.launch_resumable(2, backend="gloo", devices=[0, 0], **dict(arguments, n_batch=2))
