"""kb.training.launch_resumable and train_ranks_resumable without a GPU: their signatures, what the launcher refuses before it starts
or writes anything, the ranks' stop vote over two gloo processes, world and sync_batch_norm in the argument record, the call on a
finished run -- no process, no write -- and the launcher's signal forwarding to stand-in children."""
import inspect
import os
import pickle
import signal
import socket
import sys
import threading
import time

import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kbnet_amd as kb  # noqa: E402
import run_cases as rc  # noqa: E402
import train_cases as tc  # noqa: E402

KbnError = kb._lib.KbnError
training = kb.training
FOUR = {"max_steps": None, "max_seconds": None, "stop_signals": (signal.SIGTERM,), "keep_states": 2}


# ------------------------------------------------------------------------------------------------ signatures
def test_train_ranks_resumable_is_train_ranks_plus_four():
    ranks, ours = inspect.signature(training.train_ranks).parameters, inspect.signature(training.train_ranks_resumable).parameters
    assert list(ours)[:len(ranks)] == list(ranks) and list(ours)[len(ranks):] == list(FOUR)
    assert all(ours[name].default == p.default and ours[name].kind == p.kind for name, p in ranks.items())
    assert [ours[name].default for name in ("rank", "world", "sync_batch_norm")] == [0, 1, True]
    assert {name: ours[name].default for name in FOUR} == FOUR
    assert all(ours[name].kind is inspect.Parameter.KEYWORD_ONLY for name in FOUR)
    with pytest.raises(TypeError, match="session"):      # the loop's hook is nobody's argument
        training.train_ranks_resumable("a", "b", "c", None, None, None, None, session=1)
    # and the functions this one stands beside are as they were
    assert list(inspect.signature(training.train_resumable).parameters)[-4:] == list(FOUR)
    assert "rank" not in inspect.signature(training.train_resumable).parameters
    assert "train_ranks_resumable" in training.train_resumable.__doc__ and "is not built" not in training.train_resumable.__doc__


def test_launch_resumable_is_launch_plus_four():
    one, ours = inspect.signature(training.launch).parameters, inspect.signature(training.launch_resumable).parameters
    assert [name for name in ours if name not in FOUR] == list(one)
    assert all(ours[name].default == p.default and ours[name].kind == p.kind for name, p in one.items())
    assert {name: ours[name].default for name in FOUR} == FOUR
    assert all(ours[name].kind is inspect.Parameter.KEYWORD_ONLY for name in FOUR)
    assert list(one) == ["n_gpus", "backend", "devices", "timeout", "train_arguments"]


def _write_paths(filepath, paths):
    with open(filepath, "w") as f:
        f.write("\n".join(paths) + "\n")


def _arguments(tmp_path):
    lists = [str(tmp_path / name) for name in rc.write_lists(str(tmp_path), _write_paths)]
    arguments = dict(zip(training.PATH_ARGUMENTS, lists[:3] + lists))
    arguments.update(tc.train_settings(kb.kitti_config().narrow()), checkpoint_path=str(tmp_path / "trained"), device="cuda")
    return arguments


def test_launch_resumable_refuses_before_it_starts_anything(tmp_path, monkeypatch):
    arguments = _arguments(tmp_path)
    started = []
    monkeypatch.setattr(training.subprocess, "Popen", lambda *a, **k: started.append(a))
    before = signal.getsignal(signal.SIGTERM)
    launch = training.launch_resumable
    for n_gpus in (0, 17, -1, True, 2.0):
        with pytest.raises(KbnError, match="n_gpus"):
            launch(n_gpus, backend="gloo", **arguments)
    for devices in ([0], [0, 0, 0], [0, -1]):
        with pytest.raises(KbnError, match="devices"):
            launch(2, backend="gloo", devices=devices, **arguments)
    with pytest.raises(KbnError, match="devices"):
        launch(2, backend="nccl", devices=[0, 0], **arguments)      # RCCL ranks do not share a device
    with pytest.raises(KbnError, match="backend"):
        launch(2, backend="mpi", **arguments)
    with pytest.raises(KbnError, match="rank is set by launch_resumable"):
        launch(2, backend="gloo", rank=1, **arguments)
    with pytest.raises(KbnError, match="timeout"):
        launch(2, backend="gloo", timeout=0, **arguments)
    for value in (0, -1, 1.5, True):
        with pytest.raises(KbnError, match="max_steps"):
            launch(2, backend="gloo", devices=[0, 0], max_steps=value, **arguments)
    for value in (0, -2.0, float("nan")):
        with pytest.raises(KbnError, match="max_seconds"):
            launch(2, backend="gloo", devices=[0, 0], max_seconds=value, **arguments)
    for value in (0, -1, 1.5):
        with pytest.raises(KbnError, match="keep_states"):
            launch(2, backend="gloo", devices=[0, 0], keep_states=value, **arguments)
    assert not started and not os.path.exists(arguments["checkpoint_path"])
    assert signal.getsignal(signal.SIGTERM) == before


# ------------------------------------------------------------------------------------------------ the vote
N_TIMED = 1000
WISHES = [(False, False)] * 3 + [(False, True)] + [(False, False)] * 2 + [(True, False), (True, True)]      # (rank 0's, rank 1's) a call


def _vote_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    kb.dist.init("gloo")
    vote = kb.dist.StopVote(rank, world)
    answers = [vote.vote(wishes[rank]) for wishes in WISHES]
    quiet = [vote.vote(False) for _ in range(20)]      # nobody wishes: no stop
    kb.dist.barrier()
    started = time.perf_counter()
    for _ in range(N_TIMED):
        vote.vote(False)
    seconds = time.perf_counter() - started
    kb.dist.barrier()
    q.put((rank, answers, any(quiet), seconds / N_TIMED, vote.group is None))
    torch.distributed.destroy_process_group()


def test_the_vote_stops_both_ranks_on_the_call_one_of_them_wishes():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_vote_worker, args=(rank, 2, port, q)) for rank in range(2)]
    for p in procs:
        p.start()
    results = sorted(q.get(timeout=90) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = [a or b for a, b in WISHES]
    assert want == [False, False, False, True, False, False, True, True]
    for rank, answers, any_quiet, per_call, default_group in results:
        assert answers == want, (rank, answers)      # the stop on the call only rank 1 wished on, on none before it, and not after
        assert not any_quiet and default_group      # under gloo the default group carries the vote
        print(f"rank {rank}: {N_TIMED} votes of two gloo ranks on one host, {per_call * 1e6:.1f} us of host time a call")


def test_the_vote_of_one_process_is_its_wish():
    vote = kb.dist.StopVote(0, 1)
    assert [vote.vote(w) for w in (False, True, None, "signal 15")] == [False, True, False, True]
    with pytest.raises(KbnError, match="rank"):
        kb.dist.StopVote(2, 2)
    assert not torch.distributed.is_initialized()
    with pytest.raises(KbnError, match="process group"):
        kb.dist.StopVote(0, 2)


# ------------------------------------------------------------------------------------------------ the argument record
def _record(tmp_path, function=None, **changes):
    """-> (the record, the path lists' contents) of a call of train_ranks() -- or of `function` -- with tests/train_cases.py's settings."""
    arguments = _arguments(tmp_path)
    bound = inspect.signature(function or training.train_ranks).bind(**dict(arguments, **changes))
    bound.apply_defaults()
    contents = {name: kb.loader.read_paths(arguments[name]) for name in training.PATH_ARGUMENTS}
    return training.argument_record(dict(bound.arguments), contents), contents


def test_world_and_sync_batch_norm_are_in_the_record(tmp_path):
    first, _ = _record(tmp_path, world=2)
    assert list(first)[-2:] == ["world", "sync_batch_norm"] and first["world"] == 2 and first["sync_batch_norm"] is True
    assert "rank" not in first and "session" not in first
    training.check_argument_record(first, _record(tmp_path, world=2, rank=1)[0])      # every rank's record is the run's
    torch.save({"arguments": first}, str(tmp_path / "state.pth"))
    loaded = torch.load(str(tmp_path / "state.pth"), map_location="cpu")["arguments"]
    training.check_argument_record(loaded, _record(tmp_path, world=2)[0])
    with pytest.raises(KbnError, match=r"train_resumable: world is 4.*started with 2"):
        training.check_argument_record(loaded, _record(tmp_path, world=4)[0])
    with pytest.raises(KbnError, match=r"train_resumable: world is 1.*started with 2"):      # train_resumable() on a two-rank run
        training.check_argument_record(loaded, _record(tmp_path)[0])
    with pytest.raises(KbnError, match=r"train_resumable: sync_batch_norm is False.*started with True"):
        training.check_argument_record(loaded, _record(tmp_path, world=2, sync_batch_norm=False)[0])
    with pytest.raises(KbnError, match="train_resumable: n_batch is 2"):      # train()'s arguments come first
        training.check_argument_record(loaded, _record(tmp_path, world=4, n_batch=2)[0])
    # a state from before the two were recorded is a one-process run's
    old = {name: value for name, value in first.items() if name not in ("world", "sync_batch_norm")}
    training.check_argument_record(old, _record(tmp_path)[0])
    with pytest.raises(KbnError, match="train_resumable: world is 2"):
        training.check_argument_record(old, _record(tmp_path, world=2)[0])
    # train()'s own arguments alone, as a caller outside the loop may hand them: the record is as it was
    plain, _ = _record(tmp_path, function=training.train)
    assert "world" not in plain and list(plain) == list(first)[:-2]


# ------------------------------------------------------------------------------------------------ a finished run
def _touch_models(directory, step):
    for name in (f"depth_model-{step}.pth", f"pose_model-{step}.pth"):
        torch.save({"train_step": step}, os.path.join(str(directory), name))


def _listing(directory):
    found = {}
    for base, _, names in os.walk(directory):
        for name in names + [""]:
            path = os.path.join(base, name)
            found[os.path.relpath(path, directory)] = os.stat(path).st_mtime_ns
    return found


def _hand_made_state(tmp_path, step, **record_changes):
    """checkpoint_path with a state of `step` of a two-rank run of tests/train_cases.py's settings: three samples, batch 3, three
    epochs -- three steps."""
    record, _ = _record(tmp_path, world=2, **record_changes)
    out = tmp_path / "trained"
    out.mkdir(exist_ok=True)
    _touch_models(out, step)
    state = {"step": step, "arguments": record, "best_results": {"step": 2, "mae": 1.5, "rmse": 2.5, "imae": 0.5, "irmse": 0.75},
             "logged": [(1, 0.5), (2, 0.25), (3, 0.125)][:step], "digest": "d" * 64, "loader": {}, "epoch": step, "batch": 1}
    torch.save(state, str(out / f"train_state-{step}.pth"))
    return state


def test_a_finished_run_is_returned_without_a_process_or_a_write(tmp_path, monkeypatch):
    arguments = _arguments(tmp_path)
    assert training.n_train_steps(3, arguments["n_batch"], arguments["learning_schedule"], world=2) == 3
    state = _hand_made_state(tmp_path, 3)

    def no_process(*a, **k):
        raise AssertionError("launch_resumable started a process")

    monkeypatch.setattr(training.subprocess, "Popen", no_process)
    handler = signal.getsignal(signal.SIGTERM)
    before = _listing(arguments["checkpoint_path"])
    results, logged, checkpoints = training.launch_resumable(2, backend="gloo", devices=[0, 0], timeout=60, **arguments)
    assert results == {"train_step": 3, "best_results": state["best_results"], "finished": True, "resumed_from": 3, "digest": "d" * 64}
    assert logged == state["logged"] and checkpoints == []
    assert _listing(arguments["checkpoint_path"]) == before and signal.getsignal(signal.SIGTERM) == handler
    # what may change between sessions changes nothing here
    moved = dict(arguments, n_thread=3, workers=1, depth_model_restore_path="elsewhere.pth")
    assert training.launch_resumable(2, backend="nccl", devices=[0, 1], **moved)[0] == results
    # another argument than the run's is refused by name -- also after the end -- and nothing is written
    for changed, name in ((dict(sync_batch_norm=False), "sync_batch_norm"), (dict(n_batch=2), "n_batch")):
        with pytest.raises(KbnError, match=f"train_resumable: {name} is "):
            training.launch_resumable(2, backend="gloo", devices=[0, 0], **dict(arguments, **changed))
    with pytest.raises(KbnError, match="train_resumable: world is 1"):
        training.launch_resumable(1, backend="gloo", **arguments)
    assert _listing(arguments["checkpoint_path"]) == before


def test_an_unfinished_run_is_not_taken_for_a_finished_one(tmp_path, monkeypatch):
    arguments = _arguments(tmp_path)
    _hand_made_state(tmp_path, 2)

    class Started(Exception):
        pass

    def popen(*a, **k):
        raise Started()

    monkeypatch.setattr(training.subprocess, "Popen", popen)
    handler = signal.getsignal(signal.SIGTERM)
    with pytest.raises(Started):
        training.launch_resumable(2, backend="gloo", devices=[0, 0], **arguments)
    assert signal.getsignal(signal.SIGTERM) == handler      # put back on this way out too
    with open(os.path.join(arguments["checkpoint_path"], "rank0.out")) as f:
        assert f.read().splitlines() == ["==== launch_resumable: a session after step 2 ===="]


# ------------------------------------------------------------------------------------------------ the signal goes on to the children
STAND_IN = """
import os, pickle, signal, sys, time
rank, directory, results = os.environ["RANK"], sys.argv[1], sys.argv[2]
got = []
signal.signal(signal.SIGTERM, lambda number, frame: got.append(number))
open(os.path.join(directory, "ready" + rank), "w").close()
deadline = time.time() + 60
while not got and time.time() < deadline:
    time.sleep(0.01)
time.sleep(0.2)      # a second delivery would arrive within the launcher's next polls
with open(os.path.join(directory, "signal" + rank), "w") as f:
    f.write(" ".join(str(int(number)) for number in got))
print("rank", rank, "stopped")
if rank == "0":
    with open(results, "wb") as f:
        pickle.dump(({"finished": False, "ranks": os.environ["WORLD_SIZE"]}, [], []), f)
sys.exit(0 if got else 3)
"""


def test_a_signal_to_the_launcher_reaches_every_child_once(tmp_path, monkeypatch):
    assert threading.current_thread() is threading.main_thread()
    out = tmp_path / "trained"
    seen_commands = []

    def stand_in(arguments_path, stop_signals=()):
        seen_commands.append((arguments_path, list(stop_signals)))
        return [sys.executable, "-c", STAND_IN, str(tmp_path), os.path.join(os.path.dirname(arguments_path), training.RESULTS_FILE)]

    monkeypatch.setattr(training, "_child_command", stand_in)
    seen = []
    previous = lambda number, frame: seen.append(number)
    before = signal.signal(signal.SIGTERM, previous)

    def send_when_ready():
        deadline = time.time() + 60
        while time.time() < deadline and not all(os.path.exists(str(tmp_path / f"ready{rank}")) for rank in range(3)):
            time.sleep(0.01)
        os.kill(os.getpid(), signal.SIGTERM)

    sender = None
    try:
        for session in range(2):      # the second call appends to the ranks' files
            sender = threading.Thread(target=send_when_ready)
            sender.start()
            results, logged, checkpoints = training.launch_resumable(3, backend="gloo", devices=[0, 0, 0], timeout=120, checkpoint_path=str(out))
            sender.join()
            assert results == {"finished": False, "ranks": "3"} and logged == [] and checkpoints == []
            for rank in range(3):
                with open(str(tmp_path / f"signal{rank}")) as f:
                    assert f.read() == str(int(signal.SIGTERM)), rank      # once
                os.remove(str(tmp_path / f"ready{rank}"))
            assert signal.getsignal(signal.SIGTERM) is previous and seen == []      # the launcher held it, and the caller's is back
        assert seen_commands == [(str(out / training.ARGUMENTS_FILE), [int(signal.SIGTERM)])] * 2
        for rank in range(3):
            with open(str(out / f"rank{rank}.out")) as f:
                assert f.read().splitlines() == ["==== launch_resumable: a session from the start ====", f"rank {rank} stopped"] * 2
        with open(str(out / training.ARGUMENTS_FILE), "rb") as f:
            travelled = pickle.load(f)
        assert travelled["session"] == {"max_steps": None, "max_seconds": None, "stop_signals": [int(signal.SIGTERM)], "keep_states": 2}
        assert travelled["train"] == {"checkpoint_path": str(out)}
        signal.raise_signal(signal.SIGTERM)
        assert seen == [signal.SIGTERM]
    finally:
        if sender is not None:
            sender.join()
        signal.signal(signal.SIGTERM, before)


def test_a_child_that_fails_is_reported_as_in_launch(tmp_path, monkeypatch):
    program = "import os, sys, time\nif os.environ['RANK'] == '1':\n    sys.exit('rank 1 gives up')\ntime.sleep(60)\n"
    monkeypatch.setattr(training, "_child_command", lambda arguments_path, stop_signals=(): [sys.executable, "-c", program])
    handler = signal.getsignal(signal.SIGTERM)
    started = time.time()
    with pytest.raises(KbnError, match=r"(?s)launch_resumable: rank 1 of 2 exited with status 1.*rank 1 gives up"):
        training.launch_resumable(2, backend="gloo", devices=[0, 0], timeout=50, checkpoint_path=str(tmp_path / "trained"))
    assert time.time() - started < 25 and signal.getsignal(signal.SIGTERM) == handler      # rank 0 was ended with it, not waited for
