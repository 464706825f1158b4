"""The training entry point: the reference's train() (src/kbnet.py:31-518, what train_kbnet.py calls) over this package's classes --
the loop INTEGRATION.md ("The training iteration") spells out, with the reference's logging, schedules, validation and checkpoints
around it.

    reference                                               here
    DataLoader(KBNetTrainingDataset, shuffle=True)          loader.TrainingFrameLoader(shuffle=True): device batches
    validity map, OutlierRemoval, Transforms.transform      transforms.train_inputs: one preprocess launch, two augment launches
    KBNetModel / PoseNetModel('resnet18') in .train()       KBNetModel(trainable=True).requires_grad_(True); ResNetPoseNetModel(18,
                                                            trainable=True).requires_grad_(True).set_batch_norm('batch')
    torch.optim.Adam over two groups                        optim.Adam: one launch a step
    SummaryWriter(event_path + '-train' / '-val')           summary.EventWriter: histograms on the device, copies behind the stream
    validate() at batch 1 through a DataLoader              validation.validate over loader.InferenceFrameLoader(val_batch_size)
    loss.item() at every checkpoint                         the same: the loop's only wait for the device

    torch.nn.DataParallel over every visible device      train_ranks(rank=, world=): one process per GPU over kb.dist.GradientAverager and
                                                            BatchNormGroup, the ranks building between them the batch one process
                                                            builds; launch(n_gpus, ...) starts the processes

train() has the reference's signature and drives one GPU; train_ranks() is the same function with rank, world and
sync_batch_norm -- train() is train_ranks(world=1).  DESIGN section 8p has the design of the data-parallel form.

train_resumable() is train() in sessions: the same call, made in one job slot after another, continues the run from the state the
last one left in checkpoint_path, bit for bit as the uninterrupted run.  train_ranks_resumable() is the same for
train_ranks() -- the ranks agree on the step a session stops after, rank 0 writes the one state every rank continues from -- and
launch_resumable() starts its processes and passes the scheduler's signal on to them.  All entry points run one
loop: _train_loop names the phases of a run, top to bottom, and a _Run holds what the phases and the steps share."""

from __future__ import annotations

import contextlib
import hashlib
import inspect
import os
import pickle
import re
import signal
import socket
import subprocess
import sys
import threading
import time
import types

import numpy as np
import torch

from . import dist, loader, optim, summary, transforms, validation
from ._lib import KbnError
from .modules import KBNetModel, ResNetPoseNetModel


def n_train_steps(n_train_sample: int, n_batch: int, learning_schedule, world: int = 1) -> int:
    """reference src/kbnet.py:131-132: the last epoch of the schedule times the batches of an epoch, the last one short or not.
    With `world` ranks a batch of fewer frames than ranks is no step (train_ranks() skips it on every rank), so only the batches that
    give every rank a frame (dist.every_rank_has_frames) count."""
    if int(world) == 1:
        return int(learning_schedule[-1] * np.ceil(n_train_sample / n_batch).astype(np.int32))
    full, short = divmod(int(n_train_sample), int(n_batch))
    steps = (full if dist.every_rank_has_frames(n_batch, world) else 0) + (1 if short and dist.every_rank_has_frames(short, world) else 0)
    return int(learning_schedule[-1] * steps)


def replica_digest(models, optimizer) -> str:
    """SHA-256 over everything a replica of a data-parallel run holds: every parameter and buffer of `models` (their modules'
    state_dict, BatchNorm running statistics included) and the optimizer's state (steps and moments) and groups, names and bits.
    Equal on every rank when the replicas are bit-identical; launch() compares the ranks' values."""
    h = hashlib.sha256()

    def feed(value):
        if torch.is_tensor(value):
            t = value.detach().cpu().contiguous()
            h.update(f"{t.dtype}{tuple(t.shape)}".encode())
            h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes())
        elif isinstance(value, dict):
            for key in value:
                h.update(repr(key).encode())
                feed(value[key])
        elif isinstance(value, (list, tuple)):
            for item in value:
                feed(item)
        else:
            h.update(repr(value).encode())

    for model in models:
        for module in model.modules():
            feed(module.state_dict())
    feed(optimizer.state_dict())
    return h.hexdigest()


def scheduled(epoch: int, position: int, schedule, values, frozen: bool = False):
    """reference src/kbnet.py:378-390 for one schedule at the start of `epoch` (1-based) -> (position, value, moved): the position
    moves on by ONE when the epoch lies behind the schedule's entry at the current position, never with `frozen` (the reference's
    `-1 in augmentation_schedule`)."""
    if not frozen and epoch > schedule[position]:
        return position + 1, values[position + 1], True
    return position, values[position], False


# ------------------------------------------------------------------------------------------------ a run in sessions
PATH_ARGUMENTS = ("train_image_path", "train_sparse_depth_path", "train_intrinsics_path", "val_image_path", "val_sparse_depth_path",
                  "val_intrinsics_path", "val_ground_truth_path")
# what may change from one session of a run to the next: where the files lie, what a fresh start restores, the host's threads, and
# what is not a setting at all
UNRECORDED_ARGUMENTS = ("checkpoint_path", "depth_model_restore_path", "pose_model_restore_path", "device", "n_thread", "workers",
                        "summary_writer_factory", "return_results")
# what train_ranks() adds to train() and the record keeps: how many ranks build the batch, and over which frames the pose network
# normalises.  The values of a state written before they were recorded: the one-process run's
RANK_ARGUMENTS = {"world": 1, "sync_batch_norm": True}
STATE_FILE = "train_state-{}.pth"
_STATE_NAME = re.compile(r"^train_state-(\d+)\.pth$")


def _plain(value):
    """Lists for tuples and arrays, Python numbers for NumPy's: values that compare by content and load anywhere."""
    if isinstance(value, (list, tuple, np.ndarray)):
        return [_plain(v) for v in value]
    if isinstance(value, (bool, np.bool_)):
        return bool(value)
    if isinstance(value, (int, np.integer)):
        return int(value)
    if isinstance(value, (float, np.floating)):
        return float(value)
    return value


def argument_record(arguments: dict, path_contents: dict) -> dict:
    """Every argument of train() that shapes the trajectory, in train()'s order: all but UNRECORDED_ARGUMENTS, the seven path
    arguments by the content of their lists (`path_contents`: name -> paths; a validation argument that is None stays None).  Then
    train_ranks()'s world and sync_batch_norm, where `arguments` holds them (the loop's do): a run continues with the ranks it began
    with.  rank is no setting, and launch()'s backend and devices are recorded nowhere: they may change."""
    record = {}
    for name in _TRAIN_SIGNATURE.parameters:
        if name not in UNRECORDED_ARGUMENTS:
            record[name] = _plain(path_contents.get(name)) if name in PATH_ARGUMENTS else _plain(arguments[name])
    for name in RANK_ARGUMENTS:
        if name in arguments:
            record[name] = _plain(arguments[name])
    return record


def check_argument_record(recorded: dict, given: dict) -> None:
    """KbnError naming the first argument, in train()'s order (world and sync_batch_norm after them), whose value is not the one
    the run was started with."""
    for name in given:
        if name in RANK_ARGUMENTS and name not in recorded:      # a state from before the two were recorded: a one-process run's
            recorded = dict(recorded, **{name: RANK_ARGUMENTS[name]})
        if name not in recorded or recorded[name] != given[name]:
            was, now = recorded.get(name, "<not recorded>"), given[name]
            if name in PATH_ARGUMENTS and isinstance(was, list) and isinstance(now, list):
                was, now = f"{len(was)} paths", f"{len(now)} paths" + ("" if len(was) != len(now) else ", not the same ones")
            raise KbnError(f"train_resumable: {name} is {now!r}, the run in this checkpoint_path was started with {was!r}: a continuation "
                           "takes the arguments of the first session (checkpoint_path, the restore paths, device, n_thread and workers "
                           "may change)")


def random_state(device) -> dict:
    """The three generators a step draws from: NumPy's global one (crops, flags), torch's CPU one (the epoch's order) and the
    device's (removal densities).  All three are host-side values: nothing waits for the device."""
    name, keys, position, has_gauss, cached_gaussian = np.random.get_state()
    return {"numpy": (str(name), torch.from_numpy(keys.astype(np.int64)), int(position), int(has_gauss), float(cached_gaussian)),
            "torch": torch.get_rng_state(), "device": torch.cuda.get_rng_state(device)}


def set_random_state(state: dict, device) -> None:
    name, keys, position, has_gauss, cached_gaussian = state["numpy"]
    np.random.set_state((name, keys.numpy().astype(np.uint32), position, has_gauss, cached_gaussian))
    torch.set_rng_state(state["torch"])
    torch.cuda.set_rng_state(state["device"], device)


def find_state(checkpoint_path: str):
    """-> (the newest complete training state of `checkpoint_path` or None, a message for every newer one passed over).  A state is
    complete when its train_state-<step>.pth loads and holds that step, and depth_model-<step>.pth and pose_model-<step>.pth exist
    beside it -- the state is moved into place after the two, so a job killed while writing leaves an older state the newest."""
    steps = []
    if os.path.isdir(checkpoint_path):
        steps = sorted((int(m.group(1)) for m in map(_STATE_NAME.match, os.listdir(checkpoint_path)) if m), reverse=True)
    skipped = []
    for step in steps:
        path = os.path.join(checkpoint_path, STATE_FILE.format(step))
        missing = [name for name in (f"depth_model-{step}.pth", f"pose_model-{step}.pth")
                   if not os.path.isfile(os.path.join(checkpoint_path, name))]
        if missing:
            skipped.append(f"Skipping {path}: no {' and no '.join(missing)} beside it")
            continue
        try:
            state = torch.load(path, map_location="cpu")
            if not isinstance(state, dict) or int(state["step"]) != step:
                raise ValueError("it does not hold a state of that step")
        except Exception as e:      # noqa: BLE001  (a truncated or foreign file: whatever the unpickler makes of it)
            skipped.append(f"Skipping {path}: {type(e).__name__}: {str(e).splitlines()[0] if str(e) else 'unreadable'}")
            continue
        return state, skipped
    return None, skipped


def prune_states(checkpoint_path: str, keep_states: int, n_checkpoint: int, n_train_step: int, current=None) -> list:
    """Removes all but the newest `keep_states` train_state files, and with a removed state the two model checkpoints of its step
    when that step is a stop's: one off the n_checkpoint grid that is not the run's last.  `current`: the step whose state was just
    written -- a state of a later step is one find_state passed over (the run went on from an older one); it goes first and does
    not count, or it would push the states that load out of the `keep_states` kept.  -> the paths removed."""
    steps = sorted(int(m.group(1)) for m in map(_STATE_NAME.match, os.listdir(checkpoint_path)) if m)
    stale = [step for step in steps if current is not None and step > int(current)]
    steps = [step for step in steps if step not in stale]
    removed = []
    for step in stale + steps[:max(0, len(steps) - int(keep_states))]:
        names = [STATE_FILE.format(step)]
        if step % int(n_checkpoint) != 0 and step != int(n_train_step):
            names += [f"depth_model-{step}.pth", f"pose_model-{step}.pth"]
        for name in names:
            path = os.path.join(checkpoint_path, name)
            if os.path.exists(path):
                os.remove(path)
                removed.append(path)
    return removed


def _stored_results(state: dict):
    """What a call returns for a run that an earlier session finished: the last state's values, no checkpoint path."""
    return ({"train_step": state["step"], "best_results": state["best_results"], "finished": True, "resumed_from": state["step"],
             "digest": state["digest"]}, list(state["logged"]), [])


class Budget:
    """When a session ends before the run does: after `max_steps` steps of this session, once `max_seconds` of host time have
    passed since the context was entered (`clock`, time.monotonic; read between steps, nothing waits for the device), or when one of
    `stop_signals` has arrived.  As a context it installs a handler for each signal that sets a flag and does nothing else -- the
    step in progress completes -- and puts the previous handlers back on the way out, whatever happened inside.  Python installs
    handlers on the main thread only; on another thread none is installed and the two other limits work alone."""

    def __init__(self, max_steps=None, max_seconds=None, stop_signals=(signal.SIGTERM,), clock=time.monotonic):
        if max_steps is not None and (isinstance(max_steps, bool) or int(max_steps) != max_steps or max_steps < 1):
            raise KbnError(f"train_resumable: max_steps {max_steps!r}: None or at least one step a session")
        if max_seconds is not None and not float(max_seconds) > 0:
            raise KbnError(f"train_resumable: max_seconds {max_seconds!r}: None or a positive number")
        self.max_steps = None if max_steps is None else int(max_steps)
        self.max_seconds = None if max_seconds is None else float(max_seconds)
        self.stop_signals = tuple(stop_signals or ())
        self.clock = clock
        self.steps, self.started, self.signalled, self.installed = 0, clock(), None, {}

    def _flag(self, number, frame):
        self.signalled = number

    def __enter__(self):
        self.started = self.clock()
        if threading.current_thread() is threading.main_thread():
            try:
                for number in self.stop_signals:
                    self.installed[number] = signal.signal(number, self._flag)
            except BaseException:
                self.__exit__(None, None, None)
                raise
        return self

    def __exit__(self, *exc):
        while self.installed:
            number, previous = self.installed.popitem()
            signal.signal(number, signal.SIG_DFL if previous is None else previous)
        return False

    def step_done(self):
        """Counts a step of the session -> why the session ends here ('signal <n>', 'max_steps', 'max_seconds'), or None."""
        self.steps += 1
        if self.signalled is not None:
            return f"signal {int(self.signalled)}"
        if self.max_steps is not None and self.steps >= self.max_steps:
            return "max_steps"
        if self.max_seconds is not None and self.clock() - self.started >= self.max_seconds:
            return "max_seconds"
        return None


class _Session:
    """What train_resumable() adds to the loop: the state it continues from, the files written whole, the states pruned."""

    def __init__(self, budget: Budget, keep_states: int):
        if isinstance(keep_states, bool) or int(keep_states) != keep_states or keep_states < 1:
            raise KbnError(f"train_resumable: keep_states {keep_states!r}: at least one state is kept")
        self.budget, self.keep_states = budget, int(keep_states)
        self.checkpoint_path, self.record, self.skipped = None, None, []
        self.n_train_step = self.n_checkpoint = None
        self.vote = dist.StopVote(0, 1)      # of one process; the loop of several ranks puts theirs here

    def start(self, checkpoint_path, n_checkpoint, rank=0, world=1):
        """-> the newest complete state of `checkpoint_path`, or None for a fresh start.  Reads only.  With several ranks rank 0
        looks (find_state) and its answer -- a step or none, and the messages -- is everybody's: a file system may show one rank a
        newest state cut short and another the whole of it.  Every rank then loads that one file.  The loop checks the state's
        record against the call's (_resume_point), on every rank, and leaves the record and the run's steps here."""
        self.checkpoint_path, self.n_checkpoint = checkpoint_path, int(n_checkpoint)
        if world == 1:
            state, self.skipped = find_state(checkpoint_path)
        else:
            state, found = None, None
            if rank == 0:
                state, skipped = find_state(checkpoint_path)
                found = (None if state is None else int(state["step"]), skipped)
            step, self.skipped = dist.broadcast_object(found, src=0)
            if step is not None and rank != 0:
                state = torch.load(os.path.join(checkpoint_path, STATE_FILE.format(step)), map_location="cpu")
        return state

    def step_done(self) -> bool:
        """After every step of the session, on every rank: does the session end here?  This rank's wish (Budget.step_done) goes
        through the ranks' vote, so the answer is the same everywhere."""
        return self.vote.vote(self.budget.step_done() is not None)

    def write(self, path, writer):
        """writer(temporary name), then the move into place: `path` holds the old bytes or the new ones, never a part of them."""
        part = path + ".part"
        writer(part)
        os.replace(part, path)

    def save_state(self, snapshot: dict):
        snapshot["arguments"] = self.record
        self.write(os.path.join(self.checkpoint_path, STATE_FILE.format(snapshot["step"])), lambda part: torch.save(snapshot, part))
        prune_states(self.checkpoint_path, self.keep_states, self.n_checkpoint, self.n_train_step, current=snapshot["step"])


def _new_session(max_steps, max_seconds, stop_signals, keep_states) -> _Session:
    """A session and its Budget (session.budget, the context the loop runs in), with the refusals of both."""
    return _Session(Budget(max_steps=max_steps, max_seconds=max_seconds, stop_signals=stop_signals), keep_states)


def _train_loop(train_image_path,
          train_sparse_depth_path,
          train_intrinsics_path,
          val_image_path,
          val_sparse_depth_path,
          val_intrinsics_path,
          val_ground_truth_path,
          # Batch settings
          n_batch=8,
          n_height=320,
          n_width=768,
          # Input settings
          input_channels_image=3,
          input_channels_depth=2,
          normalized_image_range=[0, 1],
          outlier_removal_kernel_size=7,
          outlier_removal_threshold=1.5,
          # Sparse to dense pool settings
          min_pool_sizes_sparse_to_dense_pool=[5, 7, 9, 11, 13],
          max_pool_sizes_sparse_to_dense_pool=[15, 17],
          n_convolution_sparse_to_dense_pool=3,
          n_filter_sparse_to_dense_pool=8,
          # Depth network settings
          n_filters_encoder_image=[48, 96, 192, 384, 384],
          n_filters_encoder_depth=[16, 32, 64, 128, 128],
          resolutions_backprojection=[0, 1, 2, 3],
          n_filters_decoder=[256, 128, 128, 64, 12],
          deconv_type="up",
          min_predict_depth=1.5,
          max_predict_depth=100.0,
          # Weight settings
          weight_initializer="xavier_normal",
          activation_func="leaky_relu",
          # Training settings
          learning_rates=[5e-5, 1e-4, 15e-5, 1e-4, 5e-5, 2e-5],
          learning_schedule=[2, 8, 20, 30, 45, 60],
          augmentation_probabilities=[1.00, 0.50, 0.25],
          augmentation_schedule=[50, 55, 60],
          augmentation_random_crop_type=["horizontal", "vertical", "anchored", "bottom"],
          augmentation_random_flip_type=["none"],
          augmentation_random_remove_points=[0.60, 0.70],
          augmentation_random_noise_type="none",
          augmentation_random_noise_spread=-1,
          # Loss function settings
          w_color=0.15,
          w_structure=0.95,
          w_sparse_depth=0.60,
          w_smoothness=0.04,
          w_weight_decay_depth=0.00,
          w_weight_decay_pose=0.00,
          # Evaluation settings
          min_evaluate_depth=0.00,
          max_evaluate_depth=100.0,
          # Checkpoint settings
          checkpoint_path="trained_kbnet",
          n_checkpoint=5000,
          n_summary=5000,
          n_summary_display=4,
          validation_start_step=200000,
          depth_model_restore_path=None,
          pose_model_restore_path=None,
          # Hardware settings
          device="cuda",
          n_thread=8,
          *,
          workers=None,
          val_batch_size=1,
          summary_writer_factory=summary.EventWriter,
          return_results=False,
          rank=0,
          world=1,
          sync_batch_norm=True,
          session=None):
    """The loop of train_ranks() and train_resumable(): train_ranks()'s arguments and `session`, the hooks of a resumable run
    (_Session; None for train_ranks: nothing of a session is read, written or checked).  The phases of a run, top to bottom; what
    they share is the _Run's."""
    arguments = dict(locals())      # before anything else is bound: what the call was given
    s = types.SimpleNamespace(**arguments)
    run = _Run(s)                                                    # the process checks; rank 0's random state on every rank
    contents = _path_lists(arguments)
    state, finished = run.resume_point(arguments, contents)          # refused or returned before anything is built or written
    if finished:
        return _stored_results(state) if s.return_results else None
    run.build_models(state)                                          # what they refuse is refused before anything is written
    run.join_ranks()
    run.build_loaders(contents)
    with _summary_writers(s.summary_writer_factory, run.event_path, run.main) as (run.train_summary_writer, run.val_summary_writer):
        if state is None:
            run.log_head(contents)
        run.begin(state)
        run.train_epochs()
        run.finish()
    return run.results()


def _path_lists(arguments: dict) -> dict:
    """PATH_ARGUMENTS name -> the paths its file lists: the three training lists, then the four validation lists where all four are
    given (validation is off otherwise, and none of them is read).  KbnError for lists of different lengths and for no frame."""
    def read(names, what, kinds):
        lists = {name: loader.read_paths(arguments[name]) for name in names}
        n_sample = len(lists[names[0]])
        for name, kind in zip(names[1:], kinds):
            if len(lists[name]) != n_sample:
                raise KbnError(f"train: {n_sample} {what} image paths, {len(lists[name])} {kind} paths")
        return lists

    contents = read(PATH_ARGUMENTS[:3], "training", ("sparse depth", "intrinsics"))
    if not contents[PATH_ARGUMENTS[0]]:
        raise KbnError(f"train: {arguments[PATH_ARGUMENTS[0]]} lists no frame")
    if all(arguments[name] is not None for name in PATH_ARGUMENTS[3:]):
        contents.update(read(PATH_ARGUMENTS[3:], "validation", ("sparse depth", "intrinsics", "ground truth")))
    return contents


def _resume_point(arguments: dict, world: int, state, contents=None):
    """Where a call stands in its run -> (the argument record, the run's steps, finished?).  arguments: the call's, bound with their
    defaults; state: the newest complete state of its checkpoint_path, or None; contents: the path lists, where the caller has read
    them already (the loop has: it refuses them before it looks for a state).  KbnError when the state's record is not this one;
    finished: the state is one of the run's last step."""
    if contents is None:
        contents = _path_lists(arguments)
    record = argument_record(arguments, contents)
    n_train_step = n_train_steps(len(contents[PATH_ARGUMENTS[0]]), arguments["n_batch"], arguments["learning_schedule"], world=world)
    if state is not None:
        check_argument_record(state["arguments"], record)
    return record, n_train_step, state is not None and state["step"] >= n_train_step


@contextlib.contextmanager
def _summary_writers(summary_writer_factory, event_path, main):
    """-> (the train writer, the val writer), on rank 0; (None, None) elsewhere, where the factory is not called.  An exception in
    the body closes what was opened and is the one raised: the writers' own close errors are swallowed.  On the normal path the train
    writer is closed, then the val writer whatever the first close did, and their errors propagate."""
    writers = []
    try:
        for which in ("-train", "-val") if main else ():
            writers.append(summary_writer_factory(event_path + which))
        yield writers if main else (None, None)
    except BaseException:
        for writer in writers:
            with contextlib.suppress(Exception):      # the run's own exception is the one to see
                writer.close()
        raise
    with contextlib.ExitStack() as closing:      # callbacks run last in, first out, each whatever the one before it raised
        for writer in reversed(writers):
            closing.callback(writer.close)


def _named(function, values: dict) -> dict:
    """The items of `values` that `function`'s parameter list names: its keyword arguments from the settings, listed nowhere twice."""
    return {name: values[name] for name in inspect.signature(function).parameters if name in values}


class _Schedules:
    """The run's place in its two schedules, the reference's src/kbnet.py:378-390: learning_rate and augmentation_probability are
    those of the last epoch advance() was called for.  A continuation replays advance() for every epoch up to its state's."""

    def __init__(self, learning_schedule, learning_rates, augmentation_schedule, augmentation_probabilities):
        self.learning_schedule, self.learning_rates = learning_schedule, learning_rates
        self.augmentation_schedule, self.augmentation_probabilities = augmentation_schedule, augmentation_probabilities
        self.learning_position, self.learning_rate = 0, learning_rates[0]
        self.augmentation_position, self.augmentation_probability = 0, augmentation_probabilities[0]

    def advance(self, epoch: int) -> bool:
        """The two moves at the start of `epoch` (1-based) -> did the learning rate move?"""
        self.learning_position, self.learning_rate, moved = scheduled(epoch, self.learning_position, self.learning_schedule, self.learning_rates)
        self.augmentation_position, self.augmentation_probability, _ = scheduled(
            epoch, self.augmentation_position, self.augmentation_schedule, self.augmentation_probabilities, frozen=-1 in self.augmentation_schedule)
        return moved


class _Run:
    """What a run of _train_loop holds between its phases and its steps: the settings `s` as the call gave them, the process's place
    among the ranks, the models, the optimizer, the loaders, the counters and the lists.  Its methods are the loop's phases, in the
    order _train_loop calls them, and the parts of a step; they read their arguments and these attributes, nothing else."""

    def __init__(self, s):
        """The process checks, and rank 0's random state on every rank."""
        if s.device != "cuda" and s.device != "gpu":
            raise KbnError(f"train: device {s.device!r}: the HIP path has no CPU fallback (the reference trains on the CPU for anything but 'cuda' / 'gpu')")
        self.device, rank, world = torch.device("cuda"), int(s.rank), int(s.world)
        if world < 1 or not 0 <= rank < world:
            raise KbnError(f"train_ranks: rank {rank} of world {world}")
        if world > 1 and not (torch.distributed.is_available() and torch.distributed.is_initialized()
                              and torch.distributed.get_world_size() == world and torch.distributed.get_rank() == rank):
            raise KbnError(f"train_ranks: rank {rank} of world {world} needs an initialised process group of that size (kb.dist.init, or "
                           "kb.training.launch, which starts the ranks)")
        self.s, self.session, self.rank, self.world = s, s.session, rank, world
        self.main, self.transforms_seed = rank == 0, None      # main: the rank that writes
        if world > 1:      # before anything is drawn: the weights' initialisation, the epoch's order, the crops, the augmentation
            dist.broadcast_rng_state(src=0)
            self.transforms_seed = dist.broadcast_object(torch.initial_seed(), src=0)
        self.workers = int(s.n_thread if s.workers is None else s.workers)
        if int(s.val_batch_size) < 1:
            raise KbnError(f"train: val_batch_size {s.val_batch_size}")

        self.depth_model_checkpoint_path = os.path.join(s.checkpoint_path, "depth_model-{}.pth")
        self.pose_model_checkpoint_path = os.path.join(s.checkpoint_path, "pose_model-{}.pth")
        self.log_path = os.path.join(s.checkpoint_path, "results.txt") if self.main else None      # rank 0 alone keeps a log
        self.event_path = os.path.join(s.checkpoint_path, "events")
        self.write = (lambda path, writer: writer(path)) if s.session is None else s.session.write      # a session's files appear whole

        self.best_results = {"step": -1, "mae": np.inf, "rmse": np.inf, "imae": np.inf, "irmse": np.inf}
        self.logged, self.checkpoints = [], []
        self.train_step, self.epoch, self.batch = 0, 0, -1      # the last step taken, and the epoch and the batch it was
        self.first_epoch, self.first_batch, self.resumed_from = 1, 0, None
        self.seconds_before, self.time_start = 0.0, None      # trained in earlier sessions; when this one began
        self.stopped, self.digest = False, None

    def log(self, text):
        if self.main:
            summary.log(text, self.log_path)

    # ---- the phases before the first step ----
    def resume_point(self, arguments, contents):
        """-> (the state a session continues from or None, is the run finished?): the newest complete state of checkpoint_path,
        which a changed argument refuses."""
        s, session = self.s, self.session
        state = None if session is None else session.start(s.checkpoint_path, s.n_checkpoint, self.rank, self.world)
        record, self.n_train_step, finished = _resume_point(arguments, self.world, state, contents)
        if session is not None:
            session.record, session.n_train_step = record, self.n_train_step
        return state, finished

    def build_models(self, state):
        """The depth model, then the pose model, then -- on a fresh start -- what the restore paths name."""
        s = self.s
        self.depth_model = KBNetModel(**_named(KBNetModel, dict(vars(s), device=self.device, trainable=True)))      # its fifteen settings
        self.depth_model.requires_grad_(True)
        self.parameters_depth_model = self.depth_model.parameters()

        self.pose_model = ResNetPoseNetModel(18, rotation_parameterization="axis", weight_initializer=s.weight_initializer, activation_func="relu",
                                             device=self.device, trainable=True)
        self.pose_model.requires_grad_(True).set_batch_norm("batch")      # the reference's pose_model.train()
        self.parameters_pose_model = self.pose_model.parameters()

        if state is None:      # a continuation restores its own checkpoints, with the optimizer, once that exists
            for model, path in ((self.depth_model, s.depth_model_restore_path), (self.pose_model, s.pose_model_restore_path)):
                if path is not None and path != "":
                    model.restore_model(path)

    def join_ranks(self):
        """Rank 0's parameters on every rank; the averager of the gradients; the pose model's BatchNorm over the frames of all."""
        self.averager = None
        if self.world > 1:
            self.averager = dist.GradientAverager(self.parameters_depth_model + self.parameters_pose_model, self.rank, self.world)      # the list the optimizer steps
            self.averager.broadcast_parameters()
            if self.s.sync_batch_norm:
                self.pose_model.sync_batch_norm(dist.BatchNormGroup(self.rank, self.world))

    def build_loaders(self, contents):
        """checkpoint_path, the first thing a run writes; the training loader and Transforms; the validation set."""
        s = self.s
        if self.main and not os.path.exists(s.checkpoint_path):
            os.makedirs(s.checkpoint_path)
        sharding = {} if self.world == 1 else {"rank": self.rank, "world": self.world, "crops": "global"}
        self.train_loader = loader.TrainingFrameLoader(*(contents[name] for name in PATH_ARGUMENTS[:3]), shape=(s.n_height, s.n_width),
                                                       random_crop_type=s.augmentation_random_crop_type, batch_size=s.n_batch, shuffle=True,
                                                       device=self.device, workers=self.workers, **sharding)
        self.train_transforms = transforms.Transforms(
            normalized_image_range=s.normalized_image_range, random_flip_type=s.augmentation_random_flip_type,
            random_remove_points=s.augmentation_random_remove_points, random_noise_type=s.augmentation_random_noise_type,
            random_noise_spread=s.augmentation_random_noise_spread, seed=self.transforms_seed)
        self.validation_available = PATH_ARGUMENTS[3] in contents
        if self.validation_available:      # every ground truth with its validity map, on the host
            self.ground_truths = [np.stack(loader.load_depth_with_validity_map(path), axis=-1) for path in contents[PATH_ARGUMENTS[6]]]
            self.val_dataloader = loader.InferenceFrameLoader(*(contents[name] for name in PATH_ARGUMENTS[3:6]), use_image_triplet=True,
                                                              batch_size=int(s.val_batch_size), device=self.device, workers=self.workers)

    def log_head(self, contents):
        """The head of results.txt, once, on the fresh start: the two path blocks and the six settings blocks."""
        s = self.s
        for title, names in (("Training input paths:", PATH_ARGUMENTS[:3]), ("Validation input paths:", PATH_ARGUMENTS[3:])):
            self.log(title)
            for name in names:
                self.log(getattr(s, name))
            self.log("")
        if self.main:      # every summary.log_*_settings function is given what its own parameter list names
            values = dict(vars(s), log_path=self.log_path, n_train_sample=len(contents[PATH_ARGUMENTS[0]]), n_train_step=self.n_train_step,
                          parameters_depth_model=self.parameters_depth_model, parameters_pose_model=self.parameters_pose_model,
                          summary_event_path=self.event_path, device=self.device)
            for name in ("input", "network", "training", "loss_func", "evaluation", "system"):
                function = getattr(summary, f"log_{name}_settings")
                function(**_named(function, values))

    def begin(self, state):
        """The schedules and the optimizer; the fresh start or the continuation from `state`; the ranks' vote; the clock."""
        s = self.s
        self.schedules = _Schedules(s.learning_schedule, s.learning_rates, s.augmentation_schedule, s.augmentation_probabilities)
        self.optimizer = optim.Adam([{"params": self.parameters_depth_model, "weight_decay": s.w_weight_decay_depth},
                                     {"params": self.parameters_pose_model, "weight_decay": s.w_weight_decay_pose}], lr=self.schedules.learning_rate)
        if state is None:
            self.log("Begin training...")
        else:
            self.resume(state)
        if self.session is not None and self.world > 1:      # on every rank, here: making the vote's group is a collective
            self.session.vote = dist.StopVote(self.rank, self.world)
        self.time_start = time.time()

    def resume(self, state):
        """The checkpoints of the state's step, the optimizer with them; every schedule position up to the state's epoch, replayed;
        the rest of that epoch, or -- after its last batch -- the next one with its own schedule moves."""
        for message in self.session.skipped:
            self.log(message)
        self.train_step = self.resumed_from = state["step"]
        self.depth_model.restore_model(self.depth_model_checkpoint_path.format(self.train_step), self.optimizer)
        self.pose_model.restore_model(self.pose_model_checkpoint_path.format(self.train_step))
        for epoch in range(1, state["epoch"] + 1):
            self.schedules.advance(epoch)
        self.set_learning_rate()
        self.first_epoch, self.first_batch = (state["epoch"], state["batch"]) if state["loader"] else (state["epoch"] + 1, 0)
        self.train_loader.load_state_dict(state["loader"])
        self.train_transforms.load_state_dict(state["transforms"])
        self.best_results, self.logged, self.seconds_before = state["best_results"], list(state["logged"]), float(state["seconds"])
        set_random_state(state["random"], self.device)      # last: building the models drew from the generators
        self.log("Resuming training from step {}...".format(self.train_step))

    def set_learning_rate(self):
        for g in self.optimizer.param_groups:
            g["lr"] = self.schedules.learning_rate

    # ---- the epochs ----
    def train_epochs(self):
        """Every step that is left, or every step until the session's end: self.stopped says which."""
        s, session = self.s, self.session
        for epoch in range(self.first_epoch, s.learning_schedule[-1] + 1):
            # not in the middle of the epoch a continuation starts in: its moves were replayed by resume()
            if self.first_batch == 0 and self.schedules.advance(epoch):
                self.set_learning_rate()
            batches, self.first_batch = enumerate(self.train_loader, self.first_batch), 0
            for batch, frames in batches:
                self.epoch, self.batch = epoch, batch
                taken = self.step(batch, frames)
                if taken is None:
                    continue
                loss, loss_info, shown, n_global = taken
                summary_step, checkpoint_step = (self.train_step % s.n_summary) == 0, (self.train_step % s.n_checkpoint) == 0
                if self.world > 1 and (summary_step or checkpoint_step):
                    loss = self.global_loss(loss_info, n_global)
                if summary_step:
                    self.summarise(loss_info, shown, n_global)
                if checkpoint_step:
                    self.checkpoint(loss)
                # every step of a session, on every rank, whatever the step: the ranks' vote is a collective (host-side; no
                # wait for the device), and the wish of any rank during step s stops them all after step s
                if session is not None and session.step_done() and self.train_step < self.n_train_step:
                    # the session ends here, the step complete: off the checkpoint grid its two checkpoints and its state are
                    # written now (on the grid they just were), and neither a Step= line nor a validation is
                    if not checkpoint_step:
                        self.write_checkpoints()
                        self.save_state()
                    self.stopped = True
                    return

    def step(self, batch, frames):
        """One training step on this rank's frames of global batch `batch` -> (the loss, loss_info, the tensors a summary shows, the
        global batch's frame count), or None for a global batch of fewer frames than ranks: the same answer on every rank, no step."""
        s = self.s
        image0, image1, image2, sparse_depth0, intrinsics = frames
        shard = n_global = None
        if self.world > 1:
            n_global = self.train_loader.global_batch_size(batch)
            if not dist.every_rank_has_frames(n_global, self.world):
                return None
            shard = (dist.shard_bounds(n_global, self.rank, self.world)[0], n_global)
        self.train_step = self.train_step + 1
        image0, image1, image2, sparse_depth0, filtered_sparse_depth0, filtered_validity_map_depth0 = transforms.train_inputs(
            self.train_transforms, image0, image1, image2, sparse_depth0, self.schedules.augmentation_probability,
            kernel_size=s.outlier_removal_kernel_size, threshold=s.outlier_removal_threshold, shard=shard)
        output_depth0 = self.depth_model.forward(image=image0, sparse_depth=sparse_depth0,
                                                 validity_map_depth=filtered_validity_map_depth0, intrinsics=intrinsics)
        pose01 = self.pose_model.forward(image0, image1)
        pose02 = self.pose_model.forward(image0, image2)
        loss, loss_info = self.depth_model.compute_loss(
            image0=image0, image1=image1, image2=image2, output_depth0=output_depth0, sparse_depth0=filtered_sparse_depth0,
            validity_map_depth0=filtered_validity_map_depth0, intrinsics=intrinsics, pose01=pose01, pose02=pose02,
            w_color=s.w_color, w_structure=s.w_structure, w_sparse_depth=s.w_sparse_depth, w_smoothness=s.w_smoothness)
        self.optimizer.zero_grad()
        loss.backward()
        if self.averager is not None:
            self.averager.average(image0.shape[0], n_global)
        self.optimizer.step()
        shown = dict(image0=image0, output_depth0=output_depth0, sparse_depth0=filtered_sparse_depth0,
                     validity_map0=filtered_validity_map_depth0, pose01=pose01, pose02=pose02)
        return loss, loss_info, shown, n_global

    def global_loss(self, loss_info, n_global):
        """The global batch's loss, only where the loop waits anyway: the frames' four terms summed over the ranks in fp64, then
        compute_loss's own expressions -> the loss; loss_info holds it and its terms."""
        s = self.s
        terms = dist.sum_over_ranks(loss_info["per_frame"].sum(dim=0)) / n_global
        color, structure, sparse, smooth = terms.float().unbind(0)
        loss = s.w_color * color + s.w_structure * structure + s.w_sparse_depth * sparse + s.w_smoothness * smooth
        loss_info.update(loss_color=color, loss_structure=structure, loss_sparse_depth=sparse, loss_smoothness=smooth, loss=loss)
        return loss

    def summarise(self, loss_info, shown, n_global):
        """log_summary of the step: the whole global batch's, by rank 0."""
        shown = dict(shown, image01=loss_info.pop("image01"), image02=loss_info.pop("image02"), output_depth0=shown["output_depth0"].detach())
        loss_info.pop("per_frame")      # N x 4, this package's addition: a writer's add_scalar wants one number
        if self.world > 1:      # rank order is batch order; every n_summary steps, so its cost is not a concern
            shown = {name: dist.gather_frames(t, n_global, self.rank, self.world) for name, t in shown.items()}
        if self.main:
            self.depth_model.log_summary(summary_writer=self.train_summary_writer, tag="train", step=self.train_step, scalars=loss_info,
                                         n_display=min(self.s.n_batch, self.s.n_summary_display), **shown)

    def checkpoint(self, loss):
        """The Step= line, the validation, the two checkpoints and a session's state."""
        s = self.s
        value = loss.item()      # the loop's wait for the device, where the reference logs the loss
        time_elapse = (self.seconds_before + time.time() - self.time_start) / 3600
        time_remain = (self.n_train_step - self.train_step) * time_elapse / self.train_step
        self.log("Step={:6}/{}  Loss={:.5f}  Time Elapsed={:.2f}h  Time Remaining={:.2f}h".format(
            self.train_step, self.n_train_step, value, time_elapse, time_remain))
        self.logged.append((self.train_step, value))
        if self.train_step >= s.validation_start_step and self.validation_available:
            self.best_results = validation.validate(
                depth_model=self.depth_model, dataloader=self.val_dataloader, ground_truths=self.ground_truths, step=self.train_step,
                best_results=self.best_results, min_evaluate_depth=s.min_evaluate_depth, max_evaluate_depth=s.max_evaluate_depth,
                device=self.device, summary_writer=self.val_summary_writer, n_summary_display=s.n_summary_display, log_path=self.log_path,
                outlier_removal_kernel_size=s.outlier_removal_kernel_size, outlier_removal_threshold=s.outlier_removal_threshold,
                normalized_image_range=s.normalized_image_range)
        self.write_checkpoints()
        if self.train_step < self.n_train_step:      # the last step's state follows the loop
            self.save_state()

    # ---- what a step leaves on the disk ----
    def write_checkpoints(self):
        """The two checkpoints of the last step taken: written by rank 0, and their paths noted on every rank, once."""
        for model, pattern in ((self.depth_model, self.depth_model_checkpoint_path), (self.pose_model, self.pose_model_checkpoint_path)):
            path = pattern.format(self.train_step)
            if self.main:
                self.write(path, lambda part: model.save_model(part, self.train_step, self.optimizer))
            if path not in self.checkpoints:
                self.checkpoints.append(path)

    def snapshot(self, digest=None):
        """What a continuation needs beyond the two checkpoints; no wait for the device."""
        return {"step": self.train_step, "epoch": self.epoch, "batch": self.batch + 1, "loader": self.train_loader.state_dict(),
                "transforms": self.train_transforms.state_dict(), "random": random_state(self.device),
                "best_results": {k: _plain(v) for k, v in self.best_results.items()}, "logged": list(self.logged),
                "seconds": self.seconds_before + time.time() - self.time_start, "digest": digest}

    def save_state(self, digest=None):
        """A session's state of the last step taken, by rank 0."""
        if self.session is not None and self.main:
            self.session.save_state(self.snapshot(digest))

    # ---- the end ----
    def finish(self):
        """After the last step: the final checkpoints, the digest, the last state, and no rank leaves before rank 0 has written."""
        if not self.stopped:
            self.write_checkpoints()
        if self.world > 1 or (self.session is not None and (self.s.return_results or not self.stopped)):
            self.digest = replica_digest((self.depth_model, self.pose_model), self.optimizer)
        if not self.stopped:
            self.save_state(self.digest)
        if self.world > 1:
            dist.barrier()      # no rank leaves, and nobody reads the checkpoints or the state, before rank 0 has written them

    def results(self):
        if not self.s.return_results:
            return None
        results = {"train_step": self.train_step, "best_results": self.best_results}
        if self.world > 1:
            results["digest"] = self.digest      # of this rank's replica: the one value that may differ between ranks, and must not
        if self.session is not None:
            results.update(finished=not self.stopped, resumed_from=self.resumed_from, digest=self.digest)
        return results, self.logged, self.checkpoints


def train_ranks(*arguments, **keywords):
    """train() with three more keyword-only arguments -- rank, world, sync_batch_norm -- and everything train()'s docstring says.

    Data-parallel training: `rank` of `world` processes, one a GPU, each calling train_ranks() with the same arguments inside an
    initialised process group (kb.dist.init; KbnError otherwise, before anything is written) on its current device -- launch()
    below starts them ("On several GPUs").  n_batch stays the GLOBAL batch.  With the ranks started from one set of seeds, the tensors every rank feeds
    its networks are, bit for bit, its dist.shard_bounds slice of the batch a one-process train() builds under those seeds -- crop,
    flips, removed points and noise -- and the logged loss, the summaries, results.txt and the checkpoints are those of the
    global batch, written once, by rank 0.  In this order:
      * rank 0's random state becomes everybody's before anything is drawn (dist.broadcast_rng_state), and rank 0's
        torch.initial_seed() every rank's Transforms.seed;
      * both models are built, and restored, on every rank; GradientAverager.broadcast_parameters(); the pose model's BatchNorm
        layers normalise over the frames of all ranks (sync_batch_norm(BatchNormGroup)) unless sync_batch_norm=False, which gives
        the reference's DataParallel behaviour -- every replica normalises with its own shard's statistics, the reduced gradient
        is then not the whole batch's, and the checkpoint holds rank 0's running statistics;
      * the loader shards every global batch and draws the crops of all of it (crops="global"), Transforms draws for all of it
        (shard=); a global batch of fewer frames than ranks is skipped on every rank and is no step (n_train_steps(world=));
      * every step: the forwards and the backward on the rank's frames, GradientAverager.average(n_local, n_global), the optimizer's
        step on the reduced gradients -- no collective besides the averager's and BatchNorm's;
      * at a checkpoint or summary step, where the loop waits anyway, the ranks' per-frame loss terms are summed (one all-reduce
        of four fp64 numbers): Loss= and the scalars are the global batch's, sum over ranks of n_local / n_global x the rank's;
      * at a summary step the tensors log_summary takes are gathered in rank order, which is batch order, and rank 0 makes the one
        call: histograms and panels are the whole batch's;
      * writers (summary_writer_factory is not called elsewhere), results.txt and checkpoints are rank 0's alone; a barrier follows
        the last save_model;
      * validate() runs on every rank over the whole validation set -- the replicas are bit-identical, so are the numbers and
        best_results; only rank 0 has a writer and a log.  Sharding the validation set is not built.
    With return_results every rank returns the same values; the dict has one more key, 'digest': replica_digest() of the rank's
    final parameters, buffers and optimizer state, equal on every rank while the replicas are bit-identical (they are with
    sync_batch_norm=True; with False the BatchNorm running statistics are per rank).  world=1 is the one-process path, bit for bit."""
    bound = _RANKS_SIGNATURE.bind(*arguments, **keywords)
    return _train_loop(*bound.args, **bound.kwargs)


def train(*arguments, **keywords):
    """The reference's train() (src/kbnet.py:31-518): its arguments, names, order and defaults (src/global_constants.py), then
    keyword-only workers (host threads of the two loaders; None: n_thread), val_batch_size (frames a validation forward),
    summary_writer_factory (called with event_path + '-train' and event_path + '-val'; any object with add_scalar, add_histogram,
    add_image and close fits) and return_results.

    The four path arguments of each set are newline-delimited files of paths (loader.read_paths); a validation argument that is
    None switches validation off.  Writes checkpoint_path/results.txt (the two path blocks, the six settings blocks, a line every
    n_checkpoint steps, validate()'s lines), checkpoint_path/depth_model-<step>.pth and pose_model-<step>.pth every n_checkpoint
    steps and after the last epoch, and the two event directories checkpoint_path/events-train and events-val.

    Returns None, as the reference; with return_results a tuple: {'train_step', 'best_results'}, the list of (step, loss) logged at
    the checkpoints, and the checkpoint paths written, depth and pose model alternating.

    The loop waits for the device where the reference logs the loss, at a checkpoint (loss.item()), and in validate(); between
    checkpoints nothing does.  Differences from the reference, on purpose: the shuffle order and the augmentation draws
    (loader.TrainingFrameLoader, transforms.Transforms); validation runs val_batch_size frames a forward; device 'cpu' and path
    lists of different lengths raise KbnError; a configuration the backward pass does not serve (deconv_type='transpose') raises
    before anything is written; restore_model's and the writers' errors propagate; neither model's train() / eval() is called
    (KBNetModel has one mode, the pose model's batch statistics are set_batch_norm('batch')).

    One process, one GPU: train_ranks() below is this function run by one process a GPU ("On several GPUs"), and
    launch() starts those processes."""
    bound = _TRAIN_SIGNATURE.bind(*arguments, **keywords)      # TypeError for rank, world, sync_batch_norm: they are train_ranks()'s
    return train_ranks(*bound.args, **bound.kwargs)


def train_resumable(*arguments, max_steps=None, max_seconds=None, stop_signals=(signal.SIGTERM,), keep_states=2, **keywords):
    """train() in sessions: train()'s arguments, names, order and defaults, and four more keyword-only ones.  The same call, made
    in one job slot after another, carries a run to its end, and the run it makes is, bit for bit, the one an uninterrupted
    train() makes under the seeds of the first session ("Training in job slots").

    A call looks for the newest complete training state in checkpoint_path (find_state).  None: a fresh start, as train()'s, the two
    restore paths honoured.  One of the last step: the run is finished, the call returns at once and writes nothing.  Otherwise it
    continues after that state's step: the two checkpoints of the step with the optimizer's state, the loader's place in its epoch
    with the crops already drawn ahead (TrainingFrameLoader.load_state_dict), Transforms' seed and call count, NumPy's, torch's and
    the device's generator states, best_results, the logged losses and the time trained so far; the schedule positions are
    replayed.  Every argument that shapes the trajectory must be what the first session was given (argument_record; KbnError names
    the first that differs, before anything is written); checkpoint_path, the restore paths, device, n_thread, workers, the
    writers' factory and return_results may change.

    The session ends early -- the step in progress always completes -- after max_steps steps, after max_seconds of host time
    since the call began (read between steps; no step waits for the device that does not in train()), or when one of stop_signals
    arrives (Budget: the handlers set a flag, are installed on the main thread only and are put back on return or error).
    checkpoint_path/train_state-<step>.pth is written after the two checkpoints of every n_checkpoint-th step, of the step a
    session stops at (that step's two checkpoints with it when it is off the grid; no Step= line, no validation) and of the last
    step.  Each of the three files is written under a temporary name and moved into place.  keep_states states are kept; an older
    one goes, and with it the checkpoints of a stop's step; those of the grid and of the last step stay.

    results.txt: the path and settings blocks once, "Resuming training from step <s>..." where a continuation begins, Time Elapsed
    over all sessions.  Every session opens its own event files.  With return_results the results dict has three more keys:
    'finished', 'resumed_from' (a step or None) and 'digest' (replica_digest of what the session ended with); the logged list
    is the whole run's, the checkpoint paths are this session's.

    One process, one GPU.  A data-parallel run (train_ranks, launch) is continued by train_ranks_resumable() and
    launch_resumable() below."""
    bound = _TRAIN_SIGNATURE.bind(*arguments, **keywords)
    session = _new_session(max_steps, max_seconds, stop_signals, keep_states)
    with session.budget:
        return _train_loop(*bound.args, **bound.kwargs, session=session)


def train_ranks_resumable(*arguments, max_steps=None, max_seconds=None, stop_signals=(signal.SIGTERM,), keep_states=2, **keywords):
    """train_ranks() in sessions: train_ranks()'s arguments, names, order and defaults (rank, world, sync_batch_norm too) and
    train_resumable()'s four keyword-only ones, with everything the two docstrings say.  `world` processes, each calling it with
    the same arguments inside an initialised process group -- launch_resumable() below starts them -- carry one data-parallel run
    through job slots, and the run they make is, bit for bit, the one an uninterrupted launch() makes under the seeds of the first
    session ("Training in job slots").  world=1 is train_resumable(), bit for bit.

    What several ranks add to a session:
      * the stop is agreed.  Signals and clocks differ between ranks, and a rank that left the loop alone would leave the others
        waiting in the next step's all-reduce.  After EVERY step every rank takes part in one vote (kb.dist.StopVote: a MAX
        all-reduce of one integer on a CPU tensor over gloo -- a gloo group beside an RCCL default group); the session ends after
        step s on every rank if any rank's Budget wished so during step s.  The vote is host-side: no step waits for the device
        that does not in train_ranks();
      * rank 0 alone writes the two checkpoints and train_state-<step>.pth, under temporary names moved into place, and prunes; the
        final barrier follows the last state;
      * rank 0 alone looks for the state (find_state); the step it found and the messages for the states it passed over are
        broadcast, every rank loads that one file and the two checkpoints of its step.  The state is one process's: the loader's is
        the global one (TrainingFrameLoader.state_dict with crops="global": the plans of whole global batches, of which every rank
        takes its shard), the generators are rank 0's, set last on every rank -- the ranks draw alike, as after
        dist.broadcast_rng_state on a fresh start;
      * the argument record holds world and sync_batch_norm too: a continuation with another value raises KbnError naming it, on
        every rank, before anything is written.  A continuation at another world is not built.  The process group's backend and
        the ranks' devices are not recorded and may change, as device may; a backend that sums in another order then gives
        other bits from there on.
    With return_results every rank returns the same values."""
    bound = _RANKS_SIGNATURE.bind(*arguments, **keywords)
    session = _new_session(max_steps, max_seconds, stop_signals, keep_states)
    with session.budget:
        return _train_loop(*bound.args, **bound.kwargs, session=session)


# train()'s signature is the reference's and stays it: the loop's without its four last arguments, written once
_RANKS_SIGNATURE = inspect.signature(_train_loop)
_RANKS_SIGNATURE = _RANKS_SIGNATURE.replace(parameters=[p for p in _RANKS_SIGNATURE.parameters.values() if p.name != "session"])
_TRAIN_SIGNATURE = _RANKS_SIGNATURE.replace(parameters=[p for p in _RANKS_SIGNATURE.parameters.values()
                                                        if p.name not in ("rank", "world", "sync_batch_norm")])
train_ranks.__signature__ = _RANKS_SIGNATURE
train.__signature__ = _TRAIN_SIGNATURE
_SESSION_PARAMETERS = [inspect.Parameter(name, inspect.Parameter.KEYWORD_ONLY, default=default)
                       for name, default in (("max_steps", None), ("max_seconds", None), ("stop_signals", (signal.SIGTERM,)), ("keep_states", 2))]
train_resumable.__signature__ = _TRAIN_SIGNATURE.replace(parameters=list(_TRAIN_SIGNATURE.parameters.values()) + _SESSION_PARAMETERS)
train_ranks_resumable.__signature__ = _RANKS_SIGNATURE.replace(parameters=list(_RANKS_SIGNATURE.parameters.values()) + _SESSION_PARAMETERS)


# ------------------------------------------------------------------------------------------------ one process per GPU
MAX_RANKS = 16
ARGUMENTS_FILE, RESULTS_FILE = "launch-arguments.pkl", "launch-results.pkl"


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _tail(path: str, lines: int = 20) -> str:
    try:
        with open(path, errors="replace") as f:
            return "".join(f.readlines()[-lines:])
    except OSError:
        return ""


def launch(n_gpus, *, backend="nccl", devices=None, timeout=None, **train_arguments):
    """train_ranks() on `n_gpus` GPUs of this host: starts one fresh child process a rank (subprocess; no process's program is ever
    replaced), waits for them, and returns rank 0's return_results tuple.  The calling process does not need the GPU and does not
    touch it.

    train_arguments: train()'s arguments by name (the seven path arguments too), without rank, world and return_results.  They
    travel to the children through a file, checkpoint_path/launch-arguments.pkl, so they must pickle (a summary_writer_factory
    that is a class or a module-level function does).  With them travels the caller's random state: the children start from
    NumPy's global state and torch's CPU generator as they are here, and from torch.manual_seed(torch.initial_seed()) for the
    device generators -- so launch() under a seed trains as train() called in its place under that seed would.

    Each child gets RANK, LOCAL_RANK, WORLD_SIZE, MASTER_ADDR=127.0.0.1 and MASTER_PORT (a free port) in its environment, selects
    its device, runs kb.dist.init(backend) and then train_ranks(..., rank=rank, world=n_gpus).  devices: the device index of every rank;
    None: rank r on device r.  Ranks may share a device under backend="gloo" ([0, 0]: two ranks on one GPU, the tests' form);
    "nccl" (RCCL) needs a device a rank.  Host thread counts come from n_thread / workers alone.  The children's output goes to
    checkpoint_path/rank<r>.out and rank<r>.err, never to pipes: a rank whose pipe is full would keep the others waiting in a
    collective.  Every rank also leaves checkpoint_path/rank<r>.digest, replica_digest() of what it holds at the end.

    1 <= n_gpus <= 16 and len(devices) == n_gpus, else KbnError before anything is started or written.  The first child to exit
    with a non-zero status, or `timeout` seconds for the whole run (None: no limit), ends the others; launch then raises KbnError
    with that rank's last lines of stderr."""
    world, devices, checkpoint_path, threads = _launch_checks("launch", n_gpus, backend, devices, timeout, train_arguments)
    arguments_path, results_path = _write_launch_arguments(checkpoint_path, backend=backend, devices=devices, train=train_arguments, threads=threads)
    _run_children("launch", _child_command(arguments_path), devices, checkpoint_path, threads, timeout)
    return _launch_results("launch", results_path)


def _write_launch_arguments(checkpoint_path, **travelling):
    """What the ranks of a launch read, into checkpoint_path/launch-arguments.pkl: `travelling`, the caller's random state and where
    rank 0 leaves its results; an older results file goes -> (the arguments file, the results file)."""
    os.makedirs(checkpoint_path, exist_ok=True)
    arguments_path, results_path = os.path.join(checkpoint_path, ARGUMENTS_FILE), os.path.join(checkpoint_path, RESULTS_FILE)
    if os.path.exists(results_path):
        os.remove(results_path)
    with open(arguments_path, "wb") as f:
        pickle.dump(dict(travelling, results=results_path, random=(np.random.get_state(), torch.get_rng_state(), torch.initial_seed())), f)
    return arguments_path, results_path


def _launch_checks(what, n_gpus, backend, devices, timeout, train_arguments):
    """What launch() and launch_resumable() refuse before anything is started or written -> (world, devices, checkpoint_path, the
    children's host threads)."""
    if isinstance(n_gpus, bool) or not isinstance(n_gpus, (int, np.integer)) or not 1 <= int(n_gpus) <= MAX_RANKS:
        raise KbnError(f"{what}: n_gpus {n_gpus!r}: 1 to {MAX_RANKS} ranks")
    world = int(n_gpus)
    if devices is None:
        devices = list(range(world))
    devices = [int(d) for d in devices]
    if len(devices) != world or any(d < 0 for d in devices):
        raise KbnError(f"{what}: devices {devices}: one device index for each of the {world} ranks")
    if backend not in ("nccl", "gloo"):
        raise KbnError(f"{what}: backend {backend!r}: 'nccl' (RCCL) or 'gloo'")
    if backend == "nccl" and len(set(devices)) != world:
        raise KbnError(f"{what}: devices {devices}: RCCL needs a device a rank (ranks share one under backend='gloo')")
    for name in ("rank", "world", "return_results"):
        if name in train_arguments:
            raise KbnError(f"{what}: {name} is set by {what} itself")
    if timeout is not None and not float(timeout) > 0:
        raise KbnError(f"{what}: timeout {timeout!r}")
    checkpoint_path = train_arguments.get("checkpoint_path", "trained_kbnet")
    threads = train_arguments.get("workers")
    threads = max(1, int(train_arguments.get("n_thread", 8) if threads is None else threads))
    return world, devices, checkpoint_path, threads


def _child_command(arguments_path: str, stop_signals=()) -> list:
    """The command line of a rank: a fresh interpreter that imports this package from where it lies and runs _rank_main.  A child
    of launch_resumable() first gives every stop signal a handler that only notes it: one that arrives while the package is still
    being imported must not end the rank (_rank_main hands what was noted to the session's Budget)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    early = ""
    if stop_signals:
        early = (f"import signal; early = []; [signal.signal(number, lambda number, frame: early.append(number)) "
                 f"for number in {[int(number) for number in stop_signals]!r}]; ")
    program = ("import sys; " + early + "sys.path.insert(0, sys.argv[1]); import kbnet_amd; kbnet_amd.training._rank_main(sys.argv[2]"
               + (", early" if stop_signals else "") + ")")
    return [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", program, root, arguments_path]


def _run_children(what, command, devices, checkpoint_path, threads, timeout, session_mark=None, arrivals=None) -> None:
    """Starts `command` once a rank, waits for all of them, and raises KbnError for the first that exits with a non-zero status or
    when `timeout` seconds have passed; no child outlives the call.  session_mark: the rank<r>.out / .err files are opened for
    appending and begin with that line (launch_resumable); None: they are written anew.  arrivals: a list a signal handler of the
    caller appends signal numbers to; each is sent on, once, to every child still running."""
    world = len(devices)
    port = _free_port()
    children, logs, forwarded = [], [], 0
    try:
        for rank in range(world):
            env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(devices[rank]), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                       MASTER_PORT=str(port))
            env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: RCCL between processes needs it (as bench.py sets it)
            env.setdefault("OMP_NUM_THREADS", str(threads))
            out = open(os.path.join(checkpoint_path, f"rank{rank}.out"), "w" if session_mark is None else "a")
            err = open(os.path.join(checkpoint_path, f"rank{rank}.err"), "w" if session_mark is None else "a")
            logs += [out, err]
            if session_mark is not None:
                for f in (out, err):
                    f.write(session_mark + "\n")
                    f.flush()
            children.append(subprocess.Popen(command, stdin=subprocess.DEVNULL, stdout=out, stderr=err, env=env))
        deadline = None if timeout is None else time.monotonic() + float(timeout)
        failed = None      # (rank, why)
        while failed is None and any(c.poll() is None for c in children):
            while arrivals is not None and forwarded < len(arrivals):
                for child in children:
                    if child.poll() is None:
                        child.send_signal(arrivals[forwarded])
                forwarded += 1
            for rank, child in enumerate(children):
                if child.poll() is not None and child.returncode != 0:
                    failed = (rank, f"exited with status {child.returncode}")
                    break
            else:
                if deadline is not None and time.monotonic() > deadline:
                    rank = next(r for r, c in enumerate(children) if c.poll() is None)
                    failed = (rank, f"was still running after the timeout of {float(timeout):g} s")
                else:
                    time.sleep(0.05)
        if failed is None:
            failed = next(((r, f"exited with status {c.returncode}") for r, c in enumerate(children) if c.returncode != 0), None)
    finally:
        for child in children:
            if child.poll() is None:
                child.kill()
                child.wait()
        for f in logs:
            f.close()
    if failed is not None:
        rank, why = failed
        raise KbnError(f"{what}: rank {rank} of {world} {why}; the end of {os.path.join(checkpoint_path, f'rank{rank}.err')}:\n"
                       + _tail(os.path.join(checkpoint_path, f"rank{rank}.err")))


def _launch_results(what, results_path):
    if not os.path.exists(results_path):
        raise KbnError(f"{what}: every rank exited with status 0, but rank 0 left no {results_path}")
    with open(results_path, "rb") as f:
        return pickle.load(f)


class _Arrivals(Budget):
    """Budget's handlers -- installed on the main thread only, the previous ones back on every way out -- noting every signal that
    arrives, in order, for launch_resumable() to send on."""

    def __init__(self, stop_signals):
        super().__init__(stop_signals=stop_signals)
        self.arrived = []

    def _flag(self, number, frame):
        self.arrived.append(number)


def launch_resumable(n_gpus, *, backend="nccl", devices=None, timeout=None, max_steps=None, max_seconds=None,
                     stop_signals=(signal.SIGTERM,), keep_states=2, **train_arguments):
    """launch() with children that run train_ranks_resumable(): launch()'s arguments and train_resumable()'s four, and everything
    the three docstrings say.  The same call, made in one job slot after another -- `timeout -k 10 <slot> python job.py` is the
    intended use -- carries a run on `n_gpus` GPUs to its end ("Training in job slots").

    Before anything is started the launcher itself looks for the run's newest complete state (find_state: host code, no GPU).  A
    state whose arguments are not this call's -- world and sync_batch_norm among them -- raises KbnError naming the first, and
    nothing is written.  A state of the run's last step (n_train_steps(..., world=n_gpus)): the run is finished, the call returns
    the stored results at once, starts no child and writes nothing.

    While it waits the launcher holds handlers for stop_signals that only note the signal (on the main thread; the previous handlers
    are back on every way out), and its polling loop sends each noted signal on, once, to every child still running.  The children
    hold handlers of their own from their first line on (their session's Budget), so a scheduler that signals the whole process
    group ends nobody either: every rank finishes its step, the ranks agree on the stop, rank 0 writes the state, and the call
    returns that session's results with finished=False.  max_steps and max_seconds are the children's, max_seconds counted from
    each child's start.  `timeout` keeps launch()'s meaning: it ends the children hard, and the call raises.  A child that raises
    is ended with the others and reported, as in launch().

    rank<r>.out and rank<r>.err are appended to, each session under a line that marks it; launch-results.pkl is rank 0's result of
    the last session, rank<r>.digest every rank's replica_digest() of what it held when that session ended.  backend and devices
    are not part of the run's record and may change between sessions, as device may; with a backend that sums in another order the
    bits differ from there on."""
    what = "launch_resumable"
    world, devices, checkpoint_path, threads = _launch_checks(what, n_gpus, backend, devices, timeout, train_arguments)
    _new_session(max_steps, max_seconds, stop_signals, keep_states)      # their refusals
    stop_signals = [int(number) for number in (stop_signals or ())]
    state, _ = find_state(checkpoint_path)
    if state is not None:
        bound = _RANKS_SIGNATURE.bind(**train_arguments, rank=0, world=world)
        bound.apply_defaults()
        _, _, finished = _resume_point(dict(bound.arguments), world, state)      # the loop's own check and answer
        if finished:
            return _stored_results(state)

    arguments_path, results_path = _write_launch_arguments(
        checkpoint_path, backend=backend, devices=devices, train=train_arguments, threads=threads,
        session={"max_steps": max_steps, "max_seconds": max_seconds, "stop_signals": stop_signals, "keep_states": keep_states})
    mark = "==== {}: a session {} ====".format(what, "from the start" if state is None else "after step {}".format(state["step"]))
    with _Arrivals(stop_signals) as arrivals:
        _run_children(what, _child_command(arguments_path, stop_signals), devices, checkpoint_path, threads, timeout,
                      session_mark=mark, arrivals=arrivals.arrived)
    return _launch_results(what, results_path)


def _rank_main(arguments_path: str, early=None) -> None:
    """What a child of launch() runs: the device, the caller's random state, the process group, train_ranks(), and rank 0's results into
    a file.  A child of launch_resumable() runs train_ranks_resumable()'s body instead, with the session's Budget entered here,
    before the GPU is touched: its handlers hold from the first line on, and a signal noted before it (`early`, the command line's
    list) is the Budget's."""
    with open(arguments_path, "rb") as f:
        arguments = pickle.load(f)
    limits = arguments.get("session")
    if limits is None:
        return _rank_run(arguments, None)
    session = _new_session(**limits)
    with session.budget:
        if early:
            session.budget.signalled = early[0]
        return _rank_run(arguments, session)


def _rank_run(arguments: dict, session) -> None:
    rank, _, world = dist.env_world()
    torch.set_num_threads(arguments["threads"])
    torch.cuda.set_device(arguments["devices"][rank])
    numpy_state, cpu_state, seed = arguments["random"]
    torch.manual_seed(seed)      # every generator, the device's too, and torch.initial_seed()
    torch.set_rng_state(cpu_state)
    np.random.set_state(numpy_state)
    if world > 1:
        dist.init(arguments["backend"])
    if session is None:
        results = train_ranks(**arguments["train"], rank=rank, world=world, return_results=True)
    else:
        bound = _RANKS_SIGNATURE.bind(**arguments["train"], rank=rank, world=world, return_results=True)
        results = _train_loop(*bound.args, **bound.kwargs, session=session)
    if world > 1:
        with open(os.path.join(os.path.dirname(arguments["results"]), f"rank{rank}.digest"), "w") as f:
            f.write(results[0]["digest"] + "\n")
    if rank == 0:
        with open(arguments["results"] + ".part", "wb") as f:
            pickle.dump(results, f)
        os.replace(arguments["results"] + ".part", arguments["results"])
    if world > 1:      # after a clean run only: a rank that failed leaves at once, and launch() ends the others
        torch.distributed.destroy_process_group()
