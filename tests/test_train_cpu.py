"""kb.training.train without a GPU: its signature against the reference's recorded one (tests/golden/train_kitti_narrow.npz), the
schedule arithmetic, and what it refuses before anything is written."""
import inspect
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kbnet_amd as kb  # noqa: E402
import run_cases as rc  # noqa: E402
import train_cases as tc  # noqa: E402

KbnError = kb._lib.KbnError


def test_signature_is_the_references():
    golden = np.load(tc.GOLDEN)
    names, defaults = [str(n) for n in golden["parameters"]], [str(d) for d in golden["defaults"]]
    assert len(names) == 54 and names[:7] == ["train_image_path", "train_sparse_depth_path", "train_intrinsics_path", "val_image_path",
                                              "val_sparse_depth_path", "val_intrinsics_path", "val_ground_truth_path"]
    parameters = inspect.signature(kb.training.train).parameters
    ours = [p for p in parameters.values() if p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]
    assert [p.name for p in ours] == names
    assert [repr(p.default) if p.default is not inspect.Parameter.empty else "<required>" for p in ours] == defaults
    extras = {p.name: p.default for p in parameters.values() if p.kind is inspect.Parameter.KEYWORD_ONLY}
    assert extras == {"workers": None, "val_batch_size": 1, "summary_writer_factory": kb.summary.EventWriter, "return_results": False}
    assert len(parameters) == len(names) + 4
    assert "INTEGRATION.md" in kb.training.train.__doc__ and "One process, one GPU" in kb.training.train.__doc__


def test_schedule_arithmetic():
    steps = kb.training.n_train_steps
    assert steps(3, 3, [1, 3]) == 3 and steps(1003, 8, [2, 8, 20, 30, 45, 60]) == 60 * 126 and steps(8, 8, [5]) == 5 and steps(9, 8, [5]) == 10
    assert isinstance(steps(3, 3, [1, 3]), int)

    def walk(schedule, values, epochs, frozen=False):
        position, out = 0, []
        for epoch in range(1, epochs + 1):
            position, value, moved = kb.training.scheduled(epoch, position, schedule, values, frozen=frozen)
            out.append((value, moved))
        return out

    assert walk([1, 3], [1e-4, 5e-5], 3) == [(1e-4, False), (5e-5, True), (5e-5, False)]
    rates = [5e-5, 1e-4, 15e-5]
    got = walk([2, 8, 20], rates, 20)
    assert [v for v, _ in got] == [rates[0]] * 2 + [rates[1]] * 6 + [rates[2]] * 12
    assert [e + 1 for e, (_, moved) in enumerate(got) if moved] == [3, 9]
    # one position an epoch, as the reference: a schedule that repeats an entry lags behind it
    assert [v for v, _ in walk([1, 1, 4], [1, 2, 3], 4)] == [1, 2, 3, 3]
    # the reference's `-1 in augmentation_schedule`: the first probability for the whole run
    assert walk([-1], [0.0], 3, frozen=True) == [(0.0, False)] * 3
    assert walk([50, 55, 60], [1.0, 0.5, 0.25], 60, frozen=False)[49:56] == [(1.0, False), (0.5, True)] + [(0.5, False)] * 4 + [(0.25, True)]
    # the golden's learning rates follow from it: checkpoints of steps 1, 2, 3 (one step an epoch)
    golden = np.load(tc.GOLDEN)
    by_step = {int(s): lr for s, lr in zip(golden["checkpoint_steps"], golden["checkpoint_lrs"])}
    assert {s: tuple(lr) for s, lr in by_step.items()} == {1: (1e-4, 1e-4), 2: (5e-5, 5e-5), 3: (5e-5, 5e-5)}


def test_refusals_come_before_anything_is_written(tmp_path):
    from kbnet_amd import loader
    lists = [str(tmp_path / name) for name in rc.write_lists(str(tmp_path), _write_paths)]
    settings = tc.train_settings(kb.kitti_config().narrow())
    out = str(tmp_path / "trained")
    with pytest.raises(KbnError, match="no CPU fallback"):
        kb.training.train(lists[0], lists[1], lists[2], lists[0], lists[1], lists[2], lists[3], checkpoint_path=out, device="cpu", **settings)
    short = str(tmp_path / "short.txt")
    _write_paths(short, loader.read_paths(lists[1])[:2])
    with pytest.raises(KbnError, match="3 training image paths, 2 sparse depth paths"):
        kb.training.train(lists[0], short, lists[2], lists[0], lists[1], lists[2], lists[3], checkpoint_path=out, device="cuda", **settings)
    with pytest.raises(KbnError, match="3 validation image paths, 2 ground truth paths"):
        kb.training.train(lists[0], lists[1], lists[2], lists[0], lists[1], lists[2], short, checkpoint_path=out, device="gpu", **settings)
    with pytest.raises(KbnError, match="transpose"):
        kb.training.train(lists[0], lists[1], lists[2], lists[0], lists[1], lists[2], lists[3], checkpoint_path=out, device="cuda",
                          **dict(settings, deconv_type="transpose"))
    with pytest.raises(KbnError, match="val_batch_size"):
        kb.training.train(lists[0], lists[1], lists[2], lists[0], lists[1], lists[2], lists[3], checkpoint_path=out, val_batch_size=0, **settings)
    assert not os.path.exists(out)


def _write_paths(filepath, paths):
    with open(filepath, "w") as f:
        f.write("\n".join(paths) + "\n")
