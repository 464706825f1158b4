"""GPU: eight steps of kb.training.train against the fp64 restatement of the same run (tests/train_oracle.py), past the first step:
what the pieces do TOGETHER -- the schedules, Adam's state, the packed-weight caches, the BatchNorm running statistics, validate()
between steps -- compared with something independent of the package.

    python -m pytest tests/test_train_trajectory_gpu.py -m gpu -q -s

One train() run of eight steps on the three 24 x 40 frames (learning_schedule [3, 8], a checkpoint and a validation every step),
one fp64 oracle run and eight single fp64 oracle steps, shared through module fixtures.  Two modes:

  teacher-forced   for t = 1 .. 8 the fp64 oracle resumes from the DEVICE's checkpoint of step t - 1 (parameters, Adam's moments and
                   step counts, running statistics), takes one step, and is compared with the device's checkpoint of step t: every
                   step is a step-1-grade comparison, and a failure names its step.  The primary gates.
  free             the device's eight losses, its depth update at steps 4 and 8, its running statistics, the two networks as
                   functions (the depth output of the restored fused KBNetModel, the pose six-vectors of the restored pose model on
                   its running statistics) and the validation rows of its results.txt against the fp64 oracle's free run.

Every gate is 3 x the fixture's fp32 yardstick for that quantity and step (tests/golden/train_trajectory_kitti_narrow.npz: torch's
fp32 CPU kernels against fp64, the worst of twelve runs -- six frame orders, two image layouts; nothing of the device is in it),
floored at the package's own bar where the device arithmetic is not IEEE fp32 (train_oracle.FLOORS, metric_floor).  The
teacher-forced gates of the update ratios and of Adam's moments take the worst of steps 2 to 8 instead of the step's own figure, which
single activation decisions decide (train_oracle.ENVELOPE_GATES has the measurement).  tests/test_train_oracle_cpu.py shows that every planted
multi-step mistake leaves these gates, and that the reference's own run passes the teacher-forced ones."""
import os
import shutil

import numpy as np
import pytest
import torch

import kbnet_amd as kb
import pre_eval_cases as pec
import run_cases as rc
import train_cases as tc
import train_oracle as to

pytestmark = pytest.mark.gpu
STEPS = range(1, to.N_STEPS + 1)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    return np.load(to.GOLDEN)


@pytest.fixture(scope="module")
def device_run(dev, tmp_path_factory):
    """train() once: -> 'records' (one a step: the logged loss, the state of the step's two checkpoints, the probes of the restored
    models and the logged validation row), 'text' (results.txt), 'rows' (its validation rows)."""
    root = tmp_path_factory.mktemp("trajectory_inputs")

    def write_paths(filepath, paths):
        with open(filepath, "w") as f:
            f.write("\n".join(paths) + "\n")

    lists = [str(root / name) for name in rc.write_lists(str(root), write_paths)]
    depth = shutil.copy(rc.CHECKPOINT, str(root))
    pose = str(root / tc.POSE_CHECKPOINT)
    tc.write_pose_checkpoint(kb, pose)
    cfg = kb.kitti_config().narrow()
    out = str(tmp_path_factory.mktemp("trajectory") / "trained")
    torch.manual_seed(0)
    np.random.seed(0)
    results, logged, checkpoints = kb.training.train(
        lists[0], lists[1], lists[2], lists[0], lists[1], lists[2], lists[3], checkpoint_path=out, depth_model_restore_path=depth,
        pose_model_restore_path=pose, device="cuda", workers=2, return_results=True, **to.trajectory_settings(cfg))
    assert results["train_step"] == to.N_STEPS and [step for step, _ in logged] == list(STEPS)
    assert len(checkpoints) == 2 * to.N_STEPS
    with open(os.path.join(out, "results.txt")) as f:
        text = f.read()
    rows = to.validation_rows(text)
    assert [int(r[0]) for r in rows] == list(range(to.VALIDATION_START_STEP, to.N_STEPS + 1))

    b = {k: v.to(dev) for k, v in to.batch(torch.float32).items()}      # the frames in validation order
    truth, validity = to.ground_truths()
    depth_model = kb.modules.KBNetModel.from_config(cfg, device=dev)      # the default, fused model
    records = []
    for step, (_, loss) in zip(STEPS, logged):
        paths = [os.path.join(out, f"{which}_model-{step}.pth") for which in ("depth", "pose")]
        depth_ckpt, pose_ckpt = (torch.load(p, map_location="cpu") for p in paths)
        assert int(depth_ckpt["train_step"]) == int(pose_ckpt["train_step"]) == step
        state = to.state_from_checkpoints(depth_ckpt, pose_ckpt, torch.float64, step=step)
        got_step, _ = depth_model.restore_model(paths[0])
        assert got_step == step
        pose_model = kb.modules.load_pose_model(paths[1], device=dev, activation_func="relu")      # not trainable: running statistics
        with torch.no_grad():
            output = depth_model.forward(b["image0"], b["sparse"], b["filtered_validity"], b["intrinsics"])
            dofs = [pose_model.forward(b["image0"], b[other], return_all=True)[1] for other in ("image1", "image2")]
        output = output.double().cpu()
        logged_row = [r[1:] for r in rows if int(r[0]) == step]
        metrics = logged_row[0] if logged_row else pec.eval_oracle(output.float().numpy(), truth, validity, 0.0, 100.0)[0].mean(axis=0)
        records.append({"step": step, "loss": float(loss), "state": state,
                        "probes": {"depth": output, "dof01": dofs[0].double().cpu(), "dof02": dofs[1].double().cpu(),
                                   "metrics": np.asarray(metrics, dtype=np.float64)}})
    return {"records": records, "text": text, "rows": rows}


@pytest.fixture(scope="module")
def run64():
    """The fp64 oracle's free run of the eight steps, at test time."""
    return to.run(torch.float64)


@pytest.fixture(scope="module")
def gates(golden, run64):
    floors = np.stack([to.metric_floor(r["probes"]["depth"]) / r["probes"]["metrics"] for r in run64])
    return to.gate_table(golden, metric_floors=floors)


@pytest.fixture(scope="module")
def forced(device_run):
    """(distances, exact findings) a step: one fp64 oracle step from the device's own state of the step before."""
    return to.forced_against(device_run["records"])


def _line(step, distances, bounds, names):
    parts = []
    for name in names:
        bound = bounds[name][step - 1]
        parts.append(f"{name} {distances[name]:.2e}" + ("" if bound is None else f"/{bound:.2e}={distances[name] / bound:.2f}"))
    return f"step {step}: " + "  ".join(parts)


# ------------------------------------------------------------------------------------------------ teacher-forced
@pytest.mark.parametrize("step", STEPS)
def test_teacher_forced_step(forced, gates, step):
    """One fp64 oracle step from the device's checkpoint of step - 1 against the device's checkpoint of `step`: the loss, the update
    ||.||_2 ratios of the depth parameters, the pose parameters and the running statistics, Adam's m and v of both networks
    (adam_oracle.fraction) -- and exactly: every step count, num_batches_tracked, which parameters have moments, the rates in the
    checkpoint."""
    measured, findings = forced
    distances, table = measured[step - 1], gates["forced"]
    print(_line(step, distances, table, to.FORCED_GATES))
    assert not findings[step - 1], findings[step - 1]
    failed = {name: (distances[name], table[name][step - 1]) for name in to.FORCED_GATES if not distances[name] <= table[name][step - 1]}
    assert not failed, failed


def test_counts_exactly(device_run):
    """num_batches_tracked == 1000 + 2 t in every BatchNorm layer (two pose forwards a step), Adam's step count == t for every
    parameter the forward uses and no state for the others, the scheduled rate in every checkpoint."""
    for record in device_run["records"]:
        state, t = record["state"], record["step"]
        counts = {int(v) for k, v in state["running"].items() if k.endswith("num_batches_tracked")}
        assert counts == {1000 + 2 * t}, (t, counts)
        assert set(state["count"].values()) == {0, t}, (t, set(state["count"].values()))
        assert sorted(k for k, c in state["count"].items() if c) == sorted(state["m"]) == sorted(state["v"])
        assert state["lr"] == [to.learning_rate(t)] * 2, (t, state["lr"])


# ------------------------------------------------------------------------------------------------ the free run
def test_free_run(device_run, run64, gates, golden):
    """The device's run against the fp64 oracle's free run: the eight losses within 3 x the running maximum of the fp32 envelope,
    the depth update ratio at steps 4 and 8, the running statistics, the restored networks as functions at every step, and the
    validation rows of results.txt from step 2 on (printed beside the reference's recorded rows)."""
    origin = to.initial_state(torch.float64)
    measured = [to.distances(got, want, origin) for got, want in zip(device_run["records"], run64)]
    table = gates["free"]
    for step in STEPS:
        print(_line(step, measured[step - 1], table, to.FREE_GATES))
    print("pose update ratio (not gated: 0.16 to 0.28 in fp32 alone, DESIGN section 8q): " + "  ".join(f"{d['pose']:.3f}" for d in measured))
    reference = {int(r[0]): r[1:] for r in golden["reference_validation"]}
    for row in device_run["rows"]:
        step = int(row[0])
        print(f"step {step}: validation row  device " + " ".join(f"{v:10.3f}" for v in row[1:]) + "   fp64 oracle "
              + " ".join(f"{v:10.3f}" for v in run64[step - 1]["probes"]["metrics"]) + "   reference "
              + " ".join(f"{v:10.3f}" for v in reference[step]))
    failed = {}
    for name, per_step in to.ratios(measured, table).items():
        step, worst = to.first_failure(per_step)
        if step is not None:
            failed[name] = (step, worst)
    print("worst ratio per gate: " + "  ".join(f"{name} {to.first_failure(v)[1]:.2f}" for name, v in to.ratios(measured, table).items()))
    assert not failed, failed


def test_worst_ratios_of_the_teacher_forced_gates(forced, gates):
    """The log's summary line: the worst ratio of every teacher-forced gate over the eight steps (asserted per step above)."""
    measured, _ = forced
    per_gate = to.ratios(measured, gates["forced"])
    print("worst ratio per gate: " + "  ".join(f"{name} {to.first_failure(v)[1]:.2f}" for name, v in per_gate.items()))
    assert all(np.isfinite(to.first_failure(v)[1]) for v in per_gate.values())
