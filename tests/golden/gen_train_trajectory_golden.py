#!/usr/bin/env python
"""Generate tests/golden/train_trajectory_kitti_narrow.npz: eight steps of THE REFERENCE's train() (src/kbnet.py:31-518) on the CPU,
measured against tests/train_oracle.py in fp64, and the oracle's own fp32 runs measured the same way.

    python tests/golden/gen_train_trajectory_golden.py <the reference's src directory>

The manner of gen_train_golden.py: the reference's `src` is imported only when this runs, nothing of its source is stored, the
fixture is data -- and a few kilobytes: no tensor of either network goes into it.  The run is train_cases.train_settings with
train_oracle.trajectory_settings' changes: eight epochs of one step, learning_schedule [3, 8] with the rates [1e-4, 5e-5] (the
change lands at step 4, away from Adam's special first step), validation from step 2 on, a checkpoint every step.  Recorded:

  from the reference
    reference_losses        the loss of every step as compute_loss returned it, float64 of the float32
    reference_validation    the 'Validation results' rows of results.txt as numbers: step, MAE, RMSE, iMAE, iRMSE
    reference_update        ||p_ref,8 - p_64,8|| / ||p_64,8 - p_0|| over the depth parameters, over the pose parameters and over the
                            pose running statistics, p_64 the fp64 oracle's (frame order (0, 1, 2)): three numbers
    reference_counts        num_batches_tracked of the first BatchNorm layer and Adam's largest step count at step 8
    reference_forced        steps x train_oracle.FORCED_GATES: ONE fp64 oracle step from the reference's own checkpoint of step t - 1
                            against its checkpoint of step t -- the reference measured as the device is
  from the oracle in fp32, for each of the twelve runs of train_oracle.fixture_runs() (the six frame orders with the images
  contiguous, then with the images channels-last: another summation order of the same values) and every step, against the fp64
  oracle in the same frame order
    free                    runs x steps x distances (train_oracle.DISTANCES): the free-running fp32 run
    forced                  the same for ONE fp32 step from the fp64 state of the step before (teacher-forced)
    forced_own              runs x steps x train_oracle.FORCED_GATES: the free-running fp32 run's step against ONE fp64 step from
                            its own state of the step before -- the fp32 oracle measured as the device is
    orders, distances, forced_names   the frame orders and the names of the last axes

Nothing derived from the device goes into the file: these are the yardsticks of tests/test_train_trajectory_gpu.py."""
import os
import shutil
import sys
import tempfile
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import kbnet_amd as kb  # noqa: E402
import run_cases as rc  # noqa: E402
import train_cases as tc  # noqa: E402
import train_oracle as to  # noqa: E402

def run_reference(reference_src):
    """-> (losses, the text of results.txt, the state of every step as train_oracle.state_from_checkpoints reads its two checkpoints,
    in fp64)."""
    sys.path.insert(0, reference_src)
    torchvision = types.ModuleType("torchvision")
    torchvision.utils = types.ModuleType("torchvision.utils")
    torchvision.utils.make_grid = lambda tensor, nrow=8: tensor[0]
    sys.modules.setdefault("torchvision", torchvision)
    sys.modules.setdefault("torchvision.utils", torchvision.utils)
    tensorboard = types.ModuleType("torch.utils.tensorboard")
    tensorboard.SummaryWriter = tc.RecordingWriter
    sys.modules["torch.utils.tensorboard"] = tensorboard
    if not hasattr(np, "infty"):      # the reference was written against NumPy 1
        np.infty = np.inf
    import data_utils, kbnet, kbnet_model  # noqa: E401,E402  (reference)

    torch.manual_seed(0)
    np.random.seed(0)
    settings = to.trajectory_settings(kb.kitti_config().narrow())
    losses = []
    compute_loss = kbnet_model.KBNetModel.compute_loss

    def recorded(self, *args, **kwargs):
        loss, info = compute_loss(self, *args, **kwargs)
        losses.append(float(loss.detach().double()))
        return loss, info

    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            lists = rc.write_lists(tmp, data_utils.write_paths)
            shutil.copy(rc.CHECKPOINT, tmp)
            tc.write_pose_checkpoint(kb, tc.POSE_CHECKPOINT)
            kbnet_model.KBNetModel.compute_loss = recorded
            try:
                kbnet.train(lists[0], lists[1], lists[2], lists[0], lists[1], lists[2], lists[3], checkpoint_path="trained",
                            depth_model_restore_path=os.path.basename(rc.CHECKPOINT), pose_model_restore_path=tc.POSE_CHECKPOINT,
                            device="cpu", **settings)
            finally:
                kbnet_model.KBNetModel.compute_loss = compute_loss
            with open(os.path.join("trained", "results.txt")) as f:
                text = f.read()
            states = []
            for step in range(1, to.N_STEPS + 1):
                depth, pose = (torch.load(os.path.join("trained", f"{which}_model-{step}.pth"), map_location="cpu", weights_only=False)
                               for which in ("depth", "pose"))
                states.append(to.state_from_checkpoints(depth, pose, torch.float64, step=step))
        finally:
            os.chdir(cwd)
    assert len(losses) == to.N_STEPS, losses
    return np.asarray(losses, dtype=np.float64), text, states


def main(reference_src):
    torch.set_num_threads(to.THREADS)      # the reference's run under the condition of the six fp32 oracle runs (free_and_forced)
    out = {}
    losses, text, states = run_reference(reference_src)
    reference = states[-1]
    out["reference_losses"] = losses
    # teacher-forced: one fp64 oracle step from the reference's own checkpoint of step t - 1 against its checkpoint of step t
    records = [{"loss": float(loss), "state": state} for loss, state in zip(losses, states)]
    measured, findings = to.forced_against(records)
    assert not any(findings), findings      # step counts, num_batches_tracked and the rates of every checkpoint are the oracle's
    out["reference_forced"] = np.asarray([[d[name] for name in to.FORCED_GATES] for d in measured])
    out["reference_validation"] = to.validation_rows(text)
    assert out["reference_validation"].shape == (to.N_STEPS - to.VALIDATION_START_STEP + 1, 5), out["reference_validation"]
    origin = to.initial_state(torch.float64)
    last = None
    for last in to.iterate(torch.float64, with_probes=False):
        pass
    want = last["state"]
    findings = to.exact_findings(reference, want)
    assert not findings, findings      # the reference's step counts and num_batches_tracked are the oracle's
    out["reference_update"] = np.asarray([to.update_ratio(reference["depth"], want["depth"], origin["depth"]),
                                          to.update_ratio(reference["pose"], want["pose"], origin["pose"]),
                                          to.update_ratio(to._floating(reference["running"]), to._floating(want["running"]),
                                                          to._floating(origin["running"]))])
    out["reference_counts"] = np.asarray([int(reference["running"]["enc::conv1.batch_norm.num_batches_tracked"]),
                                          max(reference["count"].values())], dtype=np.int64)
    free, forced, own = [], [], []
    for layout, order in to.fixture_runs():
        a, b, c = to.free_and_forced(order, layout=layout)
        free.append([[d[name] for name in to.DISTANCES] for d in a])
        forced.append([[d[name] for name in to.DISTANCES] for d in b])
        own.append([[d[name] for name in to.FORCED_GATES] for d in c])
        print(layout, order, "done")
    out["free"], out["forced"], out["forced_own"] = np.asarray(free), np.asarray(forced), np.asarray(own)
    out["forced_names"] = np.array(to.FORCED_GATES)
    out["orders"] = np.asarray(to.ORDERS, dtype=np.int64)
    out["distances"] = np.array(to.DISTANCES)
    np.set_printoptions(precision=3, linewidth=200)
    print("reference losses:", losses)
    print("reference validation rows:\n", out["reference_validation"])
    print("reference update distances (depth, pose, running):", out["reference_update"])
    print("reference, teacher-forced (steps x", list(to.FORCED_GATES), "):\n", out["reference_forced"])
    print("free, worst of the runs (steps x", list(to.DISTANCES), "):\n", out["free"].max(axis=0))
    print("forced, worst of the runs:\n", out["forced"].max(axis=0))
    print("forced from the fp32 run's own states, worst of the orders (steps x", list(to.FORCED_GATES), "):\n", out["forced_own"].max(axis=0))
    np.savez_compressed(to.GOLDEN, **out)
    print(to.GOLDEN, os.path.getsize(to.GOLDEN), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
