#!/usr/bin/env python
"""Generate tests/golden/train_kitti_narrow.npz by RUNNING THE REFERENCE's train() (src/kbnet.py:31-518) on the CPU.

    python tests/golden/gen_train_golden.py <the reference's src directory>

Nothing of the reference's source is stored: the fixture is data.  `torchvision` is stubbed in sys.modules (its make_grid returns
the first tile: only the calls are recorded, not the pictures) and torch.utils.tensorboard.SummaryWriter is replaced by
train_cases.RecordingWriter, which keeps (method, tag, step).  Inputs (tests/train_cases.py, tests/run_cases.py): the three
24 x 40 frames of golden/io as ONE batch an epoch (the shuffle only permutes frames inside a mean), no crop, augmentation
probability 0, the narrow KITTI configuration, learning_schedule [1, 3] with two rates, a summary and a checkpoint every step,
validation from step 2 on against run_cases.path_lists()' ground truths, n_thread 0 (no worker processes), device 'cpu'.  The depth
model restores ckpt_kitti_narrow.pth, the pose model a checkpoint written here from kb.synthetic's seeded weights
(train_cases.write_pose_checkpoint).  The run works inside a temporary directory with RELATIVE paths, so the logged text does not
depend on where it ran.  Recorded:
  results            the text of checkpoint_path/results.txt
  calls_train, calls_val   the writers' (method, tag, step) lists, as arrays of strings
  losses             the loss of every step as compute_loss returned it (wrapped), float64 of the float32
  checkpoints        the sorted names of the checkpoint files
  checkpoint_steps, checkpoint_lrs   each file's train_step and its param_groups' learning rates
  parameters, defaults   the names of train()'s parameters in order, and repr() of each default"""
import inspect
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


def main(reference_src):
    sys.path.insert(0, reference_src)
    torchvision = types.ModuleType("torchvision")
    torchvision.utils = types.ModuleType("torchvision.utils")
    torchvision.utils.make_grid = lambda tensor, nrow=8: tensor[0]
    sys.modules.setdefault("torchvision", torchvision)
    sys.modules.setdefault("torchvision.utils", torchvision.utils)
    writers = []

    def writer(log_dir):
        writers.append(tc.RecordingWriter(log_dir))
        return writers[-1]

    tensorboard = types.ModuleType("torch.utils.tensorboard")
    tensorboard.SummaryWriter = writer
    sys.modules["torch.utils.tensorboard"] = tensorboard
    if not hasattr(np, "infty"):      # the reference was written against NumPy 1
        np.infty = np.inf
    import data_utils, kbnet, kbnet_model  # noqa: E401,E402  (reference)

    torch.manual_seed(0)
    np.random.seed(0)
    cfg = kb.kitti_config().narrow()
    settings = tc.train_settings(cfg)
    out = {}
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
                out["results"] = np.array(f.read())
            names = sorted(n for n in os.listdir("trained") if n.endswith(".pth"))
            steps, lrs = [], []
            for name in names:
                ckpt = torch.load(os.path.join("trained", name), map_location="cpu", weights_only=False)
                steps.append(int(ckpt["train_step"]))
                lrs.append([float(g["lr"]) for g in ckpt["optimizer_state_dict"]["param_groups"]])
            out["checkpoints"] = np.array(names)
            out["checkpoint_steps"] = np.asarray(steps, dtype=np.int64)
            out["checkpoint_lrs"] = np.asarray(lrs, dtype=np.float64)
        finally:
            os.chdir(cwd)

    assert len(writers) == 2 and writers[0].log_dir.endswith("events-train") and writers[1].log_dir.endswith("events-val")
    out["calls_train"] = np.array([[m, t, str(s)] for m, t, s in writers[0].calls])
    out["calls_val"] = np.array([[m, t, str(s)] for m, t, s in writers[1].calls])
    assert len(losses) == tc.N_EPOCH
    out["losses"] = np.asarray(losses, dtype=np.float64)
    parameters = inspect.signature(kbnet.train).parameters
    out["parameters"] = np.array(list(parameters))
    out["defaults"] = np.array([repr(p.default) if p.default is not inspect.Parameter.empty else "<required>" for p in parameters.values()])
    print("losses:", losses)
    print("train calls:", len(writers[0].calls), " val calls:", len(writers[1].calls), " checkpoints:", list(out["checkpoints"]))
    print(str(out["results"]))
    np.savez_compressed(tc.GOLDEN, **out)
    print(tc.GOLDEN, os.path.getsize(tc.GOLDEN), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
