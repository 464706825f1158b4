"""What tests/golden/gen_train_golden.py and the tests of kb.training.train share: the run's settings, the pose checkpoint both sides
restore (kb.synthetic's seeded CPU weights -- a ResNet-18 checkpoint would not fit the size limit of a committed file), and the
recording stub of a summary writer."""
import os

import torch

import run_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(rc.GOLDEN_DIR, "train_kitti_narrow.npz")
POSE_SEED = 11
POSE_CHECKPOINT = "pose_init.pth"
N_BATCH, N_HEIGHT, N_WIDTH = 3, 24, 40      # the three 24 x 40 frames of golden/io: one batch an epoch
N_EPOCH = 3
WRITER_METHODS = ("add_scalar", "add_histogram", "add_image")


def train_settings(cfg):
    """train()'s keyword arguments for a KBNetConfig (the narrow KITTI one): three epochs of one step, two learning rates, no crop,
    no augmentation, a summary and a checkpoint every step, validation from step 2 on."""
    settings = rc.run_settings(cfg)
    settings.update(
        n_batch=N_BATCH, n_height=N_HEIGHT, n_width=N_WIDTH, learning_rates=[1e-4, 5e-5], learning_schedule=[1, N_EPOCH],
        augmentation_probabilities=[0.0], augmentation_schedule=[-1], augmentation_random_crop_type=["none"],
        augmentation_random_flip_type=["none"], augmentation_random_remove_points=[0.60, 0.70], augmentation_random_noise_type="none",
        augmentation_random_noise_spread=-1, w_color=0.15, w_structure=0.95, w_sparse_depth=0.60, w_smoothness=0.04,
        w_weight_decay_depth=0.0, w_weight_decay_pose=1e-4, n_checkpoint=1, n_summary=1, n_summary_display=4, validation_start_step=2,
        n_thread=0)
    return settings


def write_pose_checkpoint(kb, path):
    """A checkpoint of the reference's PoseNetModel('resnet18') layout (DataParallel's `module.` prefix) from
    kb.synthetic.make_resnet_pose_weights(18, seed=POSE_SEED): CPU tensors, the same bits wherever it is built."""
    enc, dec = kb.synthetic.make_resnet_pose_weights(18, seed=POSE_SEED)
    torch.save({"train_step": 0, "optimizer_state_dict": {},
                "encoder_state_dict": {"module." + k: v for k, v in enc.items()},
                "decoder_state_dict": {"module." + k: v for k, v in dec.items()}}, path)


class RecordingWriter:
    """A summary writer that keeps (method, tag, step) of every call, and with keep=True the tensors handed to it (cloned)."""

    def __init__(self, log_dir, keep=False):
        self.log_dir, self.keep = log_dir, keep
        self.calls, self.tensors, self.closed = [], [], 0

    def _record(self, method, tag, value, global_step):
        self.calls.append((method, tag, int(global_step)))
        if self.keep:
            self.tensors.append(value.detach().clone() if torch.is_tensor(value) else value)

    def add_scalar(self, tag, scalar_value, global_step=None, **_):
        self._record("add_scalar", tag, scalar_value, global_step)

    def add_histogram(self, tag, values, global_step=None, **_):
        self._record("add_histogram", tag, values, global_step)

    def add_image(self, tag, img_tensor, global_step=None, **_):
        self._record("add_image", tag, img_tensor, global_step)

    def flush(self):
        pass

    def close(self):
        self.closed += 1
