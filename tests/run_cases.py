"""What tests/golden/gen_run_golden.py and the tests of kb.inference.run share: the run's inputs, the fixed argument sets of the six
log_*_settings functions, the planted values of the export conversions and their NumPy oracle (and its near-misses)."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_DIR = os.path.join(HERE, "golden")
IO = os.path.join(GOLDEN_DIR, "io")
GOLDEN = os.path.join(GOLDEN_DIR, "run_kitti_narrow.npz")
CHECKPOINT = os.path.join(GOLDEN_DIR, "ckpt_kitti_narrow.pth")
N_FRAMES = 3
DIRECTORIES = ("image", "output_depth", "sparse_depth", "ground_truth")


def path_lists():
    """(image, sparse depth, intrinsics, ground truth) paths: the three 24 x 40 frames of golden/io; frame i is scored against
    depth_{(i + 1) % 3}.png."""
    frames = range(N_FRAMES)
    return ([os.path.join(IO, f"triplet_{i}.png") for i in frames], [os.path.join(IO, f"depth_{i}.png") for i in frames],
            [os.path.join(IO, f"k_{i}.npy") for i in frames], [os.path.join(IO, f"depth_{(i + 1) % N_FRAMES}.png") for i in frames])


def write_lists(directory, write_paths):
    """Writes the four lists into `directory` with `write_paths(filepath, paths)`; -> their file names (relative: the log holds them)."""
    names = ("image.txt", "sparse_depth.txt", "intrinsics.txt", "ground_truth.txt")
    for name, paths in zip(names, path_lists()):
        write_paths(os.path.join(directory, name), paths)
    return names


def run_settings(cfg):
    """run()'s model and evaluation arguments for a KBNetConfig (the narrow KITTI one), as lists like run_kbnet.py's argparse."""
    return dict(
        input_channels_image=cfg.input_channels_image, input_channels_depth=cfg.input_channels_depth, normalized_image_range=[0, 1],
        outlier_removal_kernel_size=7, outlier_removal_threshold=1.5,
        min_pool_sizes_sparse_to_dense_pool=list(cfg.min_pool_sizes_sparse_to_dense_pool),
        max_pool_sizes_sparse_to_dense_pool=list(cfg.max_pool_sizes_sparse_to_dense_pool),
        n_convolution_sparse_to_dense_pool=cfg.n_convolution_sparse_to_dense_pool, n_filter_sparse_to_dense_pool=cfg.n_filter_sparse_to_dense_pool,
        n_filters_encoder_image=list(cfg.n_filters_encoder_image), n_filters_encoder_depth=list(cfg.n_filters_encoder_depth),
        resolutions_backprojection=list(cfg.resolutions_backprojection), n_filters_decoder=list(cfg.n_filters_decoder),
        deconv_type=cfg.deconv_type, min_predict_depth=cfg.min_predict_depth, max_predict_depth=cfg.max_predict_depth,
        weight_initializer=cfg.weight_initializer, activation_func=cfg.activation_func, min_evaluate_depth=0.0, max_evaluate_depth=100.0)


class _Parameter:
    def __init__(self, count):
        self.count = count

    def numel(self):
        return self.count


class _Device:
    def __init__(self, kind):
        self.type = kind


def log_cases():
    """name -> (function name, keyword arguments): one fixed set each, the training and the inference form of log_input_settings and
    log_system_settings both."""
    network = dict(
        min_pool_sizes_sparse_to_dense_pool=[5, 7, 9, 11, 13], max_pool_sizes_sparse_to_dense_pool=[15, 17], n_convolution_sparse_to_dense_pool=3,
        n_filter_sparse_to_dense_pool=8, n_filters_encoder_image=[48, 96, 192, 384, 384], n_filters_encoder_depth=[16, 32, 64, 128, 128],
        resolutions_backprojection=[0, 1, 2, 3], n_filters_decoder=[256, 128, 128, 64, 12], deconv_type="up", min_predict_depth=1.5,
        max_predict_depth=100.0, weight_initializer="xavier_normal", activation_func="leaky_relu")
    return {
        "input_train": ("log_input_settings", dict(n_batch=8, n_height=320, n_width=768, input_channels_image=3, input_channels_depth=2,
                                                   normalized_image_range=[0, 1], outlier_removal_kernel_size=7, outlier_removal_threshold=1.5)),
        "input_train_partial": ("log_input_settings", dict(n_batch=4, n_width=96, normalized_image_range=[-1, 1], outlier_removal_threshold=2.0)),
        "input_run": ("log_input_settings", dict(input_channels_image=3, input_channels_depth=2, normalized_image_range=[0, 255],
                                                 outlier_removal_kernel_size=5, outlier_removal_threshold=1.25)),
        "network_both": ("log_network_settings", dict(network, parameters_depth_model=[_Parameter(1200), _Parameter(34)],
                                                      parameters_pose_model=[_Parameter(567)])),
        "network_depth": ("log_network_settings", dict(network, deconv_type="transpose", parameters_depth_model=[_Parameter(6957172)])),
        "training": ("log_training_settings", dict(
            n_batch=8, n_train_sample=1003, n_train_step=7500, learning_rates=[5e-5, 1e-4, 15e-5, 1e-4, 5e-5, 2e-5],
            learning_schedule=[2, 8, 20, 30, 45, 60], augmentation_probabilities=[1.00, 0.50, 0.25], augmentation_schedule=[50, 55, 60],
            augmentation_random_crop_type=["horizontal", "vertical", "anchored", "bottom"], augmentation_random_flip_type=["none"],
            augmentation_random_remove_points=[0.60, 0.70], augmentation_random_noise_type="none", augmentation_random_noise_spread=-1)),
        "loss": ("log_loss_func_settings", dict(w_color=0.15, w_structure=0.95, w_sparse_depth=0.60, w_smoothness=0.04,
                                                w_weight_decay_depth=0.0, w_weight_decay_pose=1e-4)),
        "evaluation": ("log_evaluation_settings", dict(min_evaluate_depth=0.0, max_evaluate_depth=100.0)),
        "system_train": ("log_system_settings", dict(
            checkpoint_path="trained_kbnet/model", n_checkpoint=5000, summary_event_path="trained_kbnet/model/events", n_summary=1000,
            n_summary_display=4, validation_start_step=200000, depth_model_restore_path="", pose_model_restore_path="pose.pth",
            device=_Device("cuda"), n_thread=8)),
        "system_train_partial": ("log_system_settings", dict(checkpoint_path="somewhere", n_summary_display=2, device=_Device("cpu"), n_thread=2)),
        "system_run": ("log_system_settings", dict(checkpoint_path="results", depth_model_restore_path="depth.pth", device=_Device("cuda"),
                                                   n_thread=1)),
    }


def logged_text(function, kwargs, directory, name):
    """What `function(log_path, **kwargs)` writes into a fresh file of `directory`."""
    log_path = os.path.join(directory, name + ".txt")
    function(log_path, **kwargs)
    with open(log_path) as f:
        return f.read()


# ------------------------------------------------------------------------------------ the export conversions
def planted_values():
    """The values every conversion test plants: the edges of both rules and what must not take a process down."""
    one_below = np.nextafter(np.float32(1.0), np.float32(0.0))
    special = [0.0, -0.0, 1.0, one_below, np.nan, np.inf, -np.inf, -3.0, 300.0, 255.99609375, 256.0, 1.0 / 256.0,
               np.nextafter(np.float32(1.0 / 256.0), np.float32(0.0))]
    return np.concatenate([np.asarray(special, dtype=np.float32), np.arange(256, dtype=np.float32) / np.float32(255.0)])


def oracle_rgb(image, scale, shift, rounding=False, planar=False):
    """N x 3 x H x W float32 -> N x H x W x 3 uint8: clamp(trunc(scale * v + shift), 0, 255), NaN -> 0, product and sum in float32.
    Near-misses for the proof of power: `rounding` rounds to nearest instead of truncating; `planar` keeps the channel planes
    (the bytes of an N x 3 x H x W array read as if interleaved)."""
    with np.errstate(invalid="ignore", over="ignore"):
        x = (np.float32(scale) * np.asarray(image, dtype=np.float32)).astype(np.float32) + np.float32(shift)
        x = np.where(np.isnan(x), np.float32(0.0), x)
        x = np.rint(x) if rounding else np.trunc(x)
        px = np.clip(x, 0.0, 255.0).astype(np.uint8)
    if planar:
        return np.ascontiguousarray(px).reshape(px.shape[0], px.shape[2], px.shape[3], 3)
    return np.ascontiguousarray(np.transpose(px, (0, 2, 3, 1)))


def oracle_samples(depth, factor=256.0, rounding=False):
    """N x 1 x H x W (or N x H x W) float32 -> N x H x W uint16: min(trunc(z * 256), 65535), NaN and negatives -> 0."""
    z = np.asarray(depth, dtype=np.float32)
    z = z.reshape((z.shape[0],) + z.shape[-2:])
    with np.errstate(invalid="ignore", over="ignore"):
        x = z * np.float32(factor)
        x = np.where(np.isnan(x), np.float32(0.0), x)
        x = np.rint(x) if rounding else np.trunc(x)
        return np.clip(x, 0.0, 65535.0).astype(np.uint16)


def make_sources(n, h, w, seed=0):
    """(image n x 3 x h x w, depth_a n x 1 x h x w, depth_b n x 1 x h x w) float32: seeded values with the planted ones written over the
    start of every tensor (as many as fit), the depths scaled so that samples cover the 16 bits and beyond."""
    rng = np.random.default_rng(seed)
    planted = planted_values()
    image = rng.uniform(-0.05, 1.05, size=(n, 3, h, w)).astype(np.float32)
    depth_a = rng.uniform(0.0, 300.0, size=(n, 1, h, w)).astype(np.float32)
    depth_b = (rng.uniform(0.0, 90.0, size=(n, 1, h, w)) * (rng.uniform(size=(n, 1, h, w)) < 0.3)).astype(np.float32)
    for t in (image, depth_a, depth_b):
        flat = t.reshape(-1)
        k = min(flat.size, planted.size)
        flat[:k] = planted[:k]
    return image, depth_a, depth_b
