"""The training step's augmentation: the reference's Transforms (src/transforms.py) over ops.augment (csrc/augment.hip), and the
lines of the training loop in front of it (src/kbnet.py:403-422) as one call.

    transforms = kb.transforms.Transforms(normalized_image_range=[0, 1], random_flip_type=['none'],
                                          random_remove_points=[0.60, 0.70], random_noise_type='none', random_noise_spread=-1)
    [image0, image1, image2], [sparse_depth0], [filtered_sparse_depth0, filtered_validity_map_depth0] = transforms.transform(
        images_arr=[image0, image1, image2], range_maps_arr=[sparse_depth0],
        validity_maps_arr=[filtered_sparse_depth0, filtered_validity_map_depth0], random_transform_probability=p)

The per-frame decisions are drawn on the host with np.random.rand in the reference's order (`draw`), so the same np.random.seed
makes the reference's decisions; the removal densities are `(max - min) * torch.rand(n, device=device) + min` as in the reference
and stay on the device; which points go and what noise they get comes from Philox4x32-10 keyed by this object's seed and its count
of transform() calls.  Differences from the reference, on purpose: the inputs are never written (the reference flips its arguments
in place, which with range [0, 255] changes the caller's images); CPU tensors raise; 5-D inputs raise ValueError.

Data-parallel training (`shard=(first, n_global)`): the tensors are frames [first, first + n_local) of a global batch of n_global.
Every rank draws the decisions and the densities of the WHOLE batch -- so np.random and torch's generators advance exactly as in
one process, on every rank alike -- keeps its slice, and launches with frame_base=first, so that the Philox draws are those of
the frames' places in the global batch.  Ranks that start from one np.random / torch state and one `seed` thus produce, bit for
bit, the shard_bounds slices of what one process produces."""

from __future__ import annotations

from typing import List, Optional

import numpy as np
import torch

from . import ops


class Transforms(object):

    def __init__(self,
                 normalized_image_range=[0, 255],
                 random_flip_type=['none'],
                 random_remove_points=[0.70, 0.70],
                 random_noise_type=['none'],
                 random_noise_spread=-1,
                 seed: Optional[int] = None):
        """The reference's arguments (src/transforms.py:23-59), and `seed`: the 64-bit key of the removal and noise draws;
        None takes torch.initial_seed(), so that torch.manual_seed before the construction fixes it."""
        self.normalized_image_range = normalized_image_range
        self.do_random_horizontal_flip = 'horizontal' in random_flip_type
        self.do_random_vertical_flip = 'vertical' in random_flip_type
        self.do_random_remove_points = -1 not in random_remove_points
        self.remove_points_range = random_remove_points
        self.do_random_noise = random_noise_type != 'none' and random_noise_spread > 0
        self.random_noise_type = random_noise_type
        self.random_noise_spread = random_noise_spread
        self.seed = int(torch.initial_seed() if seed is None else seed) & 0xFFFFFFFFFFFFFFFF
        self.calls = 0      # transform() calls so far: a word of every draw's counter

    def state_dict(self) -> dict:
        """What the removal and noise draws of the next transform() depend on beyond np.random and torch's generators: the key and
        the count of calls."""
        return {"seed": int(self.seed), "calls": int(self.calls)}

    def load_state_dict(self, state: dict) -> None:
        seed, calls = int(state["seed"]), int(state["calls"])
        if not 0 <= seed <= 0xFFFFFFFFFFFFFFFF or calls < 0:
            raise ValueError('Transforms state: seed {} calls {}'.format(seed, calls))
        self.seed, self.calls = seed, calls

    def draw(self, n_batch: int, random_transform_probability: float = 0.50) -> List[int]:
        """The host part of transform(): one flags value a frame (ops.AUGMENT_* bits), from np.random.rand(n_batch) drawn in the
        reference's order -- the transform decision, then one more draw for each enabled branch: horizontal flip, vertical flip,
        remove points, noise -- each `<= 0.5` and ANDed with the first.  A rank of a data-parallel run calls it with the GLOBAL
        batch's n_batch and slices the result (transform(shard=...))."""
        do_random_transform = np.random.rand(n_batch) <= random_transform_probability
        flags = np.zeros(n_batch, dtype=np.int64)
        for enabled, bit in ((self.do_random_horizontal_flip, ops.AUGMENT_FLIP_HORIZONTAL), (self.do_random_vertical_flip, ops.AUGMENT_FLIP_VERTICAL),
                             (self.do_random_remove_points, ops.AUGMENT_REMOVE), (self.do_random_noise, ops.AUGMENT_NOISE)):
            if enabled:
                flags |= bit * np.logical_and(do_random_transform, np.random.rand(n_batch) <= 0.50)
        return [int(f) for f in flags]

    def transform(self,
                  images_arr,
                  range_maps_arr=[],
                  validity_maps_arr=[],
                  random_transform_probability=0.50,
                  shard=None):
        """The reference's transform (src/transforms.py:61-183): lists of N x C x H x W fp32 device tensors in, the lists that are
        not empty out (the one list itself when only one is).

        shard: None, or (first, n_global) -- the tensors are frames [first, first + N) of a global batch of n_global frames (see
        the module's docstring).  A rank with N == 0 still draws and still counts the call; it launches nothing."""
        first = images_arr[0] if len(images_arr) else next(iter(list(range_maps_arr) + list(validity_maps_arr)), None)
        if not isinstance(first, torch.Tensor) or first.dim() != 4:
            raise ValueError('Unsupported number of dimensions: {}'.format(first.dim() if isinstance(first, torch.Tensor) else None))
        n_local = first.shape[0]
        if shard is None:
            frame_base, n_batch = 0, n_local
        else:
            frame_base, n_batch = (int(v) for v in shard)
            if frame_base < 0 or frame_base + n_local > n_batch:
                raise ValueError('shard {}: frames [{}, {}) do not lie in a batch of {}'.format(tuple(shard), frame_base, frame_base + n_local, n_batch))
        flags = self.draw(n_batch, random_transform_probability)[frame_base:frame_base + n_local]
        densities = None
        if self.do_random_remove_points:    # drawn whether or not a frame is flagged, as the reference does: torch's stream stays in step
            remove_points_min, remove_points_max = self.remove_points_range
            densities = (remove_points_max - remove_points_min) * torch.rand(n_batch, device=first.device) + remove_points_min
            if shard is not None:
                densities = densities[frame_base:frame_base + n_local].contiguous()
        call = self.calls
        self.calls += 1
        outputs = ops.augment(images_arr, range_maps_arr, validity_maps_arr, flags, densities,
                              normalized_image_range=self.normalized_image_range, noise_type=self.random_noise_type,
                              noise_spread=self.random_noise_spread, seed=self.seed, call=call, frame_base=frame_base)
        outputs = [o for o in outputs if len(o) > 0]
        return outputs[0] if len(outputs) == 1 else outputs


def train_inputs(transforms: Transforms, image0, image1, image2, sparse_depth0, random_transform_probability,
                 kernel_size: int = 7, threshold: float = 1.5, shard=None):
    """Reference src/kbnet.py:403-422 in one call: the validity map of the sparse depth, OutlierRemoval.remove_outliers
    (ops.preprocess), then transforms.transform over (images, [sparse_depth0], [filtered_sparse_depth0, filtered_validity_map_depth0]).
    Returns (image0, image1, image2, sparse_depth0, filtered_sparse_depth0, filtered_validity_map_depth0).  `shard`: as
    Transforms.transform's; a rank without frames gets six tensors of zero frames, and its Transforms still draws."""
    if sparse_depth0.shape[0] == 0:      # this rank's shard of the batch is empty: nothing to filter, the draws still happen
        filtered_validity_map_depth0, filtered_sparse_depth0 = torch.empty_like(sparse_depth0), torch.empty_like(sparse_depth0)
    else:
        _, filtered_validity_map_depth0, filtered_sparse_depth0 = ops.preprocess(None, sparse_depth0, kernel_size=kernel_size, threshold=threshold)
    [image0, image1, image2], [sparse_depth0], [filtered_sparse_depth0, filtered_validity_map_depth0] = transforms.transform(
        images_arr=[image0, image1, image2],
        range_maps_arr=[sparse_depth0],
        validity_maps_arr=[filtered_sparse_depth0, filtered_validity_map_depth0],
        random_transform_probability=random_transform_probability, shard=shard)
    return image0, image1, image2, sparse_depth0, filtered_sparse_depth0, filtered_validity_map_depth0
