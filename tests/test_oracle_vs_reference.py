"""CPU: oracle == the reference at the full KITTI / VOID sizes (bitwise), including the intrinsics-scaling quirk.

A full-size depth map is larger than a committed fixture may be, so `tests/golden/fwd_full_size.npz` (written by
`tests/golden/gen_golden.py --only-full-size`, which runs the reference) holds the SHA-256 of the reference's output bits,
a seeded sample of its values and the SHA-256 of the synthetic inputs and weights it was fed."""
import hashlib

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import kbnet_oracle as orc
import kbnet_amd as kb


def _key(preset, shape, options):   # gen_golden.full_size_key
    return "_".join([preset, "%dx%d" % shape] + [str(options[k]) for k in sorted(options)])


def _sha256(tensors):   # gen_golden.sha256_of
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("preset,shape,options", [("kitti", (352, 1216), {}), ("void", (480, 640), {}),
                                                  # run_kbnet.py --deconv_type transpose / --activation_func elu | sigmoid
                                                  ("kitti", (352, 1216), {"deconv_type": "transpose", "activation_func": "elu"}),
                                                  ("void", (480, 640), {"activation_func": "sigmoid"})])
def test_full_size_bitwise(preset, shape, options):
    import dataclasses
    cfg = dataclasses.replace(kb.PRESETS[preset](), **options)
    ref = load_golden("fwd_full_size")[_key(preset, shape, options)]
    sds = kb.synthetic.make_state_dicts(cfg, seed=0, gain=kb.synthetic.PARITY_GAIN[preset] if options else 1.0)
    image, sparse, valid, k = kb.synthetic.make_frames(1, *shape, preset, seed=1)
    assert _sha256([image, sparse, valid, k] + [sd[n] for sd in sds for n in sorted(sd)]) == str(ref["inputs_sha256"]), \
        "synthetic inputs / weights differ from the ones the fixture was recorded with: regenerate it"
    out = orc.kbnet_forward(image, sparse, valid, k, *sds, cfg.min_pools, cfg.max_pools,
                            cfg.min_predict_depth, cfg.max_predict_depth, slope=orc.activation_slope(cfg.activation_func))
    assert tuple(out.shape) == tuple(ref["shape"])
    assert torch.equal(out.reshape(-1)[torch.from_numpy(ref["sample_index"])], ref["sample"])
    assert _sha256([out]) == str(ref["output_sha256"])
    assert float(out.std()) > 0
