#!/usr/bin/env python3
"""Generate the golden vectors of the depth network's BACKWARD pass by RUNNING THE REFERENCE on CPU under torch.autograd.

Needs a checkout of the reference (read-only); give the path of its `src` directory:

    python tests/golden/gen_kbnet_grad_golden.py <reference>/src

It imports the reference's `networks`, builds SparseToDensePool, KBNetEncoder and MultiScaleDecoder with the arguments its KBNetModel
passes (src/kbnet_model.py:86-137), loads synthetic.make_state_dicts into them, casts them and the inputs to fp64, runs
KBNetModel.forward's lines (:163-184) and differentiates L = sum(depth * cotangent) for a seeded N x 1 x H x W cotangent.  Written next
to this script as `kbnet_grad_*.npz` and `kbnet_grad_*_enc.npz` (the encoder's gradients; each file under 1 MiB): the fp64 gradient of every parameter that has one (`s2d::*`, `enc::*`, `dec::*`; a parameter the
forward never touches is ABSENT), `depth`, the cotangent -- and, instead of the frames and the weights, the seeds that regenerate them
with a checksum of each (`sum::*`).  Nothing of the reference's source is stored: the fixtures are data.

  kbnet_grad_kitti_odd    narrow KITTI preset, 2 x 45 x 77, leaky_relu: maps 23 x 39, 12 x 20, 6 x 10, 3 x 5, 2 x 3
  kbnet_grad_relu_kb02    narrow, resolutions_backprojection (0, 2), relu, 2 x 45 x 77: plain levels 1 and 3

Asserted here: the oracle (tests/kbnet_grad_oracle.py) agrees with the reference to 1e-9 of each tensor's largest element, its set of
parameters without a gradient is the reference's (kbnet_grad_cases.untouched), each file stays under 1 MiB.  A seed that fails one is
replaced, the assertion stays.
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "networks.py")):
    sys.exit(__doc__)
sys.path.insert(0, sys.argv[1])

import kbnet_amd as kb  # noqa: E402,F401
import kbnet_grad_cases as cases  # noqa: E402
import kbnet_grad_oracle as kgo  # noqa: E402
import networks  # noqa: E402  (reference)


def reference_gradients(cfg, image, sparse_depth, validity_map_depth, intrinsics, sd_s2d, sd_enc, sd_dec, cotangent):
    s2d = networks.SparseToDensePool(input_channels=cfg.input_channels_depth, min_pool_sizes=list(cfg.min_pool_sizes_sparse_to_dense_pool),
                                     max_pool_sizes=list(cfg.max_pool_sizes_sparse_to_dense_pool),
                                     n_convolution=cfg.n_convolution_sparse_to_dense_pool, n_filter=cfg.n_filter_sparse_to_dense_pool,
                                     weight_initializer=cfg.weight_initializer, activation_func=cfg.activation_func)
    fi, fd = list(cfg.n_filters_encoder_image), list(cfg.n_filters_encoder_depth)
    encoder = networks.KBNetEncoder(input_channels_image=cfg.input_channels_image, input_channels_depth=cfg.n_filter_sparse_to_dense_pool,
                                    n_filters_image=fi, n_filters_depth=fd, n_filters_fused=list(fi), n_convolutions_image=[1] * 5,
                                    n_convolutions_depth=[1] * 5, n_convolutions_fused=[1] * 5,
                                    resolutions_backprojection=list(cfg.resolutions_backprojection),
                                    weight_initializer=cfg.weight_initializer, activation_func=cfg.activation_func)
    decoder = networks.MultiScaleDecoder(input_channels=fi[-1] + fd[-1], output_channels=1, n_resolution=1,
                                         n_filters=list(cfg.n_filters_decoder), n_skips=cfg.n_skips,
                                         weight_initializer=cfg.weight_initializer, activation_func=cfg.activation_func,
                                         output_func="linear", use_batch_norm=False, deconv_type=cfg.deconv_type)
    mods = (s2d, encoder, decoder)
    for mod, sd in zip(mods, (sd_s2d, sd_enc, sd_dec)):
        mod.load_state_dict(sd, strict=True)
        mod.double()
    torch.set_default_dtype(torch.float64)      # net_utils.meshgrid builds the pixel grid in the default dtype
    try:
        x = s2d(torch.cat([sparse_depth.double(), validity_map_depth.double()], dim=1))      # src/kbnet_model.py:166-173
        latent, skips = encoder(image.double(), x, intrinsics.double())
        output = decoder(latent, skips, x.shape[-2:])[-1]
        depth = cfg.min_predict_depth / (torch.sigmoid(output) + cfg.min_predict_depth / cfg.max_predict_depth)
        (depth * cotangent).sum().backward()
    finally:
        torch.set_default_dtype(torch.float32)
    out = {"depth": depth.detach()}
    for grp, mod in zip(kgo.GROUPS, mods):
        for k, p in mod.named_parameters():
            if p.grad is not None:
                out[f"{grp}::{k}"] = p.grad
    return out


def case(name):
    c = cases.GOLDEN[name]
    args = cases.inputs(c)
    ref = reference_gradients(c["cfg"], *args)
    keys = kgo.gradient_keys(ref)
    absent = sorted(set(kgo.parameter_keys(*args[4:7])) - set(keys))
    assert absent == sorted(cases.untouched(c)) and absent, absent
    flat = {k: v.numpy() for k, v in ref.items()}
    flat["cotangent"] = args[7].numpy()
    flat.update({"sum::" + k: np.float64(v) for k, v in cases.checksums(*args[:7]).items()})
    flat["seed"] = np.int64(c["seed"])
    # two files per case, each under 1 MiB: the encoder's gradients (fp64, incompressible) apart from everything else
    size = 0
    for suffix, part in (("", {k: v for k, v in flat.items() if not k.startswith("enc::")}),
                         ("_enc", {k: v for k, v in flat.items() if k.startswith("enc::")})):
        path = os.path.join(HERE, name + suffix + ".npz")
        np.savez_compressed(path, **part)
        assert os.path.getsize(path) < 1 << 20, (path, os.path.getsize(path))
        size += os.path.getsize(path)
    o64 = kgo.gradients(*args, c["cfg"])
    assert sorted(kgo.gradient_keys(o64)) == sorted(keys)
    worst = max(float((o64[k] - ref[k]).abs().max() / ref[k].abs().max()) for k in keys + ["depth"])
    print(f"{name}: {size / 1024:.0f} KiB  {len(keys)} gradients, {len(absent)} parameters without one  depth "
          f"[{float(ref['depth'].min()):.2f}, {float(ref['depth'].max()):.2f}]  oracle fp64 within {worst:.1e} of the reference")
    assert worst < 1e-9, worst


def main():
    for name in cases.GOLDEN:
        case(name)


if __name__ == "__main__":
    main()
