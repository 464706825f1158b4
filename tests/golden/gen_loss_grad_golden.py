#!/usr/bin/env python3
"""Generate the golden GRADIENTS of the objective by RUNNING THE REFERENCE on CPU, in fp64, under torch.autograd.

Run in the build container only (needs /root/reference):

    python tests/golden/gen_loss_grad_golden.py

It composes the reference's `net_utils` and `losses` the way its KBNetModel.compute_loss does (gen_loss_golden.reference_loss,
reused as it is) on two cases of tests/loss_cases.py, everything_37x45 and two_plane_50x130, with the depth and the two pose
matrices as leaves, and writes `grad_loss_<case>.npz` next to this script: the gradient of the weighted loss with respect to
the depth (N x 1 x H x W) and to the two poses (N x 4 x 4), the four terms and the loss, all fp64.  The inputs are not stored:
loss_cases.case(name) rebuilds them bit for bit.  Nothing of the reference's source is stored: the fixtures are data.

tests/test_loss_grad_oracle_cpu.py holds tests/loss_oracle.py's fp64 autograd against these files, which makes that oracle the
yardstick every other gradient test uses.
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_loss_golden as base  # noqa: E402  (puts the repository, tests/ and the reference on sys.path; turns grad mode off)
import loss_cases  # noqa: E402  (tests/)

CASES = ("everything_37x45", "two_plane_50x130")


def main():
    torch.set_grad_enabled(True)
    torch.set_default_dtype(torch.float64)   # the reference builds its meshgrid and homogeneous rows in the default dtype
    for name in CASES:
        args = [t.double() for t in loss_cases.case(name)]
        for i in (3, 7, 8):
            args[i].requires_grad_(True)
        out, _, _ = base.reference_loss(*args)
        grads = torch.autograd.grad(out["loss"], [args[3], args[7], args[8]])
        flat = {"grad_output_depth": grads[0].numpy(), "grad_pose01": grads[1].numpy(), "grad_pose02": grads[2].numpy()}
        for k in base.SCALARS:
            flat[k] = np.float64(float(out[k]))
        path = os.path.join(HERE, f"grad_loss_{name}.npz")
        np.savez_compressed(path, **flat)
        size = os.path.getsize(path)
        assert size < 1 << 20, (name, size)
        print(f"grad_loss_{name}: {size / 1024:.0f} KiB  loss {float(out['loss']):.9g}  |grad depth| max {float(grads[0].abs().max()):.3g}  "
              f"|grad pose01| max {float(grads[1].abs().max()):.3g}  |grad pose02| max {float(grads[2].abs().max()):.3g}  "
              f"row 3 {float(grads[1][:, 3].abs().max()):.1g} / {float(grads[2][:, 3].abs().max()):.1g}")


if __name__ == "__main__":
    main()
