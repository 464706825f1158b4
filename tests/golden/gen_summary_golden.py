#!/usr/bin/env python
"""Generate tests/golden/summary.npz by RUNNING THE REFERENCE's log_utils.colorize (src/log_utils.py:48-75) on the CPU.

    python tests/golden/gen_summary_golden.py <the reference's src directory>

Nothing of the reference's source is stored: the fixture is data.  Recorded for 'viridis' and 'inferno':
  table::<map>     256 x 3: colorize of summary_oracle.ramp(), one value inside every entry's interval -- the colour tables
  edges::<map>     colorize of summary_oracle.EDGE_VALUES (negative, -0, 0, exactly 1, above 1, +-inf, NaN, the last entry's ends)
  random::<map>    colorize of `random::x`, 3 x 1 x 9 x 11 values in [-0.1, 1.1)
The reference's kbnet_model.py does not import here (torchvision), so log_summary's own expressions are restated in
tests/summary_oracle.py and checked against torch on the CPU by tests/test_summary_cpu.py."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import summary_oracle as so  # noqa: E402


def main(reference_src):
    sys.path.insert(0, reference_src)
    import log_utils  # noqa: E402  (reference)
    rng = np.random.default_rng(417)
    x = rng.uniform(-0.1, 1.1, size=(3, 1, 9, 11)).astype(np.float32)
    out = {"random::x": x, "edges::x": so.EDGE_VALUES}
    for name in so.MAPS:
        ramp = log_utils.colorize(torch.from_numpy(so.ramp().reshape(1, 1, 16, 16)), colormap=name).numpy()
        out["table::" + name] = np.ascontiguousarray(ramp.reshape(3, 256).T)
        out["edges::" + name] = log_utils.colorize(torch.from_numpy(so.EDGE_VALUES.reshape(1, 1, 1, -1)), colormap=name).numpy()
        out["random::" + name] = log_utils.colorize(torch.from_numpy(x), colormap=name).numpy()
    path = os.path.join(HERE, "summary.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
