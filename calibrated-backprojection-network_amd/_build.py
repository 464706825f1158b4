"""Builds csrc/*.hip into libkbnet_hip.so (gfx950) with hipcc, in-tree.

The shared library is git-ignored but travels to the GPU box with the snapshot.
`python -m kbnet_build` style use: `from kbnet_amd import _build; _build.build()`.
"""

from __future__ import annotations

import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libkbnet_hip.so")
OBJ_DIR = os.path.join(HERE, "csrc", "_obj")
# longest translation units first: the pool then ends with the short ones
SOURCES = ["conv_igemm.hip", "conv_dma_t1.hip", "conv_dma_t2.hip", "conv_dma_t4.hip", "conv_split.hip", "upconv_split.hip", "conv_up2x.hip", "kb_pair_nb3.hip",
           "conv_wino.hip", "s2d.hip", "kb1_depth_front.hip", "kb1_front.hip", "kb_pair_nb4.hip", "conv1x1s2_split.hip", "kb_pair.hip", "head.hip", "tail.hip", "kb.hip", "conv_dma.hip",
           "tune.hip", "abi.hip", "pre_eval.hip", "loss.hip", "loss_backward.hip", "conv_bwd_weight.hip", "posenet_backward.hip", "bn_sync.hip", "conv_affine_backward.hip", "kbnet_backward.hip", "posenet.hip", "conv_affine.hip", "unpack.hip", "unpack_train.hip", "unpack_packed.hip", "unpack_sequence.hip", "pack_frames.hip", "frame_pack.hip", "export_pack.hip", "point_cloud.hip", "io_png.hip", "elementwise.hip", "adam.hip", "augment.hip", "multi_copy.hip", "summary.hip", "histogram.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Wall",
         "-Wno-unused-function"]


def _hipcc() -> str:
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found (needed to build libkbnet_hip.so)")
    return exe


def _stale(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _depfile_deps(depfile: str):
    """The prerequisites hipcc -MMD wrote for one object (the source and every header it included), or None when the
    depfile is missing or unreadable."""
    try:
        with open(depfile) as f:
            text = f.read().replace("\\\n", " ")
        deps = text.split(":", 1)[1].split()
    except (OSError, IndexError):
        return None
    return deps if deps and all(os.path.exists(d) for d in deps) else None


def build(force: bool = False, verbose: bool = True) -> str:
    hipcc = _hipcc()
    extra = os.environ.get("KBN_HIPCC_FLAGS", "").split()  # experiments, e.g. -DKBN_WAVES_PER_SIMD=3
    if extra:
        force = True
    os.makedirs(OBJ_DIR, exist_ok=True)
    jobs = []
    objs = []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(OBJ_DIR, src.replace(".hip", ".o"))
        objs.append(o)
        deps = _depfile_deps(o + ".d")   # written by the compiler with the object: the source and every header it read
        if force or deps is None or _stale(o, [s] + deps):
            jobs.append([hipcc] + FLAGS + extra + ["-MMD", "-MF", o + ".d", "-c", s, "-o", o])

    def run(cmd):
        if verbose:
            print("[kbnet build]", " ".join(os.path.relpath(c) if os.path.isabs(c) else c for c in cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed:\n" + r.stdout + r.stderr)
        if verbose and r.stderr.strip():
            print(r.stderr, file=sys.stderr)

    with ThreadPoolExecutor(max_workers=max(1, min(8, os.cpu_count() or 4))) as ex:
        list(ex.map(run, jobs))
    if force or jobs or _stale(LIB, objs):
        run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs + ["-lz"])
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
