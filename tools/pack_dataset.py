#!/usr/bin/env python3
"""Converts the PNG files of a dataset to packed frames, which the loaders decode on the GPU instead of the host.

    python tools/pack_dataset.py --paths training/kitti/kitti_train_image.txt training/kitti/kitti_train_sparse_depth.txt \\
                                 --output_root /data/kitti_packed [--list_dir training/kitti_packed] [--workers 8]

--paths: reference-style path lists (one path a line, kb.loader.read_paths) of IMAGE and SPARSE DEPTH files: these are the paths
the loaders take packed; GROUND TRUTH lists may be given too (kb.inference.run and train()'s validation read packed ground truth,
DESIGN 8u).  Intrinsics stay .npy: pass their lists on unchanged.  tools/unpack_dataset.py is the inverse.
Every listed file src becomes <output_root>/<src without its root or drive, suffix .kbf>; a file listed twice is converted once.
An image list may hold sequence entries (previous<TAB>current<TAB>next; tools/sequence_lists.py writes them): each of the
three paths is mapped like any other, every distinct frame is converted once, and the entry is rewritten field by field.
For every list a new one of the same name is written into --list_dir (default: <output_root>/lists), line for line.
Prints the total bytes before and after.  No GPU is needed."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import kbnet_amd as kb  # noqa: E402


def packed_path(src: str, output_root: str) -> str:
    relative = os.path.splitdrive(os.path.normpath(src))[1].lstrip(os.sep)
    while relative.startswith(".." + os.sep):
        relative = relative[3:]
    return os.path.join(output_root, os.path.splitext(relative)[0] + ".kbf")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--paths", nargs="+", required=True, help="path-list files of image and sparse-depth PNGs")
    ap.add_argument("--output_root", required=True)
    ap.add_argument("--list_dir", default=None)
    ap.add_argument("--workers", type=int, default=8)
    args = ap.parse_args()
    list_dir = args.list_dir or os.path.join(args.output_root, "lists")
    os.makedirs(list_dir, exist_ok=True)
    sources, seen = [], set()
    for list_path in args.paths:
        paths = kb.loader.read_paths(list_path)
        kb.loader.write_paths(os.path.join(list_dir, os.path.basename(list_path)),
                              [kb.loader.map_sample(p, lambda path: packed_path(path, args.output_root)) for p in paths])
        for entry in paths:
            for p in kb.loader.split_sample(entry) or (entry,):
                if p not in seen:
                    seen.add(p)
                    sources.append(p)
    before, after = kb.loader.pack_frames(sources, [packed_path(p, args.output_root) for p in sources], workers=args.workers)
    print(f"{len(sources)} files: {before} bytes of PNG -> {after} bytes packed ({after / max(1, before):.3f} of the PNG size)")
    print(f"path lists written to {list_dir}")


if __name__ == "__main__":
    main()
