#!/usr/bin/env python3
"""Writes the image path list of a directory of frame sequences as sequence entries: one line a sample,
previous<TAB>current<TAB>next, the three frames by path.  The loaders assemble the batch from those files; no triplet file is written.

    python tools/sequence_lists.py --root /data/kitti_raw/image_02 --output training/kitti/kitti_train_image.txt [--window 1] [--ends drop]

--root: a directory whose sub-directories are the sequences, taken in sorted order; a sequence is the sorted *.png and *.kbf files of
its directory (a root that holds such files itself is one sequence).  --window: the neighbours are frame idx - window and
idx + window (the reference uses 1 for KITTI, 10 for NYUv2; 0 writes p<TAB>p<TAB>p, its validation and testing images).  --ends:
"drop" leaves out the frames without both neighbours, "repeat" lets the frame stand in for a missing one (kb.loader.sequence_lines).
The sparse-depth, intrinsics and ground-truth lists stay one path a line and must follow the same order: --samples writes the
`current` path of every entry, one a line, to derive them from.  No GPU is needed."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import kbnet_amd as kb  # noqa: E402

FRAME_EXTENSIONS = (".png", ".kbf")


def frames_of(directory: str) -> list:
    return [os.path.join(directory, name) for name in sorted(os.listdir(directory))
            if os.path.splitext(name)[1].lower() in FRAME_EXTENSIONS and os.path.isfile(os.path.join(directory, name))]


def sequences_of(root: str) -> list:
    """The sequences under `root`, each a sorted list of frame paths; directories without frames are skipped."""
    found = [frames_of(os.path.join(root, name)) for name in sorted(os.listdir(root)) if os.path.isdir(os.path.join(root, name))]
    return [frames for frames in [frames_of(root)] + found if frames]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", required=True, help="a directory of sequence directories")
    ap.add_argument("--output", required=True, help="the image path list to write")
    ap.add_argument("--window", type=int, default=1)
    ap.add_argument("--ends", choices=("drop", "repeat"), default="drop")
    ap.add_argument("--samples", default=None, help="also write the current frame of every entry, one a line")
    args = ap.parse_args(argv)
    sequences = sequences_of(args.root)
    lines = [line for frames in sequences for line in kb.loader.sequence_lines(frames, window=args.window, ends=args.ends)]
    kb.loader.write_paths(args.output, lines)
    if args.samples:
        kb.loader.write_paths(args.samples, [kb.loader.sample_name(line) for line in lines])
    print(f"{len(sequences)} sequences, {sum(len(frames) for frames in sequences)} frames -> {len(lines)} samples in {args.output}")


if __name__ == "__main__":
    main()
