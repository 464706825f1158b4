#!/usr/bin/env python3
"""Converts packed frames back to PNG files: the inverse of tools/pack_dataset.py, for whoever must hand PNGs on
(a KITTI submission, a viewer) after exporting with kb.inference.run_with_format(..., output_format="packed").

    python tools/unpack_dataset.py --paths outputs/output_depth.txt --output_root /data/submission \\
                                   [--list_dir /data/submission/lists] [--workers 8] [--png_level 6]

--paths: path lists (one path a line, kb.loader.read_paths) of packed files.  Every listed file src becomes
<output_root>/<src without its root or drive, suffix .png>; a file listed twice is converted once.  For every list a new one of the
same name is written into --list_dir (default: <output_root>/lists), line for line.
8-bit RGB, 8-bit gray and 16-bit gray frames become PNGs with the same pixels (host decode, the native PNG encoders, threads); a
file of any other format is refused by name.  Prints the total bytes before and after.  No GPU is needed."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import kbnet_amd as kb  # noqa: E402


def png_path(src: str, output_root: str) -> str:
    relative = os.path.splitdrive(os.path.normpath(src))[1].lstrip(os.sep)
    while relative.startswith(".." + os.sep):
        relative = relative[3:]
    return os.path.join(output_root, os.path.splitext(relative)[0] + ".png")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--paths", nargs="+", required=True, help="path-list files of packed frames")
    ap.add_argument("--output_root", required=True)
    ap.add_argument("--list_dir", default=None)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--png_level", type=int, default=6)
    args = ap.parse_args()
    list_dir = args.list_dir or os.path.join(args.output_root, "lists")
    os.makedirs(list_dir, exist_ok=True)
    sources, seen = [], set()
    for list_path in args.paths:
        paths = kb.loader.read_paths(list_path)
        kb.loader.write_paths(os.path.join(list_dir, os.path.basename(list_path)), [png_path(p, args.output_root) for p in paths])
        for p in paths:
            if p not in seen:
                seen.add(p)
                sources.append(p)
    before, after = kb.loader.unpack_frames(sources, [png_path(p, args.output_root) for p in sources], workers=args.workers,
                                            level=args.png_level)
    print(f"{len(sources)} files: {before} bytes packed -> {after} bytes of PNG ({after / max(1, before):.3f} of the packed size)")
    print(f"path lists written to {list_dir}")


if __name__ == "__main__":
    main()
