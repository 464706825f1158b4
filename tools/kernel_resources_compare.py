#!/usr/bin/env python3
"""Are the kernels of two source trees the same?  Compiles every csrc/*.hip of both to device assembly (hipcc, _build.py's FLAGS,
--offload-device-only -S), runs tools/kernel_resources.py over each file and prints one line a source file: its kernels, the
largest VGPR (arch + acc), SGPR, LDS and scratch figure among them, and SHA-256 prefixes of the tool's whole per-kernel table and
of the assembly (the compilation-unit id, a hash of the source path, masked), before -> after, each marked same or DIFFERENT.
Exit status 1 when anything differs.  A change that touches host code only must give `same` everywhere (profiles/r23).
usage: kernel_resources_compare.py BEFORE_CSRC AFTER_CSRC [--jobs N] [--tables DIR]   (--tables: keep the full per-kernel tables there)
       e.g.  git archive HEAD~1 calibrated-backprojection-network_amd/csrc include | tar -x -C /tmp/parent"""
import argparse, glob, hashlib, importlib.util, os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
spec = importlib.util.spec_from_file_location("_build", os.path.join(HERE, "..", "calibrated-backprojection-network_amd", "_build.py"))
_build = importlib.util.module_from_spec(spec)
spec.loader.exec_module(_build)


def assembly(src, out):
    subprocess.run([_build._hipcc()] + _build.FLAGS + ["--offload-device-only", "-S", "-c", src, "-o", out], check=True, capture_output=True)
    with open(out) as f:
        return re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", f.read())


def table(path):
    return subprocess.run([sys.executable, os.path.join(HERE, "kernel_resources.py"), path], check=True, capture_output=True, text=True).stdout


VGPR = r"vgpr\(arch\+acc\)"


def top(text, key):
    return max([int(x) for x in re.findall(key + r"\s+(\d+)", text)] or [0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--jobs", type=int, default=max(1, min(16, os.cpu_count() or 1)))
    ap.add_argument("--tables", default=None)
    args = ap.parse_args()
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(args.after, "*.hip")))
    digest = lambda t: hashlib.sha256(t.encode()).hexdigest()[:16]
    with tempfile.TemporaryDirectory() as tmp:
        def one(job):
            side, name = job
            src = os.path.join(args.before if side == "before" else args.after, name)
            if not os.path.exists(src):
                return job, ("", "")
            out = os.path.join(tmp, side + "_" + name[:-4] + ".s")
            asm = assembly(src, out)
            return job, (asm, table(out))
        with ThreadPoolExecutor(max_workers=args.jobs) as pool:
            done = dict(pool.map(one, [(side, n) for n in names for side in ("before", "after")]))
    kernels = different = 0
    for name in names:
        (asm_b, tab_b), (asm_a, tab_a) = done[("before", name)], done[("after", name)]
        n = len(tab_a.splitlines())
        kernels += n
        different += (tab_a != tab_b) + (asm_a != asm_b)
        print(f"{name:26s} {n:4d} kernels  max vgpr {top(tab_a, VGPR):4d} sgpr {top(tab_a, 'sgpr'):4d} lds {top(tab_a, 'lds'):6d} "
              f"scratch {top(tab_a, 'scratch'):5d}  table {digest(tab_b)} -> {digest(tab_a)} {'same' if tab_a == tab_b else 'DIFFERENT'}  "
              f"assembly {digest(asm_b)} -> {digest(asm_a)} {'same' if asm_a == asm_b else 'DIFFERENT'}")
        if args.tables:
            os.makedirs(args.tables, exist_ok=True)
            for side, text in (("before", tab_b), ("after", tab_a)):
                with open(os.path.join(args.tables, f"{name[:-4]}_{side}.txt"), "w") as f:
                    f.write(text)
    print(f"total {kernels} kernels, {different} differences")
    return 1 if different else 0


if __name__ == "__main__":
    sys.exit(main())
