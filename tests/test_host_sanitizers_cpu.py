"""CPU: the host code between untrusted bytes and the device, and the size functions Python allocates from, in sanitizer builds.

tests/host_san holds three stand-alone programs, each with its own main():
  codec_fuzz      csrc/frame_pack.hip + csrc/io_png.hip under AddressSanitizer and UndefinedBehaviorSanitizer
  size_sweep      every size_t-returning function of include/kbnet_hip.h over extreme arguments, same sanitizers
  png_batch_tsan  kbn_png_decode_batch under ThreadSanitizer
This module builds them (hipcc, the flags of _build.py with -O3 replaced by -O1 -g, the sanitizers on the host side only) into
pytest's temporary directory and runs them with subprocess.  The sanitized objects are linked into these programs alone: nothing
sanitized is loaded into python, no library is preloaded, nothing here touches a GPU.

The power of it all is proved here too: a ten-line program with a heap overrun and a signed overflow must be reported by the same
build helper (the sanitizer flags do something), and codec_fuzz built against a copy of frame_pack.hip with a check removed must
exit nonzero with a sanitizer report."""
import ctypes
import os
import re
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import pytest

import kbnet_amd as kb
from conftest import GOLDEN_DIR, ROOT

HERE = os.path.join(ROOT, "tests", "host_san")
CSRC = kb._build.CSRC
JOBS = max(1, min(16, os.cpu_count() or 1))
ASAN_UBSAN = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
TSAN = ["-Xarch_host", "-fsanitize=thread"]
# the sources that define the size functions or what those call; linked with --gc-sections, so that the launch paths these files
# also hold (and the rest of the library they call) stay out: the sweep launches nothing
SIZE_SOURCES = ["conv_igemm.hip", "conv_split.hip", "conv_up2x.hip", "conv_wino.hip", "conv_affine.hip", "conv1x1s2_split.hip",
                "kb1_front.hip", "kb1_depth_front.hip", "tail.hip", "posenet.hip", "posenet_backward.hip", "conv_affine_backward.hip",
                "conv_bwd_weight.hip", "augment.hip", "pack_frames.hip", "frame_pack.hip", "io_png.hip"]


def _flags(sanitizer):
    """_build.py's FLAGS with -O3 replaced by -O1 -g; debug information for the host only (the device side of a file is compiled as
    ever, and nothing here runs it: -g there only costs build time)."""
    assert "-O3" in kb._build.FLAGS
    out = []
    for f in kb._build.FLAGS:
        out += ["-O1", "-g", "-Xarch_device", "-g0"] if f == "-O3" else [f]
    return out + sanitizer


def _link_flag(sanitizer):
    return [f for f in sanitizer if f.startswith("-fsanitize=")]


class BuildError(RuntimeError):
    pass


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise BuildError(" ".join(cmd[:1] + cmd[-4:]) + "\n" + (r.stdout + r.stderr)[-3000:])


def compile_one(src, obj, sanitizer, extra=()):
    _run([kb._build._hipcc()] + _flags(sanitizer) + list(extra) + ["-x", "hip", "-c", src, "-o", obj])
    return obj


def link(objs, exe, sanitizer, extra=()):
    _run([kb._build._hipcc(), "--offload-arch=gfx950"] + _link_flag(sanitizer) + list(extra) + list(objs) + ["-o", exe, "-lz"])
    return exe


def execute(cmd, timeout=300):
    """(exit status, output) of a program; its environment is this process's, untouched."""
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    return r.returncode, r.stdout + r.stderr


def fixtures():
    import glob
    names = sorted(glob.glob(os.path.join(GOLDEN_DIR, "io", "*.png")) + glob.glob(os.path.join(GOLDEN_DIR, "train_io", "*.png")))
    assert len(names) >= 15
    return names


TEN_LINES = """
#include <stdio.h>
#include <stdlib.h>
int main(int argc, char** argv) {
    volatile int big = 2147483646;
    volatile size_t n = 16;             /* a size the compiler cannot see: the overrun is AddressSanitizer's to find */
    unsigned char* p = (unsigned char*)malloc(n);
    if (argc > 1) p[n] = 1;             /* one byte past the block */
    big += argc + 1;                    /* past INT_MAX */
    printf("%d %d\\n", (int)big, (int)p[0] * 0);
    free(p);
    return 0;
}
"""


@pytest.fixture(scope="module")
def toolchain(tmp_path_factory):
    """The directory the programs are built in -- after the ten-line program has linked.  The only skip of this module: a toolchain
    without the sanitizers' runtime libraries, which shows as a link error of that program."""
    d = tmp_path_factory.mktemp("host_san")
    src = d / "ten_lines.cpp"
    src.write_text(TEN_LINES)
    compile_one(str(src), str(d / "ten_lines.o"), ASAN_UBSAN)
    try:
        link([str(d / "ten_lines.o")], str(d / "ten_lines"), ASAN_UBSAN)
    except BuildError as e:
        text = str(e)      # only a runtime library the linker cannot find: any other failed link is a failure
        if re.search(r"(cannot find|cannot open|unable to find|no such file)[^\n]*(clang_rt\.(asan|ubsan)|lib(asan|ubsan))", text, flags=re.I):
            pytest.skip("the toolchain has no sanitizer runtime to link: " + text[-600:])
        raise
    return d


@pytest.fixture(scope="module")
def programs(toolchain):
    """The three programs, built together on at most min(16, CPUs) jobs.  {name: path}, 'seconds': the build's wall clock,
    'objects': what codec_fuzz was linked from (the power test swaps one of them)."""
    d = toolchain
    t0 = time.time()
    jobs = []
    for name in SIZE_SOURCES:      # the long translation units first
        jobs.append((os.path.join(CSRC, name), str(d / ("size_" + name[:-4] + ".o")), ASAN_UBSAN, ("-ffunction-sections", "-fdata-sections")))
    for name in ("frame_pack.hip", "io_png.hip"):
        jobs.append((os.path.join(CSRC, name), str(d / (name[:-4] + ".o")), ASAN_UBSAN, ()))
    jobs.append((os.path.join(CSRC, "io_png.hip"), str(d / "io_png_tsan.o"), TSAN, ()))
    jobs.append((os.path.join(HERE, "codec_fuzz.cpp"), str(d / "codec_fuzz.o"), ASAN_UBSAN, ()))
    jobs.append((os.path.join(HERE, "size_sweep.cpp"), str(d / "size_sweep.o"), ASAN_UBSAN, ()))
    jobs.append((os.path.join(HERE, "png_batch_tsan.cpp"), str(d / "png_batch_tsan.o"), TSAN, ()))
    with ThreadPoolExecutor(max_workers=JOBS) as pool:
        list(pool.map(lambda j: compile_one(*j), jobs))
    out = {"objects": [str(d / "codec_fuzz.o"), str(d / "frame_pack.o"), str(d / "io_png.o")]}
    out["codec_fuzz"] = link(out["objects"], str(d / "codec_fuzz"), ASAN_UBSAN)
    out["size_sweep"] = link([str(d / "size_sweep.o")] + [j[1] for j in jobs[:len(SIZE_SOURCES)]], str(d / "size_sweep"), ASAN_UBSAN,
                             ("-Wl,--gc-sections",))
    out["png_batch_tsan"] = link([str(d / "png_batch_tsan.o"), str(d / "io_png_tsan.o")], str(d / "png_batch_tsan"), TSAN)
    out["seconds"] = time.time() - t0
    return out


def _report(capsys, text):
    with capsys.disabled():      # the log lists the programs, their counts and times even when everything passes
        sys.stdout.write("\n" + text.rstrip() + "\n")


# ------------------------------------------------------------------------------ the power of the build helper
def test_the_sanitizer_flags_are_live(toolchain):
    """-Xarch_host silently doing nothing would make every other test here vacuous."""
    exe = str(toolchain / "ten_lines")
    status, out = execute([exe, "overrun"])
    assert status != 0 and "heap-buffer-overflow" in out, out[-800:]
    status, out = execute([exe])
    assert status != 0 and "runtime error:" in out and "signed integer overflow" in out, out[-800:]


# ------------------------------------------------------------------------------ what the sweep found, kept in the plain suite
def test_size_functions_refuse_what_the_sweep_found():
    """The arguments size_sweep first failed on, through the ordinary library: each answers 0 (before: signed overflow in ceil_div /
    round_up, or the low 64 bits of a longer product), ordinary shapes answer as before, and the entry points that size a caller's
    blob by these functions refuse too."""
    lib = kb._lib.load()
    top = 2 ** 31 - 1
    assert lib.kbn_conv2d_packed_weight_bytes(top - 1, 1, 1, 1) == 0 and lib.kbn_conv2d_packed_weight_bytes(1, top, 3, 2) == 0
    assert lib.kbn_upconv2x_packed_weight_bytes(top - 1, 1) == 0
    assert lib.kbn_conv3x3_split_packed_weight_bytes(top - 1, 16, 0) == 0
    assert lib.kbn_conv1x1s2_split_packed_weight_bytes(top - 1, 16, 0) == 0
    assert lib.kbn_conv2d_s2_affine_packed_weight_bytes(top - 1, 1, 3) == 0
    assert lib.kbn_conv2d_s2_backward_data_packed_weight_bytes(1, top - 1, 3) == 0
    assert lib.kbn_conv2d_affine_packed_weight_bytes(top - 1, 1, 1) == 0
    assert lib.kbn_conv2d_backward_data_packed_weight_bytes(1, top - 1, 1, 1) == 0
    assert lib.kbn_conv2d_s2_backward_weight_scratch_bytes(1, 1, 1, 3, top, 1, 1) == 0
    assert lib.kbn_conv2d_backward_weight_scratch_bytes(1, top, 1, 1, 1, 1, 1, 1) == 0
    assert lib.kbn_conv2d_backward_weight_scratch_bytes(1 << 20, 512, 65535, 1, 1, 1 << 24, 1 << 20, 512) == 0
    assert lib.kbn_frame_encode_bound(top, top, 4, 8) == 0 and lib.kbn_pack_frames_stride(top, top, 4, 8) == 0
    records = (kb._lib.AugmentTensor * 2)()
    for r in records:
        r.channels, r.role = top, kb._lib.KBN_AUGMENT_ROLE_RANGE
    assert lib.kbn_augment_workspace_bytes(records, 2, top, 3, 1) == 0
    records[0].channels = records[1].channels = 1
    assert lib.kbn_augment_workspace_bytes(records, 2, 4, 8, 16) == 2 * 4 * (16 + 8 * 8 * 16)
    # the limits themselves are inside
    m = kb._lib.KBN_MAX_CHANNELS
    assert lib.kbn_conv2d_packed_weight_bytes(m, 16, 1, 1) >= 2 * m * 16 and lib.kbn_conv2d_packed_weight_bytes(m + 1, 16, 1, 1) == 0
    assert lib.kbn_conv2d_packed_weight_bytes(m, 256, 1, 1) > 0 and lib.kbn_conv2d_packed_weight_bytes(m, 257, 1, 1) == 0      # 2^28 weights
    assert lib.kbn_conv2d_packed_weight_bytes(64, 48, 3, 1) > 0 and lib.kbn_upconv2x_packed_weight_bytes(64, 48) > 0
    with open(os.path.join(ROOT, "include", "kbnet_hip.h")) as f:
        header = f.read()
    for name, value in (("KBN_MAX_CHANNELS", m), ("KBN_MAX_WEIGHT_ELEMENTS", kb._lib.KBN_MAX_WEIGHT_ELEMENTS), ("KBN_MAX_MAP_SIDE", kb._lib.KBN_MAX_MAP_SIDE)):
        assert int(re.search(r"#define " + name + r" (\d+)", header).group(1)) == value
    # entry points that size a blob by these functions refuse before any launch (the pointers are never followed)
    assert lib.kbn_conv2d_pack_weight(0x1000, 0x2000, top - 1, 1, 1, 1, None) == kb._lib.KBN_ERR_UNSUPPORTED
    assert lib.kbn_upconv2x_pack_weight(0x1000, 0x2000, top - 1, 1, None) == kb._lib.KBN_ERR_UNSUPPORTED
    assert lib.kbn_conv3x3_split_pack_weight(0x1000, 0x2000, top - 1, 16, 0, None) == kb._lib.KBN_ERR_INVALID_ARGUMENT
    buf, n = (ctypes.c_ubyte * 16)(), ctypes.c_size_t(5)
    assert lib.kbn_frame_encode(buf, top, top, 4, 8, buf, 16, ctypes.byref(n)) == kb._lib.KBN_ERR_UNSUPPORTED and n.value == 5


# ------------------------------------------------------------------------------ the three programs
def test_codec_fuzz(programs, capsys):
    t0 = time.time()
    status, out = execute([programs["codec_fuzz"]] + fixtures())
    lines = [l for l in out.splitlines() if l.startswith("codec_fuzz")]
    _report(capsys, f"host_san: built in {programs['seconds']:.0f} s on {JOBS} jobs; codec_fuzz ran {time.time() - t0:.1f} s\n" + "\n".join(lines))
    assert status == 0 and "codec_fuzz: ok" in out, out[-3000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out
    assert any("non-canonical" in l for l in lines) and any(l.startswith("codec_fuzz png:") and "fixtures" in l for l in lines)


def test_size_sweep(programs, capsys):
    """One process a function: a sanitizer report ends a process, and one function's report must not hide the next one's."""
    t0 = time.time()
    status, out = execute([programs["size_sweep"], "--list"])
    names = out.split()
    with open(os.path.join(ROOT, "include", "kbnet_hip.h")) as f:
        declared = re.findall(r"^size_t (kbn_\w+)\(", f.read(), flags=re.M)
    assert status == 0 and sorted(names) == sorted(declared) and len(names) >= 20      # every size function of the header is swept
    with ThreadPoolExecutor(max_workers=JOBS) as pool:
        results = list(pool.map(lambda n: execute([programs["size_sweep"], n]), names))
    failed, summary = [], []
    for name, (status, out) in zip(names, results):
        summary += [l for l in out.splitlines() if l.startswith(name)]
        if status != 0 or "runtime error:" in out or "ERROR: AddressSanitizer" in out or "FAIL" in out:
            keep = [l for l in out.splitlines() if "runtime error:" in l or "ERROR:" in l or l.startswith(("FAIL", "size_sweep:"))]
            failed.append(f"{name} (exit {status}):\n    " + "\n    ".join(keep[:8]))
    _report(capsys, f"host_san: size_sweep ran {time.time() - t0:.1f} s, {len(names)} functions\n" + "\n".join(summary))
    assert not failed, f"{len(failed)} of {len(names)} size functions fail:\n" + "\n".join(failed)


def test_png_batch_tsan(programs, capsys):
    t0 = time.time()
    status, out = execute([programs["png_batch_tsan"]] + fixtures())
    _report(capsys, f"host_san: png_batch_tsan ran {time.time() - t0:.1f} s\n" + "\n".join(l for l in out.splitlines() if l.startswith("png_batch_tsan")))
    assert status == 0 and "png_batch_tsan: ok" in out and "ThreadSanitizer" not in out, out[-3000:]
    assert "32 decoded, 32 refused" in out


# ------------------------------------------------------------------------------ the power of codec_fuzz
# (old text, new text): exact replacements in a temporary copy of csrc/frame_pack.hip, each a check of check_file removed.
# check_file walks the entries in order and reads a plane's header bytes before it looks at the next entry, so `hi > payload_bytes`
# (with `hi - lo >= heads`) is what keeps `lo + heads` inside the payload: without it a file whose payload is cut short, with
# payload_bytes and the last entry saying so and an inner entry above them, is read past its end.  Without the `heads` check a
# plane cut inside its header bytes is; without the `bits` check the bit reader shifts by 64 and more.
PLANTED = {
    "entry above payload_bytes": ("if (lo > hi || hi > L.payload_bytes) return KBN_ERR_INVALID_ARGUMENT;", "if (lo > hi) return KBN_ERR_INVALID_ARGUMENT;"),
    "plane shorter than its header bytes": ("        if (hi - lo < heads) return KBN_ERR_INVALID_ARGUMENT;\n", ""),
    "header byte above bits": ("                if (b > L.bits) return KBN_ERR_INVALID_ARGUMENT;\n", ""),
}


@pytest.mark.parametrize("name", sorted(PLANTED))
def test_codec_fuzz_catches_a_planted_mistake(programs, toolchain, name):
    old, new = PLANTED[name]
    with open(os.path.join(CSRC, "frame_pack.hip")) as f:
        text = f.read()
    assert text.count(old) == 1, f"csrc/frame_pack.hip moved: {old!r} occurs {text.count(old)} times"
    tag = "planted_" + str(sorted(PLANTED).index(name))
    src = toolchain / (tag + ".hip")
    src.write_text(text.replace(old, new))
    obj = compile_one(str(src), str(toolchain / (tag + ".o")), ASAN_UBSAN, ("-I", CSRC))
    objects = [obj if o.endswith("frame_pack.o") else o for o in programs["objects"]]
    assert obj in objects
    exe = link(objects, str(toolchain / ("codec_fuzz_" + tag)), ASAN_UBSAN)
    status, out = execute([exe])      # the packed half is enough: no PNG given
    assert status != 0, out[-1500:]
    assert "ERROR: AddressSanitizer" in out or "runtime error:" in out, out[-1500:]
    assert "codec_fuzz: ok" not in out and "seed" in out      # and the report names where
