"""CPU: sequence entries of an image path list -- the syntax (split_sample, sequence_lines), tools/sequence_lists.py,
pack_frames on shared frames, and the two new entry points up to the point where they would launch: header, binding and exported
symbols, and every argument check with its documented code.  No GPU is needed: the checks come before any launch."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import kbnet_amd as kb
from conftest import ROOT

KbnError = kb._lib.KbnError
INVALID, UNSUPPORTED = kb._lib.KBN_ERR_INVALID_ARGUMENT, kb._lib.KBN_ERR_UNSUPPORTED
ENTRY_POINTS = ("kbn_unpack_sequence_frames_forward", "kbn_unpack_packed_sequence_frames_forward")


# ------------------------------------------------------------------------------------------------ the syntax
def test_split_sample_knows_a_path_from_three():
    assert kb.loader.split_sample("/data/a b/triplet.png") is None
    assert kb.loader.split_sample("p.png\tc.png\tn.png") == ("p.png", "c.png", "n.png")
    assert kb.loader.split_sample("c\tc\tc") == ("c", "c", "c")
    assert kb.loader.sample_name("p.png\tdir/c.png\tn.png") == "dir/c.png" and kb.loader.sample_name("t.png") == "t.png"
    assert kb.loader.map_sample("a\tb\tc", str.upper) == "A\tB\tC" and kb.loader.map_sample("a", str.upper) == "A"


@pytest.mark.parametrize("entry", ["a\tb", "a\tb\tc\td", "\tb\tc", "a\t\tc", "a\tb\t", "\t", "\t\t"])
def test_split_sample_refuses_malformed_entries(entry):
    with pytest.raises(KbnError) as e:
        kb.loader.split_sample(entry)
    assert repr(entry) in str(e.value), "the entry is quoted"


def _expected_lines(paths, window, ends):
    """The issue's rule, written out: neighbours idx -+ window; drop: range(w, n - w); repeat: the frame itself."""
    n = len(paths)
    out = []
    for idx in range(n):
        lo, hi = idx - window, idx + window
        if ends == "drop" and (lo < 0 or hi >= n):
            continue
        out.append((paths[lo] if lo >= 0 else paths[idx], paths[idx], paths[hi] if hi < n else paths[idx]))
    return out


@pytest.mark.parametrize("window", [0, 1, 10])
@pytest.mark.parametrize("ends", ["drop", "repeat"])
@pytest.mark.parametrize("n", [0, 1, 2, 3, 5, 20, 21, 25])
def test_sequence_lines(window, ends, n):
    paths = [f"seq/{i:04d}.png" for i in range(n)]
    lines = kb.loader.sequence_lines(paths, window=window, ends=ends)
    assert [kb.loader.split_sample(line) for line in lines] == _expected_lines(paths, window, ends)
    if ends == "drop":
        assert len(lines) == max(0, n - 2 * window), "shorter than 2 window + 1: nothing"
    else:
        assert len(lines) == n
    if window == 0:
        assert lines == [f"{p}\t{p}\t{p}" for p in paths]


def test_sequence_lines_defaults_and_refusals():
    paths = ["a", "b", "c", "d"]
    assert kb.loader.sequence_lines(paths) == ["a\tb\tc", "b\tc\td"]
    assert kb.loader.sequence_lines(paths, ends="repeat") == ["a\ta\tb", "a\tb\tc", "b\tc\td", "c\td\td"]
    for bad in (dict(window=-1), dict(ends="wrap")):
        with pytest.raises(KbnError):
            kb.loader.sequence_lines(paths, **bad)
    for bad in (["a", "b\tc"], ["a", ""]):
        with pytest.raises(KbnError):
            kb.loader.sequence_lines(bad)


def test_read_paths_returns_a_sequence_entry_whole(tmp_path):
    lines = kb.loader.sequence_lines(["x/0.png", "x/1.png", "x/2.png"], ends="repeat")
    kb.loader.write_paths(str(tmp_path / "image.txt"), lines)
    assert kb.loader.read_paths(str(tmp_path / "image.txt")) == lines


# ------------------------------------------------------------------------------------------------ tools/sequence_lists.py
def _tree(root):
    """Two sequences and a directory without frames; names that sort differently as numbers and as strings stay out."""
    made = {}
    for name, frames in (("drive_b", ["0002.png", "0000.png", "0001.png", "notes.txt"]), ("drive_a", ["00.kbf", "01.kbf", "02.kbf", "03.kbf"]),
                         ("empty", ["readme.md"])):
        os.makedirs(root / name)
        for f in frames:
            (root / name / f).write_bytes(b"")
        made[name] = sorted(str(root / name / f) for f in frames if f.endswith((".png", ".kbf")))
    return made


@pytest.mark.parametrize("window, ends", [(1, "drop"), (0, "drop"), (2, "repeat")])
def test_sequence_lists_tool(tmp_path, window, ends):
    made = _tree(tmp_path / "raw")
    out, samples = str(tmp_path / "image.txt"), str(tmp_path / "current.txt")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "sequence_lists.py"), "--root", str(tmp_path / "raw"), "--output", out,
                          "--window", str(window), "--ends", ends, "--samples", samples], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-600:]
    want = kb.loader.sequence_lines(made["drive_a"], window, ends) + kb.loader.sequence_lines(made["drive_b"], window, ends)
    assert kb.loader.read_paths(out) == want and len(want) > 0
    assert kb.loader.read_paths(samples) == [kb.loader.split_sample(line)[1] for line in want]
    assert "2 sequences, 7 frames" in res.stdout


# ------------------------------------------------------------------------------------------------ pack_frames
def test_pack_frames_packs_each_shared_frame_once(tmp_path):
    rng = np.random.default_rng(5)
    frames = [rng.integers(0, 256, size=(9, 17, 3), dtype=np.uint8) for _ in range(4)]
    src = [str(tmp_path / "png" / f"{i}.png") for i in range(4)]
    os.makedirs(tmp_path / "png")
    for path, px in zip(src, frames):
        with open(path, "wb") as f:
            f.write(kb.loader.encode_image_png(px))
    entries = kb.loader.sequence_lines(src, window=1, ends="repeat")      # 4 entries, 12 fields, 4 distinct files
    to_packed = lambda path: str(tmp_path / "packed" / (os.path.splitext(os.path.basename(path))[0] + ".kbf"))
    rewritten = [kb.loader.map_sample(entry, to_packed) for entry in entries]
    before, after = kb.loader.pack_frames(entries, rewritten, workers=3)
    assert before == sum(os.path.getsize(p) for p in src), "every distinct PNG is read once"
    assert sorted(os.listdir(tmp_path / "packed")) == ["0.kbf", "1.kbf", "2.kbf", "3.kbf"]
    assert after == sum(os.path.getsize(tmp_path / "packed" / name) for name in os.listdir(tmp_path / "packed"))
    kb.loader.write_paths(str(tmp_path / "image.txt"), rewritten)
    for entry, original in zip(kb.loader.read_paths(str(tmp_path / "image.txt")), entries):
        for packed, png in zip(kb.loader.split_sample(entry), kb.loader.split_sample(original)):
            with open(packed, "rb") as f:
                assert np.array_equal(kb.loader.decode_frame(f.read()), frames[src.index(png)])
    # a list may mix plain paths and sequence entries; an entry and its destination must have one form
    kb.loader.pack_frames([src[0], entries[1]], [to_packed(src[0]), rewritten[1]], workers=1)
    with pytest.raises(KbnError):
        kb.loader.pack_frames([entries[0]], [to_packed(src[0])])


def test_pack_dataset_tool_rewrites_sequence_entries(tmp_path):
    os.makedirs(tmp_path / "seq")
    src = [str(tmp_path / "seq" / f"{i}.png") for i in range(3)]
    for i, path in enumerate(src):
        with open(path, "wb") as f:
            f.write(kb.loader.encode_image_png(np.full((8, 16, 3), 40 * i, dtype=np.uint8)))
    kb.loader.write_paths(str(tmp_path / "image.txt"), kb.loader.sequence_lines(src, ends="repeat"))
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pack_dataset.py"), "--paths", str(tmp_path / "image.txt"),
                          "--output_root", str(tmp_path / "out"), "--workers", "2"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-600:]
    assert res.stdout.startswith("3 files:"), res.stdout
    entries = kb.loader.read_paths(str(tmp_path / "out" / "lists" / "image.txt"))
    assert len(entries) == 3
    for entry, k in zip(entries, ((0, 0, 1), (0, 1, 2), (1, 2, 2))):
        for path, i in zip(kb.loader.split_sample(entry), k):
            with open(path, "rb") as f:
                assert np.array_equal(kb.loader.decode_frame(f.read()), np.full((8, 16, 3), 40 * i, dtype=np.uint8))


# ------------------------------------------------------------------------------------------------ header, binding, library
def _declaration(name):
    header = open(os.path.join(ROOT, "include", "kbnet_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", header, flags=re.S)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def _struct_fields(name):
    header = open(os.path.join(ROOT, "include", "kbnet_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    body = re.search(r"typedef struct " + name + r"\s*\{(.*?)\}\s*" + name + r"\s*;", header, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        ctype, names = decl.rsplit(" ", 1)[0], decl.rsplit(" ", 1)[1]
        if "," in decl:      # `int y_start, x_start`
            ctype = decl.split(" ", 1)[0]
            names = decl.split(" ", 1)[1]
        for n in names.split(","):
            n = n.strip()
            count = int(n[n.index("[") + 1:n.index("]")]) if "[" in n else 1
            fields.append((n.split("[")[0], ctype, count))
    return fields


def test_header_binding_and_library_agree_on_the_two_entry_points():
    lib = kb._lib.load()
    base = {"long long": C.c_longlong, "unsigned int": C.c_uint, "int": C.c_int}
    for entry, record, mirror, size in ((ENTRY_POINTS[0], "kbn_sequence_frame", kb._lib.SequenceFrame, 48),
                                        (ENTRY_POINTS[1], "kbn_packed_sequence_frame", kb._lib.PackedSequenceFrame, 64)):
        assert hasattr(lib, entry), entry
        args = _declaration(entry)
        res, bound = kb._lib.SIGNATURES[entry]
        assert res is C.c_int and len(args) == len(bound) == 15
        for text, ctype in zip(args, bound):
            if "size_t" in text:
                assert ctype is C.c_size_t, text
            elif record in text:
                assert ctype is C.POINTER(mirror), text
            elif "*" in text or "kbn_stream_t" in text:
                assert ctype is C.c_void_p, text
            else:
                assert text.startswith("int ") and ctype is C.c_int, text
        declared = _struct_fields(record)
        assert [(n, base[t] * k if k > 1 else base[t]) for n, t, k in declared] == [(n, t) for n, t in mirror._fields_]
        assert C.sizeof(mirror) == size
    assert kb.ops._SEQUENCE_FRAME_RECORD.size == 48 and kb.ops._PACKED_SEQUENCE_FRAME_RECORD.size == 64
    header = open(os.path.join(ROOT, "include", "kbnet_hip.h")).read()
    assert int(re.search(r"#define KBN_UNPACK_SEQUENCE_MAX_FRAMES (\d+)", header).group(1)) == kb._lib.KBN_UNPACK_SEQUENCE_MAX_FRAMES
    # the records and the rest of the parameter block stay inside the bound csrc/unpack_train.hip asserts
    assert kb._lib.KBN_UNPACK_SEQUENCE_MAX_FRAMES * 64 + 6 * 8 + 5 * 4 <= 3584
    assert kb._lib.KBN_UNPACK_SEQUENCE_MAX_FRAMES < kb._lib.KBN_UNPACK_TRAIN_MAX_FRAMES
    assert lib.kbn_version() == kb._lib.ABI_VERSION == 11


# host buffers stand in for device memory: every call below is refused before anything is launched, so no pointer is followed
_IMAGES = (C.c_ubyte * 4096)()
_DEPTHS = (C.c_ubyte * 4096)()
_OUT = (C.c_float * 4)()


def _aligned(buf):
    return (C.addressof(buf) + 15) & ~15


def _raw(frames=None, n=1, h=4, w=4, channels=3, bits=16, image_bytes=2048, depth_bytes=2048, null=()):
    """kbn_unpack_sequence_frames_forward on one 8 x 8 sample by default; `null`: argument names passed as NULL."""
    table = (kb._lib.SequenceFrame * max(1, n))()
    for rec, f in zip(table, frames or [dict()]):
        values = dict(image_offset=(0, 192, 384), depth_offset=0, height=8, width=8, y_start=0, x_start=0)
        values.update(f)
        rec.image_offset = (C.c_longlong * 3)(*values.pop("image_offset"))
        for k, v in values.items():
            setattr(rec, k, v)
    p = dict(images=_aligned(_IMAGES), depths=_aligned(_DEPTHS), frames=table, image0=C.addressof(_OUT), image1=C.addressof(_OUT),
             image2=C.addressof(_OUT), depth=C.addressof(_OUT))
    p.update({name: None for name in null})
    return kb._lib.load().kbn_unpack_sequence_frames_forward(p["images"], image_bytes, p["depths"], depth_bytes, p["frames"], n, h, w, channels,
                                                             bits, p["image0"], p["image1"], p["image2"], p["depth"], None)


def _packed(frames=None, n=1, h=4, w=4, channels=3, bits=16, image_bytes=2048, depth_bytes=2048, null=(), shift=0):
    """kbn_unpack_packed_sequence_frames_forward on one 8 x 8 sample of three 256-byte files by default."""
    table = (kb._lib.PackedSequenceFrame * max(1, n))()
    for rec, f in zip(table, frames or [dict()]):
        values = dict(image_offset=(0, 256, 512), image_bytes=(256, 256, 256), depth_offset=0, depth_bytes=256, height=8, width=8,
                      y_start=0, x_start=0)
        values.update(f)
        rec.image_offset = (C.c_longlong * 3)(*values.pop("image_offset"))
        rec.image_bytes = (C.c_uint * 3)(*values.pop("image_bytes"))
        for k, v in values.items():
            setattr(rec, k, v)
    p = dict(images=_aligned(_IMAGES) + shift, depths=_aligned(_DEPTHS), frames=table, image0=C.addressof(_OUT), image1=C.addressof(_OUT),
             image2=C.addressof(_OUT), depth=C.addressof(_OUT))
    p.update({name: None for name in null})
    return kb._lib.load().kbn_unpack_packed_sequence_frames_forward(p["images"], image_bytes, p["depths"], depth_bytes, p["frames"], n, h, w,
                                                                    channels, bits, p["image0"], p["image1"], p["image2"], p["depth"], None)


RAW_REFUSALS = {
    **{f"null {name}": (dict(null=(name,)), INVALID) for name in ("images", "depths", "frames", "image0", "image1", "image2", "depth")},
    "n = 0": (dict(n=0), INVALID),
    "n < 0": (dict(n=-3), INVALID),
    "height 0": (dict(h=0), INVALID),
    "width 0": (dict(w=0), INVALID),
    "frame height 0": (dict(frames=[dict(height=0)]), INVALID),
    "frame width 0": (dict(frames=[dict(width=0)]), INVALID),
    "crop below its frame": (dict(frames=[dict(y_start=5)]), INVALID),
    "crop right of its frame": (dict(frames=[dict(x_start=5)]), INVALID),
    "crop above its frame": (dict(frames=[dict(y_start=-1)]), INVALID),
    "crop left of its frame": (dict(frames=[dict(x_start=-1)]), INVALID),
    "crop wider than a frame, inside a triplet's width": (dict(w=9), INVALID),
    "previous before the buffer": (dict(frames=[dict(image_offset=(-1, 192, 384))]), INVALID),
    "current past the buffer": (dict(frames=[dict(image_offset=(0, 2048 - 191, 384))]), INVALID),
    "next past the buffer": (dict(frames=[dict(image_offset=(0, 192, 2048))]), INVALID),
    "depth past the buffer": (dict(frames=[dict(depth_offset=2048 - 126)]), INVALID),
    "odd 16-bit depth offset": (dict(frames=[dict(depth_offset=1)]), INVALID),
    "negative depth offset": (dict(frames=[dict(depth_offset=-2)]), INVALID),
    "the second record is wrong": (dict(n=2, frames=[dict(), dict(x_start=6)]), INVALID),
    "two channels": (dict(channels=2), UNSUPPORTED),
    "12-bit depth": (dict(bits=12), UNSUPPORTED),
}

PACKED_REFUSALS = {
    **{f"null {name}": (dict(null=(name,)), INVALID) for name in ("images", "depths", "frames", "image0", "depth")},
    "image1 without image2": (dict(null=("image2",)), INVALID),
    "image2 without image1": (dict(null=("image1",)), INVALID),
    "n = 0": (dict(n=0), INVALID),
    "height 0": (dict(h=0), INVALID),
    "width 0": (dict(w=0), INVALID),
    "misaligned buffer": (dict(shift=4), INVALID),
    "misaligned previous": (dict(frames=[dict(image_offset=(8, 256, 512))]), INVALID),
    "misaligned next": (dict(frames=[dict(image_offset=(0, 256, 520))]), INVALID),
    "misaligned depth": (dict(frames=[dict(depth_offset=4)]), INVALID),
    "negative offset": (dict(frames=[dict(image_offset=(0, -16, 512))]), INVALID),
    "crop leaves its frame": (dict(frames=[dict(x_start=5)]), INVALID),
    "frame width 0": (dict(frames=[dict(width=0)]), INVALID),
    "current too short for header and table": (dict(frames=[dict(image_bytes=(256, 40, 256))]), INVALID),
    "depth too short for header and table": (dict(frames=[dict(depth_bytes=36)]), INVALID),
    "next outside the buffer": (dict(frames=[dict(image_offset=(0, 256, 2048 - 128))]), INVALID),
    "depth outside the buffer": (dict(frames=[dict(depth_offset=2048 - 128)]), INVALID),
    "middle only still checks previous": (dict(null=("image1", "image2"), frames=[dict(image_offset=(4096, 256, 512))]), INVALID),
    "two channels": (dict(channels=2), UNSUPPORTED),
    "12-bit depth": (dict(bits=12), UNSUPPORTED),
    "wider than the LDS budget": (dict(frames=[dict(width=kb._lib.KBN_UNPACK_PACKED_MAX_RAW_WIDTH + 1)]), UNSUPPORTED),
}


@pytest.mark.parametrize("case", sorted(RAW_REFUSALS))
def test_unpack_sequence_frames_refuses_before_it_launches(case):
    arguments, code = RAW_REFUSALS[case]
    assert _raw(**arguments) == code


@pytest.mark.parametrize("case", sorted(PACKED_REFUSALS))
def test_unpack_packed_sequence_frames_refuses_before_it_launches(case):
    arguments, code = PACKED_REFUSALS[case]
    assert _packed(**arguments) == code


def test_ops_wrappers_name_the_wrong_frame_without_a_gpu():
    import torch
    images, depths = torch.zeros(2048, dtype=torch.uint8), torch.zeros(2048, dtype=torch.uint8)
    good = (0, 192, 384, 0, 8, 8, 0, 0)
    for frames, text in (([good, (0, 192, 384, 0, 8, 8, 5, 0)], "frame 1: the 4 x 4 crop at (5, 0) leaves the 8 x 8 frame"),
                         ([(0, 192, 2048, 0, 8, 8, 0, 0)], "frame 0: its next frame"),
                         ([good[:-1]], "frame 0: expected (previous_offset"),
                         ([good], "expected a CUDA/HIP tensor")):
        with pytest.raises(KbnError) as e:
            kb.ops.unpack_sequence_frames(images, depths, frames, (4, 4))
        assert text in str(e.value), str(e.value)
    good = (0, 256, 256, 256, 512, 256, 0, 256, 8, 8, 0, 0)
    for frames, text in (([good[:4] + (520,) + good[5:]], "frame 0: its packed next frame of 256 bytes at byte 520 is misaligned"),
                         ([good[:9] + (20000, 0, 0)], "a packed frame of 20000 columns is wider than the kernel takes"),
                         ([good], "expected a CUDA/HIP tensor")):
        with pytest.raises(KbnError) as e:
            kb.ops.unpack_packed_sequence_frames(images, depths, frames, (4, 4))
        assert text in str(e.value), str(e.value)
