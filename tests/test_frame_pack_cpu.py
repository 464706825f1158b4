"""CPU: the packed frame store's host side -- kbn_frame_encode / _decode / _check / _info and the argument checks of
kbn_unpack_packed_frames_forward -- against the NumPy codec of tests/frame_pack_oracle.py, which is written from DESIGN's text."""
import ctypes as C
import glob
import os
import re
import struct

import numpy as np
import pytest

import frame_pack_oracle as orc
import kbnet_amd as kb
from conftest import GOLDEN_DIR, ROOT

KbnError = kb._lib.KbnError
SIZES = [(1, 1), (15, 1), (16, 8), (17, 9), (129, 7), (129, 17)]      # W x H
CONTENTS = ["constant", "every_b", "wrap", "noise", "sparse"]


def from_residuals(w, h, c, bits, pick):
    """An image built segment by segment from its residuals: pick(serial number of the segment) -> the bit width b its largest
    field shall have; one sample of the segment gets a difference whose field is 2^(b-1) (or 2^b - 1 for the widest)."""
    a = np.zeros((h, w, c), dtype=np.int64)
    serial = 0
    for plane in range(c):
        for y in range(h):
            for k in range(-(-w // 16)):
                xs = list(range(16 * k, min(w, 16 * k + 16)))
                b = pick(serial)
                serial += 1
                z = 0 if b == 0 else ((1 << bits) - 1 if b == bits else 1 << (b - 1))
                d = z >> 1 if z % 2 == 0 else -(z >> 1) - 1
                left = y % 8 == 0
                if left:
                    a[y, xs[0], plane] = (37 * serial) % (1 << bits)
                for i, x in enumerate(xs):
                    if left and i == 0:
                        continue
                    pred = a[y, x - 1, plane] if left else a[y - 1, x, plane]
                    a[y, x, plane] = (pred + (d if i == len(xs) - 1 else 0)) % (1 << bits)
    return a


def make(content, w, h, c, bits, seed=0):
    g = np.random.Generator(np.random.Philox(seed + 1000 * w + h))
    top = (1 << bits) - 1
    if content == "constant":
        a = np.full((h, w, c), 77 if bits == 8 else 30000)
    elif content == "every_b":
        a = from_residuals(w, h, c, bits, lambda s: s % (bits + 1))
    elif content == "wrap":      # 0 <-> top and 0 -> half beside and above each other, in every order
        a = np.array([0, top, (top + 1) // 2])[g.integers(0, 3, size=(h, w, c))]
    elif content == "noise":
        a = g.integers(0, top + 1, size=(h, w, c))
    else:                        # sparse depth: 5 % of the samples set
        a = np.where(g.random((h, w, c)) < 0.05, g.integers(1, top + 1, size=(h, w, c)), 0)
    a = a.astype(np.uint16 if bits == 16 else np.uint8)
    return a[:, :, 0] if c == 1 else a


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_round_trips_and_byte_equal_encodings(size, c, bits):
    w, h = size
    for content in CONTENTS:
        a = make(content, w, h, c, bits)
        mine, theirs = kb.loader.encode_frame(a), orc.encode(a)
        assert mine == theirs, content                                          # the two encodings are byte-equal
        assert kb.loader.frame_info(mine) == (w, h, c, bits)
        kb.loader.check_frame(mine)
        got = kb.loader.decode_frame(mine)
        assert got.dtype == a.dtype and got.shape == a.shape and np.array_equal(got, a), content      # library -> library
        assert np.array_equal(orc.decode(mine), a), content                     # library -> NumPy
        assert np.array_equal(kb.loader.decode_frame(theirs), a), content       # NumPy -> library
        assert len(mine) <= kb._lib.load().kbn_frame_encode_bound(w, h, c, bits)


@pytest.mark.parametrize("bits", [8, 16])
def test_every_field_width_occurs(bits):
    """The `every_b` content does what it says at the largest size: header bytes 0 .. bits all occur, and the wrap content holds the
    differences the issue names."""
    data = orc.encode(make("every_b", 129, 17, 1, bits))
    start = (32 + 4 * (3 + 1) + 15) // 16 * 16
    table = struct.unpack("<4I", data[32:48])
    heads = b"".join(data[start + table[g]:start + table[g] + min(8, 17 - 8 * g) * 9] for g in range(3))
    assert set(heads) == set(range(bits + 1))
    a = make("wrap", 129, 17, 1, bits).astype(np.int64)
    top = (1 << bits) - 1
    pairs = set(zip(a[:, :-1].ravel(), a[:, 1:].ravel())) & set(zip(a[:-1].ravel(), a[1:].ravel()))
    assert {(0, top), (top, 0), (0, (top + 1) // 2)} <= pairs


def test_committed_version_1_files_decode():
    """Files written by the NumPy encoder when version 1 was fixed (tests/golden/gen_frames_v1_golden.py): the library must go on
    reading them."""
    names = sorted(glob.glob(os.path.join(GOLDEN_DIR, "frames_v1", "*.kbf")))
    assert len(names) == 2
    for name in names:
        with open(name, "rb") as f:
            data = f.read()
        want = np.load(name[:-4] + ".npy")
        kb.loader.check_frame(data)
        got = kb.loader.decode_frame(data)
        assert got.dtype == want.dtype and np.array_equal(got, want)
        assert np.array_equal(orc.decode(data), want)
        assert kb.loader.encode_frame(want) == data


# ----------------------------------------------------------------------------- files no encoder of ours writes
# Version 1 allows a header byte wider than its segment needs (up to `bits`), nonzero pad bits, and any b on a one-sample left-row
# segment.  The format, not the encoder, is the contract: whatever kbn_frame_check accepts decodes alike everywhere.
WIDTH_CHOICES = orc.WIDTH_CHOICES
noncanonical = orc.hand_made


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_hand_made_files_decode_like_the_oracle(size, c, bits):
    w, h = size
    for choice in WIDTH_CHOICES:
        data, a = noncanonical(choice, w, h, c, bits)
        kb.loader.check_frame(data)                                        # the library accepts it
        assert kb.loader.frame_info(data) == (w, h, c, bits)
        got = kb.loader.decode_frame(data)
        assert got.dtype == a.dtype and got.shape == a.shape
        assert np.array_equal(got, orc.decode(data)), choice               # library == NumPy
        assert np.array_equal(got, a), choice                              # == the samples it was built from (build_random: the oracle's)
        assert data != kb.loader.encode_frame(a), choice                   # and it is not what the encoder writes
        segments = orc.segments_of(data)                                   # read back from the bytes
        assert all(b >= needed for b, needed, _ in segments)
        wide, padded = sum(b > needed for b, needed, _ in segments), sum(pad != 0 for _, _, pad in segments)
        # every file of the first three choices has a header byte above its need (their samples leave room: noise / 16); a file of
        # build_random is non-canonical by a wide byte or by a pad bit (its random fields may happen to need every b)
        assert wide > 0 if choice != "build_random" else wide + padded > 0, choice
        # ... and a nonzero pad bit where the choice sets them and the file has any: every b = bits makes whole bytes, and so does
        # a file whose segments are all one-sample left-row segments (`bits` bits each)
        has_pad_bits = any((b * (n if up else n - 1)) % 8 for b, n, up in _segment_shapes(data))
        if choice in ("needed_plus_1", "random") and has_pad_bits:
            assert padded > 0, choice


def _segment_shapes(data):
    """(b, samples, is an up row) of every segment of a file, in file order."""
    w, h, c, _ = kb.loader.frame_info(data)
    heads = iter(b for b, _, _ in orc.segments_of(data))
    for group in range(-(-h // 8)):
        for _ in range(c):
            for row in range(min(8, h - 8 * group)):
                for k in range(-(-w // 16)):
                    yield next(heads), min(16, w - 16 * k), row != 0


def test_build_without_choices_is_the_encoder():
    for w, h in SIZES:
        a = make("every_b", w, h, 3, 8)
        assert orc.build(a) == orc.encode(a) == kb.loader.encode_frame(a)
        assert all(b == needed and pad == 0 for b, needed, pad in orc.segments_of(orc.encode(a)))


# ----------------------------------------------------------------------------- kbn_frame_check
def _valid():
    """A 3-plane 8-bit 37 x 19 file (three groups, a short last one; three segments a row, a short last one) and where its parts are."""
    a = make("noise", 37, 19, 3, 8, seed=5) // 8 + make("every_b", 37, 19, 3, 8)
    data = bytearray(orc.encode(a.astype(np.uint8)))
    entries = 3 * 3 + 1
    start = (32 + 4 * entries + 15) // 16 * 16
    table = list(struct.unpack(f"<{entries}I", data[32:32 + 4 * entries]))
    return data, start, table


def _with_table(data, table, payload_bytes=None):
    out = bytearray(data)
    out[32:32 + 4 * len(table)] = struct.pack(f"<{len(table)}I", *table)
    if payload_bytes is not None:
        out[24:32] = struct.pack("<Q", payload_bytes)
    return out


def _damaged():
    data, start, table = _valid()
    cases = {}

    def put(name, at, fmt, value):
        d = bytearray(data)
        d[at:at + struct.calcsize(fmt)] = struct.pack(fmt, value)
        cases[name] = d

    put("wrong magic", 6, "<B", ord("2"))
    put("rows per group 4", 20, "<H", 4)
    put("samples per segment 8", 22, "<H", 8)
    put("bits 12", 18, "<H", 12)
    put("channels 2", 16, "<H", 2)
    put("width 0", 8, "<I", 0)
    cases["truncated by a byte"] = data[:-1]
    cases["truncated inside the table"] = data[:40]
    cases["only a header"] = data[:32]
    swapped = list(table)
    swapped[3], swapped[4] = swapped[4], swapped[3]
    cases["table not monotone"] = _with_table(data, swapped)
    past = list(table)
    past[-2] = table[-1] + 5
    cases["table past the end"] = _with_table(data, past)
    first = list(table)
    first[0] = 1
    cases["table does not start at 0"] = _with_table(data, first)
    d = bytearray(data)
    d[start + table[4] + 2] = 9
    cases["a header byte of bits + 1"] = d
    # the payload of (group 1, plane 1) one byte short: its last byte removed, every later offset and payload_bytes moved with it
    cut = start + table[5] - 1
    cases["a payload one byte short"] = _with_table(data[:cut] + data[cut + 1:], table[:5] + [t - 1 for t in table[5:]], table[-1] - 1)
    cases["a payload one byte long"] = _with_table(data[:cut + 1] + b"\0" + data[cut + 1:], table[:5] + [t + 1 for t in table[5:]], table[-1] + 1)
    cases["payload_bytes above the file's"] = _with_table(data, table, table[-1] + 1)
    cases["a byte behind the payload"] = data + b"\0"
    d = bytearray(data)
    d[start - 1] = 1
    cases["padding not zero"] = d
    # the payload cut to 10 bytes, payload_bytes and every entry saying so, but entry 1 left far above: plane 0 claims room for its
    # header bytes that the file does not have (check_file reads them before it sees entry 2 fall back)
    cases["a short payload under an inner entry above payload_bytes"] = _with_table(data[:start + 10], [0, 1000] + [10] * (len(table) - 2), 10)
    return cases


DAMAGED = _damaged()


def test_check_accepts_the_undamaged_file():
    data, _, table = _valid()
    kb.loader.check_frame(bytes(data))
    assert table[0] == 0 and table[-1] == len(data) - (32 + 4 * 10 + 15) // 16 * 16
    assert (32 + 4 * 10) % 16 != 0      # so `padding not zero` has a padding byte to damage


@pytest.mark.parametrize("name", sorted(DAMAGED))
def test_check_refuses(name):
    data = bytes(DAMAGED[name])
    lib = kb._lib.load()
    assert lib.kbn_frame_check(data, len(data)) in (kb._lib.KBN_ERR_INVALID_ARGUMENT, kb._lib.KBN_ERR_UNSUPPORTED)
    with pytest.raises(KbnError):
        kb.loader.check_frame(data)
    with pytest.raises(KbnError):
        kb.loader.decode_frame(data)      # the host decoder checks first


def test_host_functions_refuse_bad_arguments():
    lib = kb._lib.load()
    a = make("noise", 17, 9, 3, 8)
    buf, n = (C.c_ubyte * 4096)(), C.c_size_t()
    ptr = a.ctypes.data_as(C.c_void_p)
    assert lib.kbn_frame_encode(ptr, 17, 9, 3, 8, buf, 10, C.byref(n)) == kb._lib.KBN_ERR_WORKSPACE
    assert lib.kbn_frame_encode(ptr, 17, 9, 2, 8, buf, 4096, C.byref(n)) == kb._lib.KBN_ERR_UNSUPPORTED
    assert lib.kbn_frame_encode(ptr, 17, 9, 3, 12, buf, 4096, C.byref(n)) == kb._lib.KBN_ERR_UNSUPPORTED
    assert lib.kbn_frame_encode(ptr, 0, 9, 3, 8, buf, 4096, C.byref(n)) == kb._lib.KBN_ERR_INVALID_ARGUMENT
    assert lib.kbn_frame_encode(None, 17, 9, 3, 8, buf, 4096, C.byref(n)) == kb._lib.KBN_ERR_INVALID_ARGUMENT
    assert lib.kbn_frame_encode_bound(17, 9, 2, 8) == 0 and lib.kbn_frame_encode_bound(17, 0, 3, 8) == 0
    data = kb.loader.encode_frame(a)
    out = np.empty(17 * 9 * 3 - 1, np.uint8)
    assert lib.kbn_frame_decode(data, len(data), out.ctypes.data_as(C.c_void_p), out.nbytes) == kb._lib.KBN_ERR_INVALID_ARGUMENT
    with pytest.raises(KbnError):
        kb.loader.encode_frame(np.zeros((4, 4, 2), np.uint8))
    with pytest.raises(KbnError):
        kb.loader.encode_frame(np.zeros((4, 4), np.float32))
    assert kb.loader.frame_info(data[:32]) == (17, 9, 3, 8)      # the header alone is enough
    with pytest.raises(KbnError):
        kb.loader.frame_info(data[:31])


# ------------------------------------------- kbn_unpack_packed_frames_forward: its checks run before any launch
def _entry(frames, n=None, h=16, w=24, c=3, dbits=16, image_bytes=1 << 20, depth_bytes=1 << 20, images=0x10000, depths=0x20000,
           image0=0x30000, image1=0x40000, image2=0x50000, depth=0x60000):
    """The entry point with made-up device addresses: every call here must be refused before anything would be launched."""
    lib = kb._lib.load()
    table = (kb._lib.PackedFrame * max(1, len(frames)))(*[kb._lib.PackedFrame(*f) for f in frames])
    return lib.kbn_unpack_packed_frames_forward(images, image_bytes, depths, depth_bytes, table, len(frames) if n is None else n, h, w, c, dbits,
                                                image0, image1, image2, depth, None)


GOOD = (0, 4096, 8192, 2048, 24, 120, 3, 5)      # image offset, depth offset, their sizes, H, 3 W (W = 40), y_start, x_start


def _record(**change):
    names = ("image_offset", "depth_offset", "image_bytes", "depth_bytes", "height", "raw_width", "y_start", "x_start")
    return tuple(change.get(name, value) for name, value in zip(names, GOOD))


@pytest.mark.parametrize("change", [
    dict(y_start=-1), dict(y_start=9), dict(x_start=-1), dict(x_start=17),                 # the crop past each of the four sides
    dict(raw_width=121), dict(raw_width=0), dict(height=0),
    dict(image_offset=-16), dict(image_offset=8), dict(depth_offset=4100), dict(image_offset=(1 << 20) - 4096),      # records outside their buffers
    dict(depth_offset=(1 << 20) - 16), dict(image_bytes=(1 << 20) + 16), dict(image_bytes=40), dict(depth_bytes=32),
], ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()))
def test_entry_point_refuses_bad_records(change):
    assert _entry([_record(**change)]) == kb._lib.KBN_ERR_INVALID_ARGUMENT
    assert _entry([GOOD, _record(**change)]) == kb._lib.KBN_ERR_INVALID_ARGUMENT      # every record is checked, not only the first


def test_entry_point_refuses_bad_arguments():
    bad, unsupported = kb._lib.KBN_ERR_INVALID_ARGUMENT, kb._lib.KBN_ERR_UNSUPPORTED
    assert _entry([GOOD], n=0) == bad
    assert _entry([GOOD], h=0) == bad and _entry([GOOD], w=0) == bad
    for name in ("images", "depths", "image0", "depth"):      # image1 and image2 are the only pointers that may be null
        assert _entry([GOOD], **{name: None}) == bad
    assert _entry([GOOD], images=0x10008) == bad              # the buffers are 16-byte aligned
    assert _entry([GOOD], c=2) == unsupported and _entry([GOOD], dbits=12) == unsupported
    cap = kb._lib.KBN_UNPACK_PACKED_MAX_RAW_WIDTH
    assert cap % 3 != 0
    wide = _record(raw_width=cap // 3 * 3 + 3)
    assert _entry([wide]) == unsupported                      # the LDS budget: stated in the header, refused on the host
    lib = kb._lib.load()
    assert lib.kbn_unpack_packed_frames_forward(0x10000, 1 << 20, 0x20000, 1 << 20, None, 1, 16, 24, 3, 16, 0x30000, None, None, 0x60000, None) == bad


def test_op_refuses_before_it_launches():
    import torch
    buf = torch.zeros(4096, dtype=torch.uint8)
    good = (0, 512, 0, 512, 24, 40, 0, 0)
    for frames, shape in (([good], (16, 24)),):
        with pytest.raises(KbnError, match="CUDA/HIP"):
            kb.ops.unpack_packed_frames(buf, buf, frames, shape)
    for frames, shape in (([], (16, 24)), ([good], (0, 24)), ([(0, 512, 0, 512, 24, 40, 9, 0)], (16, 24)), ([(8, 512, 0, 512, 24, 40, 0, 0)], (16, 24)),
                          ([(0, 8192, 0, 512, 24, 40, 0, 0)], (16, 24)), ([(0, 512, 0, 512, 24, 6000, 0, 0)], (16, 24)), ([good[:6]], (16, 24))):
        with pytest.raises(KbnError):
            kb.ops.unpack_packed_frames(buf, buf, frames, shape)
    with pytest.raises(KbnError):
        kb.ops.unpack_packed_frames(buf, buf, [good], (16, 24), channels=2)


# ------------------------------------------------------------------------------ the power of these comparisons
def _cases_for_power():
    for w, h in SIZES:
        for c, bits in ((1, 8), (3, 8), (1, 16)):
            for content in ("every_b", "noise", "wrap"):
                yield make(content, w, h, c, bits)


def test_the_comparisons_catch_planted_mistakes():
    """Each mistake of frame_pack_oracle.MISTAKES, planted into the NumPy decoder, makes at least one of the round-trip cases above
    (or, for the third's offset, the slice comparison the GPU test makes at W = 43) come out unequal; the unplanted decoder passes all."""
    cases = list(_cases_for_power())
    files = [orc.encode(a) for a in cases]
    assert all(np.array_equal(orc.decode(f), a) for f, a in zip(files, cases))
    for mistake in orc.MISTAKES:
        if mistake == "third_rounded":
            continue
        caught = [not np.array_equal(orc.decode(f, mistake), a) for f, a in zip(files, cases)]
        assert any(caught), mistake
    # ... and each is caught on a hand-made file too: the comparisons of test_hand_made_files_decode_like_the_oracle have the same power
    made = [noncanonical(choice, w, h, c, bits) for w, h in SIZES[2:] for c, bits in ((1, 8), (3, 8), (1, 16)) for choice in WIDTH_CHOICES]
    assert all(np.array_equal(orc.decode(f), a) for f, a in made)
    for mistake in orc.MISTAKES:
        if mistake != "third_rounded":
            assert any(not np.array_equal(orc.decode(f, mistake), a) for f, a in made), mistake
    g = np.random.Generator(np.random.Philox(3))
    triplet = g.integers(0, 256, size=(25, 3 * 43, 3), dtype=np.uint8)
    depth = g.integers(0, 65536, size=(25, 43), dtype=np.uint16)
    tf, df = orc.encode(triplet), orc.encode(depth)
    want = [np.ascontiguousarray(triplet[2:18, t * 43 + 7:t * 43 + 31].transpose(2, 0, 1)).astype(np.float32) for t in (1, 0, 2)]
    got = orc.unpack(tf, df, 2, 7, 16, 24)
    assert all(np.array_equal(a, b) for a, b in zip(got[:3], want))
    assert np.array_equal(got[3][0], depth[2:18, 7:31].astype(np.float32) / 256)
    planted = orc.unpack(tf, df, 2, 7, 16, 24, mistake="third_rounded")
    assert not np.array_equal(planted[0], want[0]) and not np.array_equal(planted[2], want[2])
    tf, df = orc.build(triplet, lambda *a: a[5]), orc.build(depth // 16, lambda *a: a[4] + 1, lambda *a: 0xff)      # hand-made files of the same frame
    assert tf != orc.encode(triplet) and all(np.array_equal(a, b) for a, b in zip(orc.unpack(tf, df, 2, 7, 16, 24)[:3], want))
    planted = orc.unpack(tf, df, 2, 7, 16, 24, mistake="third_rounded")
    assert not np.array_equal(planted[0], want[0]) and not np.array_equal(planted[2], want[2])


# ------------------------------------------------------------------------------ files and plumbing
def test_pack_frames_reproduces_the_png_pixels(tmp_path):
    pngs = sorted(glob.glob(os.path.join(GOLDEN_DIR, "io", "*.png")))
    assert len(pngs) >= 10
    dst = [str(tmp_path / "deep" / (os.path.basename(p)[:-4] + ".kbf")) for p in pngs]
    before, after = kb.loader.pack_frames(pngs, dst, workers=3)
    assert before == sum(os.path.getsize(p) for p in pngs) and after == sum(os.path.getsize(p) for p in dst)
    assert sorted(os.listdir(tmp_path / "deep")) == sorted(os.path.basename(p) for p in dst)      # no temporary file left
    for png, packed in zip(pngs, dst):
        with open(png, "rb") as f:
            want = kb.loader.decode_png(f.read())
        with open(packed, "rb") as f:
            data = f.read()
        assert kb.loader.is_packed_frame(data[:8])
        got = kb.loader.decode_frame(data)
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)
    with pytest.raises(KbnError):
        kb.loader.pack_frames(pngs, dst[:-1])


def test_header_library_and_binding_agree():
    with open(os.path.join(ROOT, "include", "kbnet_hip.h")) as f:
        header = f.read()
    lib = kb._lib.load()
    for name in ("kbn_frame_info", "kbn_frame_encode_bound", "kbn_frame_encode", "kbn_frame_decode", "kbn_frame_check",
                 "kbn_unpack_packed_frames_forward"):
        assert re.search(r"\b" + name + r"\s*\(", header) and name in kb._lib.SIGNATURES and hasattr(lib, name)
    assert int(re.search(r"#define KBN_UNPACK_PACKED_MAX_RAW_WIDTH (\d+)", header).group(1)) == kb._lib.KBN_UNPACK_PACKED_MAX_RAW_WIDTH
    assert C.sizeof(kb._lib.PackedFrame) == 40 and kb.ops._PACKED_FRAME_RECORD.size == 40
    body = re.sub(r"/\*.*?\*/", "", header.split("typedef struct kbn_packed_frame {")[1].split("}")[0], flags=re.S)
    assert [n for n, _ in kb._lib.PackedFrame._fields_] == re.findall(r"(\w+)\s*[,;]", body)
    assert kb._lib.ABI_VERSION == 11 and lib.kbn_version() == 11      # symbols were only added


def test_pack_dataset_tool_writes_files_and_lists(tmp_path):
    """tools/pack_dataset.py: reference-style lists in, packed files and line-for-line lists out, the two totals printed."""
    import subprocess
    import sys
    images = [os.path.join(GOLDEN_DIR, "io", f"triplet_{i}.png") for i in (0, 1, 0)]
    depths = [os.path.join(GOLDEN_DIR, "io", f"depth_{i}.png") for i in (0, 1, 0)]
    kb.loader.write_paths(str(tmp_path / "image.txt"), images)
    kb.loader.write_paths(str(tmp_path / "sparse_depth.txt"), depths)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pack_dataset.py"), "--paths", str(tmp_path / "image.txt"),
                          str(tmp_path / "sparse_depth.txt"), "--output_root", str(tmp_path / "packed"), "--workers", "2"],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-600:]
    before = sum(os.path.getsize(p) for p in images[:2] + depths[:2])
    assert res.stdout.startswith(f"4 files: {before} bytes of PNG -> ")
    for name, sources in (("image.txt", images), ("sparse_depth.txt", depths)):
        packed = kb.loader.read_paths(str(tmp_path / "packed" / "lists" / name))
        assert len(packed) == 3 and packed[0] == packed[2] != packed[1] and all(p.endswith(".kbf") for p in packed)
        for src, dst in zip(sources, packed):
            with open(src, "rb") as f, open(dst, "rb") as g:
                assert np.array_equal(kb.loader.decode_frame(g.read()), kb.loader.decode_png(f.read()))
