"""No GPU: the host side of packed outputs and packed ground truth -- the single-file readers on packed files,
tools/unpack_dataset.py, the device encoder's argument checks through the binding, the formats OutputWriter and run refuse --
and the POWER TEST of tests/test_pack_frames_gpu.py: encoders that are wrong and still round-trip, or nearly right, and the byte
comparison that notices each."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import frame_pack_oracle as oracle
import kbnet_amd as kb
import pack_cases as pc
from conftest import GOLDEN_DIR, ROOT

KbnError = kb._lib.KbnError
IO = os.path.join(GOLDEN_DIR, "io")


def read(path):
    with open(path, "rb") as f:
        return f.read()


def packed_copy(tmp_path, name):
    """A packed copy of tests/golden/io/<name>, named .png on purpose: the readers go by the magic, not the name."""
    dst = os.path.join(str(tmp_path), "packed_" + name)
    with open(dst, "wb") as f:
        f.write(kb.loader.encode_frame(kb.loader.decode_png(read(os.path.join(IO, name)))))
    assert kb.loader.is_packed_frame(read(dst))
    return dst


# ------------------------------------------------------------------------------------------------ the single-file readers
@pytest.mark.parametrize("name", ["depth_0.png", "depth_1.png", "saved_depth.png"])
def test_load_depth_reads_packed(tmp_path, name):
    src, dst = os.path.join(IO, name), packed_copy(tmp_path, name)
    for data_format in ("HW", "CHW", "HWC"):
        want, got = kb.loader.load_depth(src, data_format), kb.loader.load_depth(dst, data_format)
        assert want.dtype == got.dtype and np.array_equal(want, got)
        for a, b in zip(kb.loader.load_depth_with_validity_map(src, data_format), kb.loader.load_depth_with_validity_map(dst, data_format)):
            assert a.dtype == b.dtype and np.array_equal(a, b)


@pytest.mark.parametrize("name", ["triplet_0.png", "gray8.png", "rgba.png", "palette.png"])
def test_load_image_reads_packed(tmp_path, name):
    src, dst = os.path.join(IO, name), packed_copy(tmp_path, name)
    for normalize in (True, False):
        for data_format in ("HWC", "CHW"):
            want, got = kb.loader.load_image(src, normalize, data_format), kb.loader.load_image(dst, normalize, data_format)
            assert want.dtype == got.dtype and np.array_equal(want, got)


@pytest.mark.parametrize("name", ["triplet_0.png", "triplet_2.png"])
def test_load_image_triplet_reads_packed(tmp_path, name):
    src, dst = os.path.join(IO, name), packed_copy(tmp_path, name)
    for a, b in zip(kb.loader.load_image_triplet(src), kb.loader.load_image_triplet(dst)):
        assert a.dtype == b.dtype and np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ tools/unpack_dataset.py
def test_unpack_dataset_inverts_pack_dataset(tmp_path):
    """PNG -> packed (tools/pack_dataset.py) -> PNG (tools/unpack_dataset.py): the pixels of 8-bit RGB, 8-bit gray and 16-bit gray
    files come back, and the new path lists name the new files line for line."""
    names = ["triplet_0.png", "depth_0.png", "gray8.png", "depth_1.png", "triplet_0.png"]      # one file listed twice
    lists = os.path.join(str(tmp_path), "files.txt")
    kb.loader.write_paths(lists, [os.path.join(IO, n) for n in names])
    packed_root, png_root = os.path.join(str(tmp_path), "packed"), os.path.join(str(tmp_path), "png")
    for tool, src_list, root in (("pack_dataset.py", lists, packed_root),
                                 ("unpack_dataset.py", os.path.join(packed_root, "lists", "files.txt"), png_root)):
        done = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "--paths", src_list, "--output_root", root,
                               "--workers", "2"], capture_output=True, text=True)
        assert done.returncode == 0, done.stderr
    packed_paths = kb.loader.read_paths(os.path.join(packed_root, "lists", "files.txt"))
    png_paths = kb.loader.read_paths(os.path.join(png_root, "lists", "files.txt"))
    assert len(png_paths) == len(names) and png_paths[0] == png_paths[4]
    for name, packed, png in zip(names, packed_paths, png_paths):
        assert packed.endswith(".kbf") and png.endswith(".png") and png.startswith(png_root)
        assert os.path.basename(png) == name
        want = kb.loader.decode_png(read(os.path.join(IO, name)))
        got = kb.loader.decode_png(read(png))
        assert want.dtype == got.dtype and want.shape == got.shape and np.array_equal(want, got)
        assert kb.loader.png_info(read(png)) == kb.loader.png_info(read(os.path.join(IO, name)))


def test_unpack_frames_refuses_other_formats_by_name(tmp_path):
    for samples, what in ((np.zeros((4, 5, 4), np.uint8), "4 channels of 8 bits"), (np.zeros((4, 5, 3), np.uint16), "3 channels of 16 bits")):
        src = os.path.join(str(tmp_path), "odd.kbf")
        with open(src, "wb") as f:
            f.write(kb.loader.encode_frame(samples))
        with pytest.raises(KbnError, match="odd.kbf.*" + what):
            kb.loader.unpack_frames([src], [os.path.join(str(tmp_path), "odd.png")])
    with pytest.raises(KbnError, match="depth_0.png is not a packed frame"):
        kb.loader.unpack_frames([os.path.join(IO, "depth_0.png")], [os.path.join(str(tmp_path), "x.png")])


# ------------------------------------------------------------------------------------------------ the entry points' argument checks
def test_pack_frames_argument_checks():
    """kbn_pack_frames_forward checks everything before it launches anything, so the statuses can be read without a GPU (the
    pointers are never followed).  NULL pointers are tests/test_host_cpu.py's business."""
    lib = kb._lib.load()
    inv, unsup, work = kb._lib.KBN_ERR_INVALID_ARGUMENT, kb._lib.KBN_ERR_UNSUPPORTED, kb._lib.KBN_ERR_WORKSPACE
    cap = kb._lib.KBN_PACK_FRAMES_MAX_WIDTH
    assert cap >= 4096
    for c in (1, 3, 4):
        for bits in (8, 16):
            bound = lib.kbn_frame_encode_bound(33, 9, c, bits)
            assert lib.kbn_pack_frames_stride(33, 9, c, bits) == (bound + 15) // 16 * 16
            assert lib.kbn_pack_frames_workspace_bytes(3, 33, 9, c, bits) > 0
    assert lib.kbn_pack_frames_stride(cap, 8, 1, 8) > 0 and lib.kbn_pack_frames_stride(cap + 1, 8, 1, 8) == 0
    assert lib.kbn_pack_frames_stride(33, 9, 2, 8) == 0 and lib.kbn_pack_frames_stride(33, 9, 1, 12) == 0
    assert lib.kbn_pack_frames_stride(0, 9, 1, 8) == 0 and lib.kbn_pack_frames_stride(16384, 1 << 20, 4, 16) == 0      # past 4 GiB
    assert lib.kbn_pack_frames_workspace_bytes(0, 33, 9, 1, 8) == 0 and lib.kbn_pack_frames_workspace_bytes(1, cap + 1, 9, 1, 8) == 0

    stride, need = lib.kbn_pack_frames_stride(33, 9, 1, 16), lib.kbn_pack_frames_workspace_bytes(2, 33, 9, 1, 16)
    good = dict(samples=0x1000, n=2, width=33, height=9, channels=1, bits=16, out=0x2000, out_stride=stride, out_bytes=0x3000,
                workspace=0x4000, workspace_bytes=need)

    def status(**change):
        a = dict(good, **change)
        return lib.kbn_pack_frames_forward(a["samples"], a["n"], a["width"], a["height"], a["channels"], a["bits"], a["out"],
                                           a["out_stride"], a["out_bytes"], a["workspace"], a["workspace_bytes"], None)

    for change in (dict(n=0), dict(width=0), dict(height=-1), dict(out=0x2008), dict(out_stride=stride - 16), dict(out_stride=stride + 8),
                   dict(samples=0x1001), dict(samples=None), dict(out=None), dict(out_bytes=None), dict(workspace=None)):
        assert status(**change) == inv, change
    for change in (dict(channels=2), dict(bits=12), dict(width=cap + 1), dict(width=16384, height=1 << 20, channels=4)):
        assert status(**change) == unsup, change
    assert status(workspace_bytes=need - 1) == work
    assert status(workspace_bytes=0) == work


def test_unknown_formats_are_refused_by_name(tmp_path):
    """Before anything touches the device or the disk."""
    root = os.path.join(str(tmp_path), "out")
    with pytest.raises(KbnError, match="file_format 'jpeg'"):
        kb.loader.OutputWriter(root, file_format="jpeg")
    assert not os.path.exists(root)
    with pytest.raises(KbnError, match="output_format 'kbf'"):
        kb.inference.run_with_format("missing_images.txt", "missing_depths.txt", "missing_k.txt", checkpoint_path=root, output_format="kbf")
    assert not os.path.exists(root)
    with pytest.raises(TypeError):      # run() itself keeps the signature of DESIGN 8n
        kb.inference.run("missing_images.txt", "missing_depths.txt", "missing_k.txt", checkpoint_path=root, output_format="packed")
    assert not os.path.exists(root)
    assert kb.loader.packed_filename("0000000003.png") == "0000000003.kbf"


def test_run_with_format_is_run_plus_one_keyword():
    """run() delegates with **locals(): the two parameter lists must agree name for name, kind for kind, default for default."""
    import inspect
    run, full = (inspect.signature(f).parameters for f in (kb.inference.run, kb.inference.run_with_format))
    extra = full["output_format"]
    assert extra.kind is inspect.Parameter.KEYWORD_ONLY and extra.default == "png"
    rest = [p for name, p in full.items() if name != "output_format"]
    assert [(p.name, p.kind, p.default) for p in rest] == [(p.name, p.kind, p.default) for p in run.values()]


# ------------------------------------------------------------------------------------------------ the power test
MISTAKES = ("wide_b", "up_from_left", "msb_first")


def _pack_fields_msb(fields):
    """[(value, width)] -> bytes with the fields' bits in stream order, MOST significant bit of every byte first."""
    bits = [(value >> i) & 1 for value, width in fields for i in range(width - 1, -1, -1)]
    bits += [0] * (-len(bits) % 8)
    return bytes(sum(bit << (7 - i) for i, bit in enumerate(bits[at:at + 8])) for at in range(0, len(bits), 8))


def encode_with(samples, mistake=None):
    """tests/frame_pack_oracle.py's encoder with one mistake planted:
      wide_b        the first segment of every (group, plane) that has residuals and a b below `bits` is stored with b + 1 bits a
                    field where b suffices; table and sizes follow -- a VALID file that decodes to the samples
      up_from_left  an up row's residuals are taken from the left neighbour
      msb_first     fields packed MSB first"""
    a = np.asarray(samples)
    bits = 8 * a.dtype.itemsize
    if a.ndim == 2:
        a = a[:, :, None]
    h, w, c = a.shape
    groups, segments, start = oracle._layout(w, h, c)
    a = a.astype(np.int64)
    pack_fields = _pack_fields_msb if mistake == "msb_first" else oracle._pack_fields
    table, payload = [], b""
    for g in range(groups):
        for plane in range(c):
            table.append(len(payload))
            heads, data, widened = b"", b"", False
            for y in range(g * oracle.ROWS, min(h, (g + 1) * oracle.ROWS)):
                for k in range(segments):
                    xs = range(k * oracle.SEG, min(w, (k + 1) * oracle.SEG))
                    if y == g * oracle.ROWS or mistake == "up_from_left":
                        z = [oracle._zigzag(oracle._signed(int(a[y, x, plane] - a[y, x - 1, plane]), bits)) for x in xs[1:]]
                        if y == g * oracle.ROWS:
                            raw = [(int(a[y, xs[0], plane]), bits)]
                        else:
                            z, raw = [oracle._zigzag(oracle._signed(int(a[y, xs[0], plane] - a[y - 1, xs[0], plane]), bits))] + z, []
                    else:
                        z = [oracle._zigzag(oracle._signed(int(a[y, x, plane] - a[y - 1, x, plane]), bits)) for x in xs]
                        raw = []
                    b = max(z).bit_length() if z else 0
                    if mistake == "wide_b" and not widened and z and b < bits:
                        b, widened = b + 1, True
                    heads += bytes([b])
                    data += pack_fields(raw + [(v, b) for v in z])
            payload += heads + data
    table.append(len(payload))
    header = oracle.MAGIC + struct.pack("<IIHHHHQ", w, h, c, bits, oracle.ROWS, oracle.SEG, len(payload))
    head = header + struct.pack(f"<{len(table)}I", *table)
    return head + b"\0" * (start - len(head)) + payload


POWER_FRAMES = [pc.make("noise", 17, 33, 3, 8, seed=1) // 16 + 100, pc.make("sparse", 9, 31, 1, 16, seed=2)[:, :, 0], pc.make("ramp", 17, 33, 1, 8)[:, :, 0]]


@pytest.mark.parametrize("frame", range(len(POWER_FRAMES)))
def test_power_of_the_byte_comparison(frame):
    """Why tests/test_pack_frames_gpu.py compares BYTES.  An encoder that spends b + 1 bits where b suffice writes a file that
    check_frame accepts and decode_frame turns back into the samples -- a round-trip test passes it -- yet its bytes are not the
    host encoder's.  Two encoders that are plainly wrong (an up row predicted from the left, fields packed MSB first) are noticed
    by the same comparison; and the unmistaken copy of the planted encoder IS byte-equal, so the comparison blames the mistakes."""
    samples = POWER_FRAMES[frame]
    want = kb.loader.encode_frame(samples)
    assert encode_with(samples) == want == oracle.encode(samples)
    wasteful = encode_with(samples, "wide_b")
    kb.loader.check_frame(wasteful)                                              # a valid file ...
    assert np.array_equal(kb.loader.decode_frame(wasteful), samples)             # ... that round-trips ...
    assert np.array_equal(oracle.decode(wasteful), samples)
    assert wasteful != want and len(wasteful) > len(want)                        # ... and is not the encoder's
    for mistake in ("up_from_left", "msb_first"):
        wrong = encode_with(samples, mistake)
        assert wrong != want, mistake
        assert pc.first_difference(wrong, want) >= 24, mistake                   # magic, sizes and format are right; what follows is not
