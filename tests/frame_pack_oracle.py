"""The packed frame format, version 1, in NumPy and plain Python: an encoder and a decoder written from the text of DESIGN 8t, not
from csrc/frame_pack.hip.  Slow and obvious on purpose; tests/test_frame_pack_cpu.py and tests/test_frame_pack_gpu.py compare the
library's codec and the device decoder with it.

`decode(data, mistake=...)` and `unpack(..., mistake=...)` can plant one of MISTAKES into the decoder: the power test asserts that
the comparisons of the suite notice each of them."""
import struct

import numpy as np

MAGIC = b"KBNFRM1\0"
ROWS, SEG = 8, 16
MISTAKES = ("msb_first", "zigzag_sign", "no_group_restart", "left_as_up", "short_segment_16", "third_rounded")


def _layout(w, h, c):
    groups = -(-h // ROWS)
    start = (32 + 4 * (groups * c + 1) + 15) // 16 * 16
    return groups, -(-w // SEG), start


def _zigzag(d):
    return 2 * d if d >= 0 else -2 * d - 1


def _signed(diff, bits):
    """The representative of diff mod 2^bits in [-2^(bits-1), 2^(bits-1) - 1]."""
    diff %= 1 << bits
    return diff - (1 << bits) if diff >= 1 << (bits - 1) else diff


def _pack_fields(fields):
    """[(value, width)] -> bytes: LSB first into a little-endian byte stream, zero bits up to a whole byte."""
    acc, n = 0, 0
    for value, width in fields:
        acc |= value << n
        n += width
    return acc.to_bytes((n + 7) // 8, "little")


def encode(samples):
    """H x W or H x W x C uint8 / uint16 -> the file's bytes."""
    a = np.asarray(samples)
    bits = 8 * a.dtype.itemsize
    assert a.dtype in (np.uint8, np.uint16)
    if a.ndim == 2:
        a = a[:, :, None]
    h, w, c = a.shape
    groups, segments, start = _layout(w, h, c)
    a = a.astype(np.int64)
    table, payload = [], b""
    for g in range(groups):
        for plane in range(c):
            table.append(len(payload))
            heads, data = b"", b""
            for y in range(g * ROWS, min(h, (g + 1) * ROWS)):
                for k in range(segments):
                    xs = range(k * SEG, min(w, (k + 1) * SEG))
                    if y == g * ROWS:      # the left row of the group
                        z = [_zigzag(_signed(int(a[y, x, plane] - a[y, x - 1, plane]), bits)) for x in xs[1:]]
                        raw = [(int(a[y, xs[0], plane]), bits)]
                    else:
                        z = [_zigzag(_signed(int(a[y, x, plane] - a[y - 1, x, plane]), bits)) for x in xs]
                        raw = []
                    b = max(z).bit_length() if z else 0
                    heads += bytes([b])
                    data += _pack_fields(raw + [(v, b) for v in z])
            payload += heads + data
    table.append(len(payload))
    header = MAGIC + struct.pack("<IIHHHHQ", w, h, c, bits, ROWS, SEG, len(payload))
    head = header + struct.pack(f"<{len(table)}I", *table)
    return head + b"\0" * (start - len(head)) + payload


def info(data):
    assert data[:8] == MAGIC
    w, h, c, bits, rows, seg, payload_bytes = struct.unpack("<IIHHHHQ", data[8:32])
    assert (rows, seg) == (ROWS, SEG)
    return w, h, c, bits, payload_bytes


def _field(stream, at, width, msb_first):
    """The `width`-bit field at bit `at` of `stream` (bytes); bits past the end read as zero."""
    if not msb_first:
        return int.from_bytes(stream, "little") >> at & ((1 << width) - 1)
    value = 0
    for i in range(width):
        bit = at + i
        byte = stream[bit >> 3] if (bit >> 3) < len(stream) else 0
        if msb_first:
            value = value << 1 | (byte >> (7 - (bit & 7)) & 1)
        else:
            value |= (byte >> (bit & 7) & 1) << i
    return value


def decode(data, mistake=None):
    """The file's bytes -> H x W x C (H x W for one channel) uint8 / uint16."""
    assert mistake is None or mistake in MISTAKES
    w, h, c, bits, _ = info(data)
    groups, segments, start = _layout(w, h, c)
    table = struct.unpack(f"<{groups * c + 1}I", data[32:32 + 4 * (groups * c + 1)])
    out = np.zeros((h, w, c), dtype=np.int64)
    msb = mistake == "msb_first"
    for g in range(groups):
        for plane in range(c):
            part = data[start + table[g * c + plane]:start + table[g * c + plane + 1]]
            rows = min(ROWS, h - g * ROWS)
            heads, stream = part[:rows * segments], part[rows * segments:]
            at = 0      # byte position in stream
            for r in range(rows):
                y = g * ROWS + r
                left = r == 0
                if mistake == "no_group_restart":
                    left = y == 0
                if mistake == "left_as_up":
                    left = False
                for k in range(segments):
                    n = min(SEG, w - k * SEG)
                    if mistake == "short_segment_16":
                        n = SEG
                    b = heads[r * segments + k] if r * segments + k < len(heads) else 0
                    seg = stream[at:at + 2 * SEG + 8]      # no segment is longer
                    bit = 0
                    for i in range(n):
                        x = k * SEG + i
                        if left and i == 0:
                            value = _field(seg, 0, bits, msb)
                            bit = bits
                        else:
                            z = _field(seg, bit, b, msb)
                            bit += b
                            d = (z >> 1) if z % 2 == 0 else -(z >> 1) - 1
                            if mistake == "zigzag_sign":
                                d = -d
                            if left:
                                pred = out[y, x - 1, plane] if 0 < x <= w else 0
                            else:
                                pred = out[y - 1, x, plane] if y > 0 and x < w else 0
                            value = (pred + d) % (1 << bits)
                        if x < w:
                            out[y, x, plane] = value
                    at += (bit + 7) // 8
    out = out.astype(np.uint16 if bits == 16 else np.uint8)
    return out[:, :, 0] if c == 1 else out


def unpack(image_file, depth_file, y_start, x_start, height, width, middle_only=False, mistake=None):
    """What ops.unpack_packed_frames gives for one frame: (image0, image1, image2, sparse_depth0), 3 x h x w and 1 x h x w float32 --
    the middle, left and right third of the packed triplet (gray replicated, alpha dropped) and the depth / 256, cropped.  With
    middle_only: (image0, sparse_depth0)."""
    triplet = decode(image_file, mistake if mistake != "third_rounded" else None)
    depth = decode(depth_file, mistake if mistake != "third_rounded" else None)
    if triplet.ndim == 2:
        triplet = np.repeat(triplet[:, :, None], 3, axis=2)
    triplet = triplet[:, :, :3]
    w = triplet.shape[1] // 3
    thirds = []
    for t in (1, 0, 2):
        c0 = t * w
        if mistake == "third_rounded":
            c0 = c0 // SEG * SEG
        part = triplet[y_start:y_start + height, c0 + x_start:c0 + x_start + width]
        thirds.append(np.ascontiguousarray(part.transpose(2, 0, 1)).astype(np.float32))
    z = (depth[y_start:y_start + height, x_start:x_start + width].astype(np.float32) / np.float32(256.0))[None]
    return (thirds[0], z) if middle_only else (thirds[0], thirds[1], thirds[2], z)
