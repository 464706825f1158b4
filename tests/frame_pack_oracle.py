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


def _segment_bytes(n, b, bits, left):
    """Bytes of a segment's fields (frame_pack.h): a left row stores its first sample raw and n - 1 fields, an up row n fields."""
    return ((bits + (n - 1) * b if left else n * b) + 7) // 8


def _assemble(w, h, c, bits, parts):
    """The file around the (group, plane) payloads `parts` [(header bytes, field bytes)] in table order."""
    groups, _, start = _layout(w, h, c)
    assert len(parts) == groups * c
    table, payload = [], b""
    for heads, data in parts:
        table.append(len(payload))
        payload += heads + data
    table.append(len(payload))
    header = MAGIC + struct.pack("<IIHHHHQ", w, h, c, bits, ROWS, SEG, len(payload))
    head = header + struct.pack(f"<{len(table)}I", *table)
    return head + b"\0" * (start - len(head)) + payload


def build(samples, widths=None, pad=None):
    """A file of `samples` that need not be the canonical one: the header byte of segment (group, plane, row in group, k) is
    widths(group, plane, row, k, needed, bits) clipped to [needed, bits] (`needed`: what encode() writes), and the bits between the
    last field and the segment's end are the low bits of pad(group, plane, row, k, count).  With both None: encode(samples)."""
    a = np.asarray(samples)
    bits = 8 * a.dtype.itemsize
    assert a.dtype in (np.uint8, np.uint16)
    if a.ndim == 2:
        a = a[:, :, None]
    h, w, c = a.shape
    groups, segments, _ = _layout(w, h, c)
    a = a.astype(np.int64)
    parts = []
    for g in range(groups):
        for plane in range(c):
            heads, data = b"", b""
            for y in range(g * ROWS, min(h, (g + 1) * ROWS)):
                r = y - g * ROWS
                for k in range(segments):
                    xs = range(k * SEG, min(w, (k + 1) * SEG))
                    if r == 0:
                        z = [_zigzag(_signed(int(a[y, x, plane] - a[y, x - 1, plane]), bits)) for x in xs[1:]]
                        raw = [(int(a[y, xs[0], plane]), bits)]
                    else:
                        z = [_zigzag(_signed(int(a[y, x, plane] - a[y - 1, x, plane]), bits)) for x in xs]
                        raw = []
                    needed = max(z).bit_length() if z else 0
                    b = needed if widths is None else min(bits, max(needed, int(widths(g, plane, r, k, needed, bits))))
                    fields = raw + [(v, b) for v in z]
                    used = sum(width for _, width in fields)
                    spare = -used % 8
                    if pad is not None and spare:
                        fields.append((int(pad(g, plane, r, k, spare)) & ((1 << spare) - 1), spare))
                    heads += bytes([b])
                    data += _pack_fields(fields)
                    assert len(_pack_fields(fields)) == _segment_bytes(len(xs), b, bits, r == 0)
            parts.append((heads, data))
    out = _assemble(w, h, c, bits, parts)
    if widths is None and pad is None:
        assert out == encode(samples)
    return out


def build_random(w, h, c, bits, rng):
    """A file nobody encoded: every header byte uniform in [0, bits], every field and pad bit random, the table from the segments'
    sizes.  Returns (file, samples): the samples are what decode() makes of it."""
    groups, segments, _ = _layout(w, h, c)
    parts = []
    for g in range(groups):
        rows = min(ROWS, h - g * ROWS)
        for _ in range(c):
            heads = bytes(int(v) for v in rng.integers(0, bits + 1, size=rows * segments))
            size = sum(_segment_bytes(min(SEG, w - k * SEG), heads[r * segments + k], bits, r == 0)
                       for r in range(rows) for k in range(segments))
            parts.append((heads, bytes(int(v) for v in rng.integers(0, 256, size=size))))
    data = _assemble(w, h, c, bits, parts)
    return data, decode(data)


WIDTH_CHOICES = ("all_bits", "needed_plus_1", "random", "build_random")


def hand_made(choice, w, h, c, bits, seed=0):
    """(file, samples) of a hand-made file that is not the canonical encoding of its samples, by one of WIDTH_CHOICES: every b = bits;
    b = needed + 1 with every pad bit set; the first b = needed + 1, the others random in [needed, bits], random pad bits;
    build_random.  The samples of the first three are noise / 16: at most bits - 3 bits a field, so there is room above."""
    assert choice in WIDTH_CHOICES
    for attempt in range(10):
        g = np.random.Generator(np.random.Philox(977 * seed + 31 * w + h + 7 * c + bits + 1000 * attempt))
        if choice == "build_random":
            data, a = build_random(w, h, c, bits, g)
        else:
            a = (g.integers(0, 1 << bits, size=(h, w, c)) // 16).astype(np.uint16 if bits == 16 else np.uint8)
            a = a[:, :, 0] if c == 1 else a
            first = []

            def widths(group, plane, row, k, needed, top):
                if choice == "all_bits":
                    return top
                if choice == "needed_plus_1" or not first:
                    first.append(1)
                    return needed + 1
                return int(g.integers(needed, top + 1))

            pad = {"all_bits": None, "needed_plus_1": lambda *_: 0xff, "random": lambda *_: int(g.integers(0, 256))}[choice]
            data = build(a, widths, pad)
        if data != encode(a):
            return data, a
    raise AssertionError("no non-canonical file in ten draws")


def segments_of(data):
    """[(b, needed, pad bits as an int)] of every segment of a file, read back from its bytes: `needed` is the width of the largest
    field the segment holds."""
    w, h, c, bits, _ = info(data)
    groups, segments, start = _layout(w, h, c)
    table = struct.unpack(f"<{groups * c + 1}I", data[32:32 + 4 * (groups * c + 1)])
    out = []
    for e in range(groups * c):
        part = data[start + table[e]:start + table[e + 1]]
        rows = min(ROWS, h - e // c * ROWS)
        at = rows * segments
        for r in range(rows):
            for k in range(segments):
                n, b = min(SEG, w - k * SEG), part[r * segments + k]
                size = _segment_bytes(n, b, bits, r == 0)
                value = int.from_bytes(part[at:at + size], "little")
                used = (bits + (n - 1) * b) if r == 0 else n * b
                fields = [(value >> ((bits if r == 0 else 0) + i * b)) & ((1 << b) - 1) for i in range(n - 1 if r == 0 else n)]
                out.append((b, max(fields).bit_length() if fields else 0, value >> used))
                at += size
    return out


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
