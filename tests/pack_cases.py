"""Sample generators for the packed-frame ENCODER tests (tests/test_pack_frames_gpu.py, tests/test_pack_outputs_*.py): the contents
DESIGN 8u names, each an H x W x C uint8 / uint16 array that is a pure function of its arguments."""
import numpy as np

ROWS, SEG = 8, 16
CONTENTS = ("constant", "ramp", "wrap", "noise", "sparse")


def ramp_b(y, k, segments, bits, shift=0):
    """The header byte the ramp content asks of segment k of row y -- every value 0 .. bits in turn.  A left row's one-sample
    segment holds no residual, so its b is 0 whatever is asked."""
    return (y * segments + k + shift) % (bits + 1)


def _ramp(h, w, c, bits, shift):
    """Every segment gets residuals whose largest field is exactly b = ramp_b(...) bits long: d = 0 (b = 0), -1 (zigzag 1, b = 1),
    2^(b-2) (zigzag 2^(b-1), b >= 2).  Left rows are running sums of d along the row, up rows the row above plus d."""
    segments = -(-w // SEG)
    d = np.zeros((h, w, c), dtype=np.int64)
    for y in range(h):
        for k in range(segments):
            for plane in range(c):
                b = ramp_b(y, k, segments, bits, shift + plane)
                d[y, k * SEG:(k + 1) * SEG, plane] = 0 if b == 0 else -1 if b == 1 else 1 << (b - 2)
    a = np.zeros((h, w, c), dtype=np.int64)
    for y in range(h):
        a[y] = np.cumsum(d[y], axis=0) + 5 if y % ROWS == 0 else a[y - 1] + d[y]
    return a % (1 << bits)


def make(content, h, w, c, bits, seed=0):
    """One frame, H x W x C, uint8 (bits 8) or uint16 (bits 16)."""
    dtype = np.uint16 if bits == 16 else np.uint8
    top = (1 << bits) - 1
    rng = np.random.default_rng([seed, h, w, c, bits, CONTENTS.index(content)])
    if content == "constant":      # every b = 0: segments with no residual bits
        a = np.full((h, w, c), (37 + 41 * seed) % (top + 1))
    elif content == "ramp":
        a = _ramp(h, w, c, bits, seed)
    elif content == "wrap":        # 0 next to 2^bits - 1, both orders (seed's parity swaps them): differences of +-1 mod 2^bits
        y, x, p = np.meshgrid(np.arange(h), np.arange(w), np.arange(c), indexing="ij")
        a = np.where((y + x + p + seed) % 2 == 0, 0, top)
    elif content == "noise":
        a = rng.integers(0, top + 1, size=(h, w, c))
    elif content == "sparse":      # 1 sample in 20, as a sparse depth map
        a = np.where(rng.random((h, w, c)) < 0.05, rng.integers(1, top + 1, size=(h, w, c)), 0)
    else:
        raise ValueError(content)
    return np.ascontiguousarray(a.astype(dtype))


def batch(contents, h, w, c, bits, seed=0):
    """len(contents) frames, N x H x W x C."""
    return np.stack([make(content, h, w, c, bits, seed + i) for i, content in enumerate(contents)])


def table(data):
    """The table of a packed file: (payload start, offsets)."""
    w, h, c = int.from_bytes(data[8:12], "little"), int.from_bytes(data[12:16], "little"), int.from_bytes(data[16:18], "little")
    entries = -(-h // ROWS) * c
    start = (32 + 4 * (entries + 1) + 15) // 16 * 16
    return start, [int.from_bytes(data[32 + 4 * e:36 + 4 * e], "little") for e in range(entries + 1)]


def header_bytes(data):
    """Every segment's b of a packed file, as a flat list."""
    w, h, c = int.from_bytes(data[8:12], "little"), int.from_bytes(data[12:16], "little"), int.from_bytes(data[16:18], "little")
    start, offsets = table(data)
    segments = -(-w // SEG)
    out = []
    for e in range(len(offsets) - 1):
        rows = min(ROWS, h - (e // c) * ROWS)
        out += list(data[start + offsets[e]:start + offsets[e] + rows * segments])
    return out


def first_difference(a, b):
    """The first index at which two byte strings differ (the shorter one's length when it is a prefix of the other)."""
    return next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
