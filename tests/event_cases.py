"""What the tests of kb.summary.EventWriter, ops.histogram_tensorflow and kb.training.train share: a reader of event files written
from the documented format alone (its own CRC-32C, its own protobuf walk), NumPy's histogram as the oracle with its near-misses,
the values planted at the bucket edges, and TensorBoard's trimming restated in NumPy."""
import math
import struct

import numpy as np

# ------------------------------------------------------------------------------------------------ the reader
_TABLE = []
for _i in range(256):
    _c = _i
    for _ in range(8):
        _c = (_c >> 1) ^ (0x82F63B78 if _c & 1 else 0)
    _TABLE.append(_c)


def crc32c(data: bytes) -> int:
    """Castagnoli, one byte a step."""
    c = 0xFFFFFFFF
    for b in data:
        c = (c >> 8) ^ _TABLE[(c ^ b) & 0xFF]
    return c ^ 0xFFFFFFFF


def mask(crc: int) -> int:
    return (((crc >> 15) | (crc << 17)) + 0xA282EAD8) % (1 << 32)


def fields(message: bytes):
    """[(field number, wire type, value)] of one protobuf message: varints as ints, 64- and 32-bit values and length-delimited
    ones as bytes."""
    out, at = [], 0

    def varint():
        nonlocal at
        value, shift = 0, 0
        while True:
            b = message[at]
            at += 1
            value |= (b & 0x7F) << shift
            shift += 7
            if not b & 0x80:
                return value

    while at < len(message):
        key = varint()
        number, wire = key >> 3, key & 7
        if wire == 0:
            value = varint()
        elif wire == 1:
            value, at = message[at:at + 8], at + 8
        elif wire == 5:
            value, at = message[at:at + 4], at + 4
        elif wire == 2:
            n = varint()
            value, at = message[at:at + n], at + n
            assert len(value) == n
        else:
            raise AssertionError(f"wire type {wire}")
        out.append((number, wire, value))
    assert at == len(message)
    return out


def _one(fs, number, default=None):
    found = [v for n, _, v in fs if n == number]
    assert len(found) <= 1
    return found[0] if found else default


def _double(b):
    return struct.unpack("<d", b)[0]


def read_events(path):
    """Every record of an event file, both checksums verified -> a list of dicts: wall_time, step, and file_version or
    (tag, kind, value) -- kind 'scalar' (a float32 as float), 'image' (height, width, colorspace, png bytes) or 'histo' (a dict with
    min, max, num, sum, sum_squares, bucket_limit, bucket)."""
    with open(path, "rb") as f:
        data = f.read()
    events, at = [], 0
    while at < len(data):
        header = data[at:at + 8]
        (length,) = struct.unpack("<Q", header)
        assert struct.unpack("<I", data[at + 8:at + 12])[0] == mask(crc32c(header)), "length checksum"
        payload = data[at + 12:at + 12 + length]
        assert len(payload) == length
        assert struct.unpack("<I", data[at + 12 + length:at + 16 + length])[0] == mask(crc32c(payload)), "payload checksum"
        at += 16 + length
        fs = fields(payload)
        assert {n for n, _, _ in fs} <= {1, 2, 3, 5}
        e = {"wall_time": _double(_one(fs, 1)), "step": _one(fs, 2, 0)}
        version, summary = _one(fs, 3), _one(fs, 5)
        if version is not None:
            e["file_version"] = version.decode()
        if summary is not None:
            (value,) = [v for n, _, v in fields(summary) if n == 1]
            vs = fields(value)
            e["tag"] = _one(vs, 1).decode()
            if _one(vs, 2) is not None:
                e["kind"], e["value"] = "scalar", float(np.frombuffer(_one(vs, 2), dtype="<f4")[0])
            elif _one(vs, 4) is not None:
                im = fields(_one(vs, 4))
                e["kind"], e["value"] = "image", (_one(im, 1), _one(im, 2), _one(im, 3), _one(im, 4))
            else:
                h = fields(_one(vs, 5))
                e["kind"] = "histo"
                e["value"] = dict(min=_double(_one(h, 1)), max=_double(_one(h, 2)), num=_double(_one(h, 3)), sum=_double(_one(h, 4)),
                                  sum_squares=_double(_one(h, 5)), bucket_limit=np.frombuffer(_one(h, 6), dtype="<f8"),
                                  bucket=np.frombuffer(_one(h, 7), dtype="<f8"))
        events.append(e)
    return events


# ------------------------------------------------------------------------------------------------ the histogram
def tensorflow_edges(power=False):
    """SummaryWriter.add_histogram(bins='tensorflow')'s edges, restated; `power`: the near-miss 1e-12 * 1.1 ** k."""
    positive = []
    v, k = 1e-12, 0
    while v < 1e20:
        positive.append(v)
        k += 1
        v = 1e-12 * 1.1 ** k if power else v * 1.1
    return np.array([-e for e in reversed(positive)] + [0.0] + positive, dtype=np.float64)


def histogram_oracle(values, edges=None, inclusive_right=False, single=False):
    """np.histogram(values.astype(float), bins=edges)[0].  Near-misses for the proof of power: `inclusive_right` counts a value AT an
    edge in the bin to its left (edges[i] < x <= edges[i + 1]); `single` compares in float32."""
    edges = tensorflow_edges() if edges is None else edges
    x = np.asarray(values, dtype=np.float32).reshape(-1)
    if inclusive_right or single:
        e = edges.astype(np.float32) if single else edges
        v = x if single else x.astype(np.float64)
        v = v[np.isfinite(v)]
        index = np.searchsorted(e, v, side="left" if inclusive_right else "right") - 1
        if not inclusive_right:
            index[v == e[-1]] = len(e) - 2
        index = index[(index >= 0) & (index < len(e) - 1)]
        return np.bincount(index, minlength=len(e) - 1)
    x = x.astype(np.float64)
    return np.histogram(x[np.isfinite(x)], bins=edges)[0]      # np.histogram refuses a range with NaN; no bin takes +-inf


def planted_values():
    """0, -0, every one of +-edges[775], +-edges[776], +-edges[-1] rounded to float32 with its two float32 neighbours, +-1e-13, the
    smallest denormal, +-3e20, NaN, +-inf."""
    edges = tensorflow_edges()
    out = [0.0, -0.0]
    for e in (edges[775], edges[776], edges[-1]):
        for sign in (1.0, -1.0):
            r = np.float32(sign * e)
            out += [r, np.nextafter(r, np.float32(np.inf)), np.nextafter(r, np.float32(-np.inf))]
    out += [1e-13, -1e-13, np.float32(1e-45), 3e20, -3e20, np.nan, np.inf, -np.inf]
    return np.asarray(out, dtype=np.float32)


def seeded_values(n, seed, plant=True, finite=False):
    """n float32 values over 30 decades of both signs; the planted ones written over the front, as many as fit (`finite`: all but
    NaN and +-inf, for the gates on the sums)."""
    rng = np.random.default_rng(seed)
    x = (rng.choice([-1.0, 1.0], size=n) * 10.0 ** rng.uniform(-15.0, 15.0, size=n)).astype(np.float32)
    if plant:
        p = planted_values()
        p = p[np.isfinite(p)] if finite else p
        k = min(n, p.size)
        x[:k] = p[:k]
    return x


def stats_oracle(values):
    """(min, max, num, sum, sum_squares) as TensorBoard computes them on values.astype(float), the sums by math.fsum; and the two
    bounds 1e-9 * sum|x|, 1e-9 * sum x^2 (n * 2^-53 with n <= 2^23 holds for any summation order).  The sums are None when a value
    is not finite."""
    x = np.asarray(values, dtype=np.float32).reshape(-1).astype(np.float64)
    with np.errstate(invalid="ignore"):
        lo, hi = np.min(x), np.max(x)
    if not np.all(np.isfinite(x)):
        return lo, hi, float(x.size), None, None, None, None
    total, squares = math.fsum(x), math.fsum(x * x)
    return lo, hi, float(x.size), total, squares, 1e-9 * math.fsum(np.abs(x)), 1e-9 * squares


def make_histogram_oracle(counts, limits):
    """torch/utils/tensorboard/summary.py make_histogram's trimming, restated: (limits, counts) of the support with an empty bin kept
    to its left, right-hand limits only."""
    counts, limits = np.asarray(counts), np.asarray(limits)
    cum_counts = np.cumsum(np.greater(counts, 0))
    start, end = np.searchsorted(cum_counts, [0, cum_counts[-1] - 1], side="right")
    start, end = int(start), int(end) + 1
    counts = counts[start - 1:end] if start > 0 else np.concatenate([[0], counts[:end]])
    limits = limits[start:end + 1]
    assert counts.size and limits.size
    return limits, counts
