"""kb.summary.EventWriter and the host side of ops.histogram_tensorflow, without a GPU: the checksums, the hand-written protobuf, a
file read back by a reader written from the format (tests/event_cases.py), TensorBoard's trimming, the bucket edges, the wiring of
the new entry point and the proof that the histogram oracle tells the near-misses apart."""
import ctypes
import os
import re
import struct
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kbnet_amd as kb  # noqa: E402
import event_cases as ec  # noqa: E402
from kbnet_amd import _lib as L  # noqa: E402

ev = kb.events
KbnError = L.KbnError


def test_crc32c_known_answers_and_the_mask():
    assert ev.crc32c(b"123456789") == 0xE3069283
    assert ev.crc32c(bytes(32)) == 0x8A9136AA
    assert ev.crc32c(b"") == 0
    rng = np.random.default_rng(0)
    for n in (1, 7, 8, 9, 63, 64, 65, 1000):      # the native eight-byte steps and their tail against one byte a step
        data = rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
        assert ev.crc32c(data) == ec.crc32c(data), n
        assert ev.crc32c(data[n // 2:], ev.crc32c(data[:n // 2])) == ec.crc32c(data), n      # continued
    crc = 0xE3069283
    assert ev.masked_crc32c(b"123456789") == (((crc >> 15) | (crc << 17)) + 0xA282EAD8) % 2 ** 32 == ec.mask(crc)
    payload = b"abc"
    rec = ev.record(payload)
    assert rec[:8] == struct.pack("<Q", 3) and rec[12:15] == payload and len(rec) == 8 + 4 + 3 + 4
    assert struct.unpack("<I", rec[8:12])[0] == ec.mask(ec.crc32c(rec[:8])) and struct.unpack("<I", rec[15:])[0] == ec.mask(ec.crc32c(payload))


def test_varints_and_fields_against_hand_written_bytes():
    assert ev.varint(0) == b"\x00" and ev.varint(1) == b"\x01" and ev.varint(127) == b"\x7f"
    assert ev.varint(128) == b"\x80\x01" and ev.varint(300) == b"\xac\x02" and ev.varint(2 ** 32) == b"\x80\x80\x80\x80\x10"
    assert ev.varint(-1) == b"\xff" * 9 + b"\x01"
    assert ev.field_varint(2, 150) == b"\x10\x96\x01"
    assert ev.field_double(1, 1.0) == b"\x09" + bytes(6) + b"\xf0\x3f"
    assert ev.field_float(2, 1.5) == b"\x15\x00\x00\xc0\x3f"
    assert ev.field_float(2, 1e39) == b"\x15\x00\x00\x80\x7f"      # beyond float32: +inf, no exception
    assert ev.field_bytes(3, "brain.Event:2") == b"\x1a\x0dbrain.Event:2"
    assert ev.field_bytes(4, b"\x00\xff") == b"\x22\x02\x00\xff"
    assert ev.field_packed_doubles(6, [1.0, -2.0]) == b"\x32\x10" + struct.pack("<dd", 1.0, -2.0)
    assert ev.event(2.0, file_version="brain.Event:2") == b"\x09" + struct.pack("<d", 2.0) + b"\x1a\x0dbrain.Event:2"
    scalar = b"\x0a\x09" + b"\x0a\x02ab" + b"\x15\x00\x00\xc0\x3f"
    assert ev.summary_scalar("ab", 1.5) == scalar
    assert ev.event(2.0, step=7, summary=scalar) == b"\x09" + struct.pack("<d", 2.0) + b"\x10\x07" + b"\x2a\x0b" + scalar
    assert ev.event(2.0, step=0, summary=scalar) == b"\x09" + struct.pack("<d", 2.0) + b"\x2a\x0b" + scalar      # a default is left out
    image = ev.summary_image("t", 2, 300, b"PNG")
    assert image == b"\x0a\x11" + b"\x0a\x01t" + b"\x22\x0c" + b"\x08\x02" + b"\x10\xac\x02" + b"\x18\x03" + b"\x22\x03PNG"
    histo = ev.summary_histogram("h", -1.0, 2.0, 3.0, 4.0, 5.0, [0.5], [3.0])
    body = b"".join(bytes([8 * k + 1]) + struct.pack("<d", v) for k, v in ((1, -1.0), (2, 2.0), (3, 3.0), (4, 4.0), (5, 5.0)))
    body += b"\x32\x08" + struct.pack("<d", 0.5) + b"\x3a\x08" + struct.pack("<d", 3.0)
    assert histo == b"\x0a" + bytes([len(body) + 5]) + b"\x0a\x01h" + b"\x2a" + bytes([len(body)]) + body


def test_a_file_read_back_by_a_reader_of_the_format(tmp_path):
    counts = np.zeros(1548, dtype=np.int64)
    counts[[774, 900, 901, 1200]] = [5, 1, 7, 2]
    edges = np.asarray(kb.ops.histogram_edges())
    limits, buckets = ev.trim_histogram(counts, edges)
    with kb.summary.EventWriter(str(tmp_path / "events-train"), flush_secs=0) as w:
        w.add_scalar("train_loss", 0.25, global_step=1)
        w.add_scalar("train_big", 1e39, global_step=2)
        w.add_scalar("train_np", np.float64(-3.5), global_step=3)
        w.add_scalar("train_tensor", torch.tensor(7.0), global_step=4)
        w.add_scalar("train_step0", 1.0, global_step=0)
        w.add_histogram_raw("train_depth_distro", -0.0, 9.5, 15, 40.0, 123.0, limits, buckets, global_step=5)
        w.flush()
        assert os.path.getsize(w.path) > 0
        path = w.path
    name = os.path.basename(path)
    assert re.fullmatch(r"events\.out\.tfevents\.\d{10}\.[^/]+\.%d\.\d+" % os.getpid(), name) and os.listdir(tmp_path / "events-train") == [name]
    events = ec.read_events(path)      # checks both checksums of every record
    assert events[0]["file_version"] == "brain.Event:2" and "tag" not in events[0] and events[0]["step"] == 0
    assert all(e["wall_time"] > 1.6e9 for e in events)
    assert [(e["tag"], e["step"], e["kind"]) for e in events[1:]] == [
        ("train_loss", 1, "scalar"), ("train_big", 2, "scalar"), ("train_np", 3, "scalar"), ("train_tensor", 4, "scalar"),
        ("train_step0", 0, "scalar"), ("train_depth_distro", 5, "histo")]
    assert [e["value"] for e in events[1:6]] == [0.25, np.inf, -3.5, 7.0, 1.0]
    h = events[6]["value"]
    assert (h["min"], h["max"], h["num"], h["sum"], h["sum_squares"]) == (0.0, 9.5, 15.0, 40.0, 123.0) and np.signbit(h["min"])
    assert np.array_equal(h["bucket_limit"], limits) and np.array_equal(h["bucket"], buckets)
    assert len(h["bucket"]) == 1200 - 774 + 2 and h["bucket"][0] == 0 and h["bucket"][1] == 5 and h["bucket_limit"][1] == 1e-12


def test_errors_and_the_closed_writer(tmp_path):
    w = kb.summary.EventWriter(str(tmp_path))
    with pytest.raises(ValueError, match="one number"):
        w.add_scalar("per_frame", torch.zeros(3, 4))
    with pytest.raises(ValueError, match="one number"):
        w.add_scalar("array", np.zeros(2))
    with pytest.raises(KbnError):
        w.add_histogram("cpu", torch.ones(5))      # no CPU fallback
    with pytest.raises(KbnError):
        w.add_image("cpu", torch.ones(3, 2, 2))
    with pytest.raises(KbnError, match="3 x H x W"):
        w.add_image("gray", torch.ones(1, 2, 2))
    with pytest.raises(ValueError):
        w.add_histogram_raw("h", 0, 1, 2, 3, 4, [1.0, 2.0], [1.0])
    # an error on the writer's thread: kept, raised ONCE by flush(), the records behind it still written
    w._submit(1, lambda: ev.summary_histogram("empty", 0, 0, 0, 0, 0, *ev.trim_histogram(np.zeros(4), np.arange(5.0))))
    w.add_scalar("after", 2.0, 2)
    with pytest.raises(ValueError, match="The histogram is empty"):
        w.flush()
    w.flush()
    w.add_scalar("last", 3.0, 3)
    w.close()
    w.close()
    for call in (lambda: w.add_scalar("x", 1.0), lambda: w.flush(), lambda: w.add_histogram("x", torch.ones(2)),
                 lambda: w.add_image("x", torch.ones(3, 2, 2)), lambda: w.add_histogram_raw("h", 0, 1, 2, 3, 4, [1.0], [1.0])):
        with pytest.raises(KbnError, match=r"after close\(\)"):
            call()
    assert [e.get("tag") for e in ec.read_events(w.path)] == [None, "after", "last"]
    # an error met at close() is raised by close(), once
    w = kb.summary.EventWriter(str(tmp_path / "second"))
    w._submit(1, lambda: 1 / 0)
    with pytest.raises(ZeroDivisionError):
        w.close()
    w.close()
    assert inspect_signature_names(kb.summary.EventWriter.__init__)[:3] == ["self", "log_dir", "flush_secs"]


def inspect_signature_names(fn):
    import inspect
    return list(inspect.signature(fn).parameters)


@pytest.mark.parametrize("occupied", [[0], [1547], [700], [0, 1547], [3, 4, 9, 200], [774, 775, 1000], [1, 1546]],
                         ids=["bin0", "last", "single", "both-ends", "gaps-low", "gaps", "next-to-ends"])
def test_trimming_equals_make_histogram(occupied):
    edges = np.asarray(kb.ops.histogram_edges())
    counts = np.zeros(1548, dtype=np.int32)
    counts[occupied] = np.arange(1, len(occupied) + 1) * 3
    want_limits, want_counts = ec.make_histogram_oracle(counts, edges)
    limits, buckets = ev.trim_histogram(counts, edges)
    assert np.array_equal(limits, want_limits) and np.array_equal(buckets, want_counts) and buckets.dtype == np.float64
    assert len(limits) == len(buckets) == occupied[-1] - occupied[0] + 2 and buckets[0] == 0 and buckets[1] == 3 and buckets[-1] > 0
    assert limits[-1] == edges[occupied[-1] + 1] and limits[0] == edges[occupied[0]]
    with pytest.raises(ValueError, match="The histogram is empty"):
        ev.trim_histogram(np.zeros(1548, dtype=np.int32), edges)


def test_the_edge_table():
    edges = kb.ops.histogram_edges()
    assert len(edges) == 1549 == kb.ops.HISTOGRAM_BINS + 1 and all(type(e) is float for e in edges)
    assert edges[774] == 0.0 and edges[775] == 1e-12 and edges[776] == 1e-12 * 1.1 and edges[777] == 1e-12 * 1.1 * 1.1
    assert all(edges[774 - k] == -edges[774 + k] for k in range(775))
    assert all(a < b for a, b in zip(edges, edges[1:]))
    assert edges[-1] < 1e20 <= edges[-1] * 1.1
    assert np.array_equal(np.asarray(edges), ec.tensorflow_edges())
    # repeated multiplication, not a power: the two tables differ in the bits of most entries
    power = ec.tensorflow_edges(power=True)
    assert len(power) == 1549 and np.sum(power != np.asarray(edges)) > 1000
    assert L.KBN_HISTOGRAM_POSITIVE_EDGES == 774 and L.KBN_HISTOGRAM_BINS == 1548


def test_wiring_and_refusals_of_the_entry_point():
    assert "histogram.hip" in kb._build.SOURCES
    assert "kbn_histogram_forward" in L.SIGNATURES and "kbn_crc32c" in L.SIGNATURES
    assert L.ABI_VERSION == 11
    header = open(os.path.join(ROOT, "include", "kbnet_hip.h")).read()
    assert int(re.search(r"#define KBN_ABI_VERSION (\d+)", header).group(1)) == 11
    for name, value in (("KBN_HISTOGRAM_POSITIVE_EDGES", 774), ("KBN_HISTOGRAM_BINS", 1548), ("KBN_HISTOGRAM_WORKSPACE_BYTES", 32768)):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == value == getattr(L, name)
    decl = re.search(r"int kbn_histogram_forward\((.*?)\);", header, flags=re.S).group(1)
    assert len(decl.split(",")) == len(L.SIGNATURES["kbn_histogram_forward"][1]) == 8
    lib = L.load()
    buf = (ctypes.c_double * 4096)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    call = lambda x=ptr, n=16, e=ptr, c=ptr, s=ptr, w=ptr, wb=32768: lib.kbn_histogram_forward(x, n, e, c, s, w, wb, None)   # noqa: E731
    # checked before anything is launched (no GPU here)
    assert call(x=None) == call(e=None) == call(c=None) == call(s=None) == call(w=None) == L.KBN_ERR_INVALID_ARGUMENT
    assert call(n=0) == call(n=-1) == L.KBN_ERR_INVALID_ARGUMENT
    assert call(x=ctypes.c_void_p(ptr.value + 2)) == call(s=ctypes.c_void_p(ptr.value + 4)) == L.KBN_ERR_INVALID_ARGUMENT
    assert call(wb=32767) == L.KBN_ERR_WORKSPACE
    assert call(n=2 ** 31) == L.KBN_ERR_UNSUPPORTED
    with pytest.raises(KbnError):
        kb.ops.histogram_tensorflow(torch.ones(4))
    with pytest.raises(KbnError):
        kb.ops.histogram_tensorflow(np.ones(4, dtype=np.float32))
    for name in ("events", "training"):
        text = open(getattr(kb, name).__file__).read()
        for module in ("tensorboard", "torchvision", "matplotlib", "google"):
            assert not re.search(rf"^\s*(import|from)\s+{module}", text, flags=re.M)


def test_the_oracle_tells_the_near_misses_apart():
    """The histogram tests have power: on the planted values, `<=` in place of `<` and float32 comparisons give other counts.

    An edge table built as 1e-12 * 1.1 ** k differs from the repeated product in the bits of 1462 of its 1549 entries
    (test_the_edge_table), yet NO float32 value lies between an entry of one table and its counterpart in the other (the two are
    1e-14 apart, relative; float32 neighbours 1e-7): the counts of float32 data cannot tell the tables apart, and this test states
    that fact instead of the impossible opposite.  What tells them apart is the table itself and the bucket limits written to the
    file, which are compared bit for bit."""
    x = ec.planted_values()
    assert len(x) == 28
    good = ec.histogram_oracle(x)
    assert good.sum() == 21      # +-3e20, NaN, +-inf and the outer neighbours of +-edges[-1] are counted nowhere
    assert np.float64(np.float32(1e-12)) < 1e-12      # so fp32(1e-12) and its neighbour towards 0 lie in the bins next to 0
    assert good[774] == 4 + 2    # 0, -0, 1e-13 and the denormal in [0, 1e-12); fp32(1e-12) and its lower neighbour
    assert good[773] == 1 + 2    # -1e-13; -fp32(1e-12) and its neighbour towards 0
    assert good[775] == 1 + 2    # fp32(1e-12)'s upper neighbour; fp32(edges[776]) lies below edges[776], with its lower neighbour
    assert not np.array_equal(ec.histogram_oracle(x, inclusive_right=True), good)
    assert not np.array_equal(ec.histogram_oracle(x, single=True), good)
    edges, power = ec.tensorflow_edges(), ec.tensorflow_edges(power=True)
    lo, hi = np.minimum(edges, power), np.maximum(edges, power)
    nearest = edges.astype(np.float32).astype(np.float64)      # the only float32 candidates: the values next to each edge
    for candidate in (nearest, np.nextafter(edges.astype(np.float32), np.float32(np.inf)).astype(np.float64),
                      np.nextafter(edges.astype(np.float32), np.float32(-np.inf)).astype(np.float64)):
        assert not np.any((candidate > lo) & (candidate <= hi))
    assert np.array_equal(ec.histogram_oracle(x, edges=power), good)
