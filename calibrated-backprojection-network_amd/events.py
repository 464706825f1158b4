"""TensorBoard event files without tensorboard: the writer the training loop hands to log_summary and validate (kb.summary.EventWriter)
where the reference opens torch.utils.tensorboard.SummaryWriter (src/kbnet.py:239-240).

The file.  `events.out.tfevents.<seconds>.<hostname>.<pid>.<n>` in log_dir, a run of records
    length        8 bytes, little-endian
    masked CRC-32C of those 8 bytes      4 bytes, little-endian
    payload       `length` bytes: a serialised Event message
    masked CRC-32C of the payload        4 bytes
with mask(crc) = ((crc >> 15 | crc << 17) + 0xa282ead8) mod 2^32.  The messages are written by hand (no protobuf package):
    Event           wall_time 1 (double), step 2 (varint), file_version 3 (string; the first record: "brain.Event:2"), summary 5
    Summary         value 1 (repeated; one a record here)
    Summary.Value   tag 1, simple_value 2 (float), image 4, histo 5
    Summary.Image   height 1, width 2, colorspace 3, encoded_image_string 4 (a PNG file)
    HistogramProto  min 1, max 2, num 3, sum 4, sum_squares 5 (doubles), bucket_limit 6, bucket 7 (packed doubles)

What the caller pays.  add_histogram is ops.histogram_tensorflow (two launches over the tensor where it lies), add_image one
ops.export_pack launch, add_scalar of a device scalar nothing; each then records an event on the caller's stream, lets the writer's
side stream copy the result -- 6224 bytes, 3 bytes a pixel, one number -- into pinned memory behind it and returns.  ONE writer
thread waits for each copy, trims the histogram to its support (TensorBoard's make_histogram), encodes the PNG
(kbn_png_encode_rgb8), serialises and appends the records in call order.  flush() and close() wait for that thread and raise the
first error it met, once."""

from __future__ import annotations

import os
import queue
import socket
import struct
import threading
import time

import numpy as np
import torch

from . import _lib, ops
from ._lib import KbnError

FILE_VERSION = "brain.Event:2"
PNG_LEVEL = 6      # zlib level of an image record, as loader.OutputWriter's default
_SERIAL = [0]
_SERIAL_LOCK = threading.Lock()


# ------------------------------------------------------------------------------------------------ the record
def crc32c(data: bytes, crc: int = 0) -> int:
    """CRC-32C (Castagnoli) of `data`, continued from `crc`: crc32c(b'123456789') == 0xE3069283 (kbn_crc32c, a host function)."""
    data = bytes(data)
    return int(_lib.load().kbn_crc32c(data, len(data), crc & 0xFFFFFFFF)) & 0xFFFFFFFF


def masked_crc32c(data: bytes) -> int:
    crc = crc32c(data)
    return (((crc >> 15) | (crc << 17)) + 0xA282EAD8) & 0xFFFFFFFF


def record(payload: bytes) -> bytes:
    """One record of an event file around a serialised Event."""
    header = struct.pack("<Q", len(payload))
    return header + struct.pack("<I", masked_crc32c(header)) + payload + struct.pack("<I", masked_crc32c(payload))


# ------------------------------------------------------------------------------------------------ the messages
def varint(value: int) -> bytes:
    """Protocol buffers' base-128 varint; a negative int64 is its two's complement, ten bytes."""
    value = int(value) & 0xFFFFFFFFFFFFFFFF
    out = bytearray()
    while value > 0x7F:
        out.append((value & 0x7F) | 0x80)
        value >>= 7
    out.append(value)
    return bytes(out)


def field_varint(number: int, value: int) -> bytes:
    return varint(number << 3) + varint(value)


def field_double(number: int, value: float) -> bytes:
    return varint(number << 3 | 1) + struct.pack("<d", value)


def field_float(number: int, value: float) -> bytes:
    with np.errstate(over="ignore"):      # np.float32: +-inf beyond the range, where struct.pack raises
        return varint(number << 3 | 5) + np.asarray(value, dtype="<f4").tobytes()


def field_bytes(number: int, value) -> bytes:
    value = value.encode("utf-8") if isinstance(value, str) else bytes(value)
    return varint(number << 3 | 2) + varint(len(value)) + value


def field_packed_doubles(number: int, values) -> bytes:
    return field_bytes(number, np.asarray(values, dtype="<f8").tobytes())


def event(wall_time: float, step=None, file_version=None, summary=None) -> bytes:
    """A serialised Event; step 0 is left out, as protobuf leaves out a default."""
    out = field_double(1, wall_time)
    if step:
        out += field_varint(2, step)
    if file_version is not None:
        out += field_bytes(3, file_version)
    if summary is not None:
        out += field_bytes(5, summary)
    return out


def summary_scalar(tag: str, value: float) -> bytes:
    return field_bytes(1, field_bytes(1, tag) + field_float(2, value))


def summary_image(tag: str, height: int, width: int, png: bytes, colorspace: int = 3) -> bytes:
    image = field_varint(1, height) + field_varint(2, width) + field_varint(3, colorspace) + field_bytes(4, png)
    return field_bytes(1, field_bytes(1, tag) + field_bytes(4, image))


def summary_histogram(tag: str, minimum: float, maximum: float, num: float, total: float, sum_squares: float, bucket_limit, bucket) -> bytes:
    histo = (field_double(1, minimum) + field_double(2, maximum) + field_double(3, num) + field_double(4, total) +
             field_double(5, sum_squares) + field_packed_doubles(6, bucket_limit) + field_packed_doubles(7, bucket))
    return field_bytes(1, field_bytes(1, tag) + field_bytes(5, histo))


def trim_histogram(counts, edges):
    """TensorBoard's make_histogram on np.histogram's (counts, edges) -> (bucket_limit, bucket): the bins from the first to the last
    occupied one with ONE empty bin kept to their left (a new one when the first bin is occupied), and the right-hand limit of
    each.  No occupied bin raises ValueError, as make_histogram does."""
    counts = np.asarray(counts)
    edges = np.asarray(edges, dtype=np.float64)
    occupied = np.flatnonzero(counts > 0)
    if occupied.size == 0:
        raise ValueError("The histogram is empty, please file a bug report.")
    start, end = int(occupied[0]), int(occupied[-1]) + 1
    bucket = counts[start - 1:end] if start > 0 else np.concatenate([[0], counts[:end]])
    return edges[start:end + 1], bucket.astype(np.float64)


# ------------------------------------------------------------------------------------------------ the writer
class EventWriter:
    """add_scalar / add_histogram / add_image / flush / close of torch.utils.tensorboard.SummaryWriter for what log_summary and
    validate pass (see the module text): `values` any fp32 device tensor, `img_tensor` 3 x H x W fp32 on the device, a scalar a
    Python number or a tensor of one element (a device scalar is fetched by a deferred copy, never by .item(); more than one
    element raises ValueError).  Bytes of an image are clip(trunc(255 x), 0, 255), NaN -> 0: TensorBoard's
    (t * 255).clip(0, 255).astype(uint8).  Calls return without waiting for the device.  flush_secs: the file is flushed when a
    record is written that long after the last flush, and by flush() and close().  Calls after close() raise KbnError.  A context
    manager.  One writer is driven by one thread at a time."""

    def __init__(self, log_dir, flush_secs: float = 120):
        self.log_dir = str(log_dir)
        os.makedirs(self.log_dir, exist_ok=True)
        with _SERIAL_LOCK:
            serial = _SERIAL[0]
            _SERIAL[0] += 1
        self.path = os.path.join(self.log_dir, "events.out.tfevents.{:010d}.{}.{}.{}".format(int(time.time()), socket.gethostname(), os.getpid(), serial))
        self.flush_secs = float(flush_secs)
        self._file = open(self.path, "wb")
        self._file.write(record(event(time.time(), file_version=FILE_VERSION)))
        self._file.flush()
        self._flushed = time.monotonic()
        self._edges = np.asarray(ops.histogram_edges(), dtype=np.float64)
        self._queue: "queue.Queue" = queue.Queue()
        self._error = None
        self._closed = False
        self._copy_stream = None
        self._thread = threading.Thread(target=self._run, name="kbn-event-writer", daemon=True)
        self._thread.start()

    # -- the writer thread ----------------------------------------------------------------------
    def _run(self):
        while True:
            job = self._queue.get()
            if job is None:
                return
            if isinstance(job, threading.Event):      # flush(): everything queued before it is in the file
                try:
                    self._file.flush()
                    self._flushed = time.monotonic()
                except Exception as e:      # noqa: BLE001
                    self._error = self._error or e
                job.set()
                continue
            wall_time, step, make = job
            try:
                self._file.write(record(event(wall_time, step=step, summary=make())))
                if time.monotonic() - self._flushed >= self.flush_secs:
                    self._file.flush()
                    self._flushed = time.monotonic()
            except Exception as e:      # noqa: BLE001  (kept for flush() / close(); the records behind it are still written)
                self._error = self._error or e

    def _submit(self, step, make):
        self._queue.put((time.time(), 0 if step is None else int(step), make))

    def _open(self, what: str):
        if self._closed:
            raise KbnError(f"EventWriter: {what}() after close()")

    # -- device -> pinned memory, behind the caller's stream --------------------------------------
    def _fetch(self, t: torch.Tensor):
        """(pinned host tensor, event): the copy of the dense device tensor `t` runs on the writer's side stream once the caller's
        stream has reached this point; nobody waits here."""
        device = t.device
        with torch.cuda.device(device):
            if self._copy_stream is None or self._copy_stream.device != device:
                self._copy_stream = torch.cuda.Stream(device=device)
            ready = torch.cuda.Event()
            ready.record(torch.cuda.current_stream(device))
            self._copy_stream.wait_event(ready)
            host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            t.record_stream(self._copy_stream)      # the allocator learns that the side stream reads it
            with torch.cuda.stream(self._copy_stream):
                host.copy_(t, non_blocking=True)
                done = torch.cuda.Event()
                done.record(self._copy_stream)
        return host, done

    # -- SummaryWriter's methods --------------------------------------------------------------------
    def add_scalar(self, tag, scalar_value, global_step=None):
        self._open("add_scalar")
        tag = str(tag)
        if isinstance(scalar_value, torch.Tensor):
            if scalar_value.numel() != 1:
                raise ValueError(f"EventWriter.add_scalar: {tag}: a scalar is one number, got a tensor of shape {tuple(scalar_value.shape)}")
            if scalar_value.is_cuda:
                host, done = self._fetch(scalar_value.detach().reshape(1))

                def make():
                    done.synchronize()
                    return summary_scalar(tag, float(host.item()))
                return self._submit(global_step, make)
            scalar_value = scalar_value.item()
        elif isinstance(scalar_value, np.ndarray) and scalar_value.size != 1:
            raise ValueError(f"EventWriter.add_scalar: {tag}: a scalar is one number, got an array of shape {scalar_value.shape}")
        value = float(scalar_value)
        self._submit(global_step, lambda: summary_scalar(tag, value))

    def add_histogram(self, tag, values, global_step=None, bins="tensorflow"):
        self._open("add_histogram")
        tag = str(tag)
        if bins != "tensorflow":
            raise KbnError(f"EventWriter.add_histogram: bins={bins!r}: the kernel serves TensorBoard's default, 'tensorflow'")
        counts, _ = ops.histogram_tensorflow(values)      # raises for a CPU tensor and for an empty one
        num = float(values.numel())
        host, done = self._fetch(counts._base)      # the counts and the four sums: one buffer, one copy

        def make():
            done.synchronize()
            packed = host.numpy()
            minimum, maximum, total, sum_squares = (float(v) for v in packed[ops.HISTOGRAM_BINS:].view(np.float64))
            bucket_limit, bucket = trim_histogram(packed[:ops.HISTOGRAM_BINS], self._edges)
            return summary_histogram(tag, minimum, maximum, num, total, sum_squares, bucket_limit, bucket)
        self._submit(global_step, make)

    def add_histogram_raw(self, tag, min, max, num, sum, sum_squares, bucket_limits, bucket_counts, global_step=None):      # noqa: A002
        """SummaryWriter's method of this name: a histogram the caller made, written as it is (host numbers)."""
        self._open("add_histogram_raw")
        tag = str(tag)
        if len(bucket_limits) != len(bucket_counts):
            raise ValueError("len(bucket_limits) != len(bucket_counts), see the document.")
        numbers = [float(v) for v in (min, max, num, sum, sum_squares)]
        limits, buckets = np.array(bucket_limits, dtype=np.float64), np.array(bucket_counts, dtype=np.float64)
        self._submit(global_step, lambda: summary_histogram(tag, *numbers, limits, buckets))

    def add_image(self, tag, img_tensor, global_step=None, dataformats="CHW"):
        self._open("add_image")
        tag = str(tag)
        if dataformats != "CHW" or not isinstance(img_tensor, torch.Tensor) or img_tensor.dim() != 3 or img_tensor.shape[0] != 3:
            shape = tuple(img_tensor.shape) if isinstance(img_tensor, torch.Tensor) else type(img_tensor).__name__
            raise KbnError(f"EventWriter.add_image: {tag}: expected a 3 x H x W tensor in 'CHW', got {shape} in {dataformats!r}")
        height, width = int(img_tensor.shape[1]), int(img_tensor.shape[2])
        rgb, _, _ = ops.export_pack(image=img_tensor.unsqueeze(0), scale=255.0, shift=0.0)      # raises for a CPU tensor
        host, done = self._fetch(rgb)

        def make():
            from . import loader      # here: loader imports modules, which imports summary
            done.synchronize()
            png = loader._encode_png("rgb8", host.numpy()[0], width, height, PNG_LEVEL)
            return summary_image(tag, height, width, bytes(png))
        self._submit(global_step, make)

    def flush(self):
        """Waits until everything added so far is in the file; raises the first error the writer thread met (once)."""
        self._open("flush")
        self._wait()
        self._raise()

    def _wait(self):
        reached = threading.Event()
        self._queue.put(reached)
        reached.wait()

    def _raise(self):
        error, self._error = self._error, None
        if error is not None:
            raise error

    def close(self):
        """flush(), then the thread ends and the file is closed; raises the first error the writer thread met (once)."""
        if not self._closed:
            self._closed = True
            self._wait()
            self._queue.put(None)
            self._thread.join()
            self._file.close()
        self._raise()

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        else:           # the body failed: finish quietly, its exception is the one to see
            try:
                self.close()
            except Exception:      # noqa: BLE001
                pass
        return False
