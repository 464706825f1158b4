"""Input pipeline: PNG / .npy files -> batched device tensors.

The reference feeds inference from `datasets.KBNetInferenceDataset` through a one-worker, batch-1
`torch.utils.data.DataLoader` and moves every sample to the device on its own
(reference src/kbnet.py:764-772, 887-896; src/datasets.py:229-286; PIL decode in
src/data_utils.py:58-152).  At > 1000 frames/s per GPU that loader is the bottleneck, so here

  * a pool of host threads decodes the PNG files with the library's own reader
    (`kbn_png_decode`: zlib inflate + scanline filters in C++; ctypes drops the GIL around the call)
    straight into PINNED staging tensors, a whole batch at a time;
  * the raw bytes (3 B/px image, 2 B/px depth instead of 12 + 4 B/px of float32) cross PCIe with one
    asynchronous copy per tensor on a side stream, overlapped with the previous batch's forward;
  * `kbn_unpack_frames_forward` turns them into the dataset's tensors on the device (triplet crop,
    uint8 -> float32, depth / 256); `ops.preprocess` (row f1) continues from there.

`load_image`, `load_depth`, `load_image_triplet` mirror the reference functions of the same names
(numpy in, numpy out) on top of the same decoder.

Training (`TrainingFrameLoader`, in place of a `DataLoader` over `datasets.KBNetTrainingDataset`, reference
src/datasets.py:161-228, src/kbnet.py:134-144) takes the same road with all three images of a triplet, frames of
different raw sizes in one batch and the reference's random crop: `draw_crop` makes the reference's np.random
decisions on the host, `kbn_unpack_train_frames_forward` cuts every frame's crop out of its raw bytes on the device.
`random_crop` is the reference-named NumPy function on top of `draw_crop`.

Packed frames: both loaders take, wherever they take a PNG, a file written by `encode_frame` / `pack_frames` and
recognised by its magic.  Such a file is not decoded on the host at all: it is read straight into pinned staging, passes the
structural check `kbn_frame_check` there, crosses PCIe packed, and `ops.unpack_packed_frames` decodes, splits, crops and converts
on the device -- the same tensors bit for bit.  A batch is all PNG or all packed.  `frame_info`, `encode_frame`, `decode_frame`,
`check_frame` are the host codec.

Sequence entries: an entry of an image path list is the path of a triplet file -- frames t-1, t, t+1 side by side, what the
reference's setup scripts write -- or `previous<TAB>current<TAB>next`, the three frames by path (`split_sample` is the one place that
knows the syntax, `sequence_lines` writes such entries for an ordered sequence).  Both loaders then read every distinct file of a batch
once, PNG or packed, and `ops.unpack_sequence_frames` / `ops.unpack_packed_sequence_frames` build the triplet path's tensors, bit for
bit, from the frames where they lie; the inference loader reads `current` alone.  A batch is all triplet files or all sequence entries.

Both loaders stage every batch, PNG or packed, the same way (`_Staging`): one set of flat pinned byte buffers per slot,
`prefetch + 1` of them, grown with 1/8 of headroom when a batch needs more and never touched before the copies that last used it
are done.  A submit path lays its files out, fills the set and passes its unpack op to `_Staging.submit`, which copies the used
prefixes, launches and records the set's event.  A file's kind, size and format come from its first 33 bytes, read once a path
(`_FileHeaders`); what is read later is checked against them.

The output side (`run_kbnet.py --save_outputs`, reference src/kbnet.py:986-1026): `save_depth` / `save_depth_batch` for one tensor,
and `OutputWriter` for the whole export of a run -- `ops.export_pack` makes the pixels of a batch's files in one launch, a side
stream copies them to pinned slots, host threads encode and write while the next batch runs (kb.inference.run drives it).
`read_paths`, `write_paths` and `load_depth_with_validity_map` are the reference's data_utils functions of those names.

Point clouds: `PointCloudWriter` takes the same road for the depth maps backprojected to metric 3-D points --
`ops.point_cloud` writes the vertex records of binary PLY files on the device, the side stream copies them, host threads only write;
`ply_header` and `load_point_cloud` are the format and its strict reader.
"""

from __future__ import annotations

import ctypes as C
import os
import threading
from concurrent.futures import Future, ThreadPoolExecutor
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.utils.data

from . import _lib, ops
from ._lib import KbnError, check
from .dist import shard_bounds


# ------------------------------------------------------------------------- PNG decode
def png_info(data: bytes) -> Tuple[int, int, int, int]:
    """(width, height, channels, bit_depth) of a PNG file held in memory."""
    lib = _lib.load()
    w, h, c, b = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    check(lib.kbn_png_info(data, len(data), C.byref(w), C.byref(h), C.byref(c), C.byref(b)), "kbn_png_info")
    return w.value, h.value, c.value, b.value


def decode_png(data: bytes, out: Optional[np.ndarray] = None) -> np.ndarray:
    """PNG bytes -> H x W x C uint8 (H x W for gray) or H x W uint16 array; decodes into `out` if given
    (any C-contiguous buffer of the right size, e.g. the numpy view of a pinned tensor)."""
    lib = _lib.load()
    w, h, c, b = png_info(data)
    dtype = np.uint16 if b == 16 else np.uint8
    shape = (h, w) if c == 1 else (h, w, c)
    if out is None:
        out = np.empty(shape, dtype=dtype)
    if out.nbytes < h * w * c * dtype().itemsize or not out.flags["C_CONTIGUOUS"]:
        raise KbnError("decode_png: output buffer too small or not contiguous")
    check(lib.kbn_png_decode(data, len(data), out.ctypes.data_as(C.c_void_p), out.nbytes), "kbn_png_decode")
    return out


def decode_png_batch(files: Sequence[bytes], outs: Sequence[np.ndarray], threads: int = 8) -> None:
    """Decodes files[i] into outs[i] (C-contiguous numpy buffers of the right size) on `threads` host
    threads inside the library (`kbn_png_decode_batch`); raises on the first damaged file."""
    lib = _lib.load()
    n = len(files)
    if n != len(outs):
        raise KbnError("decode_png_batch: one output buffer per file")
    for o in outs:
        if not o.flags["C_CONTIGUOUS"]:
            raise KbnError("decode_png_batch: output buffers must be contiguous")
    fptr = (C.c_char_p * n)(*files)
    flen = (C.c_size_t * n)(*[len(f) for f in files])
    optr = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    olen = (C.c_size_t * n)(*[o.nbytes for o in outs])
    status = (C.c_int * n)()
    check(lib.kbn_png_decode_batch(fptr, flen, optr, olen, n, int(threads), status), "kbn_png_decode_batch")


def _read(path: str) -> bytes:
    with open(path, "rb") as f:
        return f.read()


# ------------------------------------------------------------------ the packed frame store
FRAME_MAGIC = b"KBNFRM1\0"      # a packed frame's first 8 bytes: the loaders tell it from a PNG by these, not by its name
FRAME_HEADER_BYTES = 32


def is_packed_frame(head: bytes) -> bool:
    """Whether a file that begins with `head` is a packed frame."""
    return bytes(head[:8]) == FRAME_MAGIC


def frame_info(data: bytes) -> Tuple[int, int, int, int]:
    """(width, height, channels, bits) of a packed frame; its first 32 bytes are enough."""
    w, h, c, b = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    check(_lib.load().kbn_frame_info(bytes(data), len(data), C.byref(w), C.byref(h), C.byref(c), C.byref(b)), "kbn_frame_info")
    return w.value, h.value, c.value, b.value


def check_frame(data) -> None:
    """kbn_frame_check: raises KbnError unless `data` (bytes, or a C-contiguous uint8 array such as a slice of pinned staging) is a
    structurally complete packed frame -- the check every file passes before its bytes may reach ops.unpack_packed_frames."""
    if isinstance(data, np.ndarray):
        if data.dtype != np.uint8 or not data.flags["C_CONTIGUOUS"]:
            raise KbnError("check_frame: expected a contiguous uint8 array")
        check(_lib.load().kbn_frame_check(data.ctypes.data_as(C.c_void_p), data.nbytes), "kbn_frame_check")
    else:
        check(_lib.load().kbn_frame_check(bytes(data), len(data)), "kbn_frame_check")


def encode_frame(array: np.ndarray) -> bytes:
    """H x W or H x W x C (C = 1, 3, 4) uint8 / uint16 samples -> the bytes of a packed frame (kbn_frame_encode): lossless, and
    decodable on the device.  ctypes drops the interpreter lock around the encoder."""
    a = np.ascontiguousarray(array)
    if a.dtype not in (np.uint8, np.uint16) or a.ndim not in (2, 3):
        raise KbnError(f"encode_frame: expected an H x W (x C) uint8 or uint16 array, got {a.dtype} {a.shape}")
    h, w = a.shape[:2]
    c = a.shape[2] if a.ndim == 3 else 1
    bits = 8 * a.dtype.itemsize
    lib = _lib.load()
    cap = lib.kbn_frame_encode_bound(w, h, c, bits)
    if cap == 0:
        raise KbnError(f"encode_frame: {h} x {w} x {c} samples of {bits} bits cannot be packed (channels 1, 3 or 4, sizes >= 1)")
    buf = getattr(_scratch, "frame", None)
    if buf is None or len(buf) < cap:
        buf = _scratch.frame = (C.c_ubyte * cap)()
    n = C.c_size_t()
    check(lib.kbn_frame_encode(a.ctypes.data_as(C.c_void_p), w, h, c, bits, buf, len(buf), C.byref(n)), "kbn_frame_encode")
    return bytes(memoryview(buf)[:n.value])


def decode_frame(data: bytes, out: Optional[np.ndarray] = None) -> np.ndarray:
    """The bytes of a packed frame -> H x W x C uint8 / uint16 (H x W for one channel), as decode_png returns a PNG's pixels:
    the host decoder (kbn_frame_decode; it runs kbn_frame_check first)."""
    w, h, c, b = frame_info(data[:FRAME_HEADER_BYTES])
    dtype = np.uint16 if b == 16 else np.uint8
    if out is None:
        out = np.empty((h, w) if c == 1 else (h, w, c), dtype=dtype)
    if out.nbytes < h * w * c * dtype().itemsize or not out.flags["C_CONTIGUOUS"]:
        raise KbnError("decode_frame: output buffer too small or not contiguous")
    check(_lib.load().kbn_frame_decode(bytes(data), len(data), out.ctypes.data_as(C.c_void_p), out.nbytes), "kbn_frame_decode")
    return out


def pack_frames(src_png_paths: Sequence[str], dst_paths: Sequence[str], workers: int = 8) -> Tuple[int, int]:
    """Converts PNG files to packed frames, src_png_paths[i] -> dst_paths[i], on `workers` host threads: decoded with the library's
    PNG reader (a palette becomes RGB), encoded with kbn_frame_encode, written under a temporary name and moved into place.
    A source may be a sequence entry (split_sample); its destination is then one too, frame for frame, and a frame that several
    entries name is converted once (map_sample rewrites the entries of a list).  Returns (PNG bytes read, packed bytes written)."""
    if len(src_png_paths) != len(dst_paths):
        raise KbnError(f"pack_frames: {len(src_png_paths)} sources, {len(dst_paths)} destinations")
    if any("\t" in entry for entry in src_png_paths):
        pairs = {}
        for src, dst in zip(src_png_paths, dst_paths):
            srcs, dsts = split_sample(src), split_sample(dst)
            if (srcs is None) != (dsts is None):
                raise KbnError(f"pack_frames: {src!r} and its destination {dst!r} must both be one path or both three")
            for pair in zip(srcs or (src,), dsts or (dst,)):
                pairs[pair] = None
        src_png_paths, dst_paths = [a for a, _ in pairs], [b for _, b in pairs]

    def one(pair):
        src, dst = pair
        png = _read(src)
        data = encode_frame(decode_png(png))
        os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
        tmp = f"{dst}.tmp{os.getpid()}.{threading.get_ident()}"
        with open(tmp, "wb") as f:
            f.write(data)
        os.replace(tmp, dst)
        return len(png), len(data)

    with ThreadPoolExecutor(max_workers=max(1, int(workers))) as ex:
        sizes = list(ex.map(one, zip(src_png_paths, dst_paths)))
    return sum(s[0] for s in sizes), sum(s[1] for s in sizes)


# ------------------------------------------------------------------ sequence entries
def split_sample(entry: str):
    """An entry of an image path list -> (previous, current, next) where it names its three frames, `previous<TAB>current<TAB>next`
    (the left-to-right order of the reference's triplet file, load_image_triplet, src/datasets.py:22-46: image1, image0, image2);
    None for a plain path, a triplet file's.  Two or four fields, or an empty one, raise KbnError."""
    if "\t" not in entry:
        return None
    fields = entry.split("\t")
    if len(fields) != 3 or not all(fields):
        raise KbnError(f"a sample names one triplet file, or previous<TAB>current<TAB>next: {entry!r}")
    return tuple(fields)


def sample_name(entry: str) -> str:
    """The path an output or log name of a sample derives from: `current` of a sequence entry, the entry itself otherwise."""
    fields = split_sample(entry)
    return entry if fields is None else fields[1]


def map_sample(entry: str, fn) -> str:
    """`entry` with `fn` applied to its path, or to each of a sequence entry's three."""
    fields = split_sample(entry)
    return fn(entry) if fields is None else "\t".join(fn(path) for path in fields)


def sequence_lines(frame_paths: Sequence[str], window: int = 1, ends: str = "drop") -> List[str]:
    """The sequence entries of one ordered sequence of frames: frame idx with its neighbours idx - window and idx + window.
    ends "drop": frames without both neighbours are left out (the reference's NYUv2 rule, range(w, n - w)); "repeat": the frame
    itself stands in for a missing neighbour.  window 0: `p<TAB>p<TAB>p`, the reference's validation and testing images."""
    window = int(window)
    if window < 0:
        raise KbnError(f"sequence_lines: window {window}")
    if ends not in ("drop", "repeat"):
        raise KbnError(f"sequence_lines: ends {ends!r}: 'drop' or 'repeat'")
    paths = list(frame_paths)
    n = len(paths)
    for path in paths:
        if not path or "\t" in path or "\n" in path:
            raise KbnError(f"sequence_lines: {path!r} cannot be a field of an entry")
    lines = []
    for idx in range(window, n - window) if ends == "drop" else range(n):
        before, after = idx - window, idx + window
        lines.append("\t".join((paths[before] if before >= 0 else paths[idx], paths[idx], paths[after] if after < n else paths[idx])))
    return lines


def _batch_entries(entries: Sequence[str], what: str):
    """split_sample of a batch's image entries: a list of (previous, current, next), or None where all are triplet files; a batch
    that mixes the two raises, naming one of each."""
    fields = [split_sample(entry) for entry in entries]
    for entry, f in zip(entries, fields):
        if (f is None) != (fields[0] is None):
            form = {True: "a triplet file", False: "a sequence entry"}
            raise KbnError(f"{what}: a batch must be all triplet files or all sequence entries: {entries[0]!r} is {form[fields[0] is None]}, "
                           f"{entry!r} is {form[f is None]}")
    return None if fields[0] is None else fields


def _image_info(head: bytes) -> Tuple[int, int, int, int]:
    """png_info or frame_info of a file's first 33 bytes, by its magic."""
    return frame_info(head[:FRAME_HEADER_BYTES]) if is_packed_frame(head) else png_info(head)


def _read_packed_into(pool, jobs: Sequence[tuple]) -> None:
    """jobs: (path, pinned flat uint8 numpy view, offset, size, (width, height, channels, bits) the batch was planned with).  Each
    file is read straight into view[offset:offset + size] on the pool's threads, and kbn_frame_check runs on the bytes where they
    lie: no file's bytes are copied to the device before it has passed."""
    def one(job):
        path, flat, at, size, want = job
        dst = flat[at:at + size]
        view, got = memoryview(dst), 0
        with open(path, "rb", buffering=0) as f:
            while got < size:
                step = f.readinto(view[got:])
                if not step:
                    break
                got += step
            more = f.read(1)
        if got != size or more:
            raise KbnError(f"{path} changed size while it was read")
        check_frame(dst)
        if frame_info(dst[:FRAME_HEADER_BYTES].tobytes()) != tuple(want):
            raise KbnError(f"{path} is not the {want[1]} x {want[0]} x {want[2]} frame of {want[3]} bits its batch was planned with")

    list(pool.map(one, jobs))


def _one_kind(paths: Sequence[str], flags: Sequence[bool], what: str) -> bool:
    """Whether a batch's files are packed frames (all of them) or PNGs (all of them); a mixed batch raises, naming two paths."""
    for path, flag in zip(paths, flags):
        if flag != flags[0]:
            kind = {True: "a packed frame", False: "a PNG"}
            raise KbnError(f"{what}: a batch must be all PNG or all packed: {paths[0]} is {kind[flags[0]]}, {path} is {kind[flag]}")
    return bool(flags[0])


class _FileHeaders(dict):
    """path -> ((width, height, channels, bits), whether the file is a packed frame), from its first 33 bytes, read once a path."""

    def __missing__(self, path: str):
        with open(path, "rb") as f:
            head = f.read(33)                            # a PNG's signature + IHDR; a packed frame's header is its first 32
        self[path] = (_image_info(head), is_packed_frame(head))
        return self[path]


def _layout(sizes: Sequence[int], images: Optional[int] = None) -> Tuple[List[int], List[int]]:
    """The files of a batch -- its `images` image files (half of them by default), then its depth maps -- laid out in the two flat
    staging buffers, each file at a 16-byte-aligned offset: the offsets, and the bytes the image and the depth buffer need."""
    ni = len(sizes) // 2 if images is None else images
    at, total = [], [0, 0]
    for j, size in enumerate(sizes):
        at.append(total[j >= ni])
        total[j >= ni] = _align16(total[j >= ni] + size)
    return at, total


def _places(st: dict, at: Sequence[int], sizes: Sequence[int], images: Optional[int] = None) -> List[tuple]:
    """(flat pinned numpy view, offset, size) of every file of a batch -- images, then depth maps -- in the staging set `st`."""
    ni = len(at) // 2 if images is None else images
    return list(zip([st["image"].numpy()] * ni + [st["depth"].numpy()] * (len(at) - ni), at, sizes))


def _packed_jobs(st: dict, paths, at, sizes, want, images: Optional[int] = None) -> List[tuple]:
    """_read_packed_into's jobs for the files `paths`, planned with the headers `want`, at _layout's offsets."""
    return [(path, view, a, size, w) for path, (view, a, size), w in zip(paths, _places(st, at, sizes, images), want)]


def _load_intrinsics(st: dict, paths: Sequence[str], starts=None) -> None:
    """The 3 x 3 matrices of `paths` into the set's pinned `k` block, each moved with its crop where `starts` gives the crops'
    (y_start, x_start)."""
    k_np = st["k"].numpy()
    for j, path in enumerate(paths):
        k = np.load(path).astype(np.float32)
        k_np[j] = k if starts is None else _crop_intrinsics(k, *starts[j]).astype(np.float32)


class _Staging:
    """The pinned staging sets of a loader, one per slot (prefetch + 1 of them), whatever kind of file a batch holds: flat uint8
    buffers `image` and `depth`, grown when a batch needs more, a `k` block of max(frames, batch_size) x 3 x 3 floats, and `done`,
    the event of the copies that last used the set."""

    def __init__(self, slots: int, batch_size: int, device, copy_stream):
        self.batch_size, self.device, self.copy_stream = batch_size, device, copy_stream
        self._sets = [{"image": None, "depth": None, "k": None, "done": None} for _ in range(slots)]

    def acquire(self, slot: int, image_bytes: int, depth_bytes: int, frames: int) -> dict:
        st = self._sets[slot]
        if st["done"] is not None:
            st["done"].synchronize()      # the copies that last used this staging set: it is not reused, let alone replaced, before
        for name, need in (("image", image_bytes), ("depth", depth_bytes)):
            if st[name] is None or st[name].numel() < need:
                st[name] = torch.empty(need + need // 8, dtype=torch.uint8).pin_memory()     # some room: the next batch's frames differ a little
        if st["k"] is None or st["k"].shape[0] < max(frames, self.batch_size):
            st["k"] = torch.empty((max(frames, self.batch_size), 3, 3), dtype=torch.float32).pin_memory()
        return st

    def submit(self, st: dict, image_bytes: int, depth_bytes: int, frames: int, unpack):
        """The set is filled: on the copy stream, the used prefix of each buffer goes to the device in one asynchronous copy,
        `unpack(images_u8, depths_u8, intrinsics)` makes the batch's tensors of them, and the set's event is recorded.
        Returns (tensors, event)."""
        with torch.cuda.stream(self.copy_stream):
            img_d = st["image"][:image_bytes].to(self.device, non_blocking=True)
            dep_d = st["depth"][:depth_bytes].to(self.device, non_blocking=True)
            k_d = st["k"][:frames].to(self.device, non_blocking=True)
            tensors = unpack(img_d, dep_d, k_d)
            done = torch.cuda.Event()
            done.record(self.copy_stream)
        st["done"] = done
        return tensors, done


# ---------------------------------------------- the reference's loader functions (numpy)
def _decode_file(path: str) -> np.ndarray:
    """The pixels of one PNG or packed file, told apart by the magic: the same array from either."""
    data = _read(path)
    return decode_frame(data) if is_packed_frame(data) else decode_png(data)


def load_image(path: str, normalize: bool = True, data_format: str = "HWC") -> np.ndarray:
    """reference src/data_utils.py:58-85 (`Image.open(path).convert('RGB')` -> float32); a packed frame is read like the PNG."""
    px = _decode_file(path)
    if px.dtype != np.uint8:
        raise KbnError("load_image: 16-bit images are not supported")
    if px.ndim == 2:
        px = np.repeat(px[:, :, None], 3, axis=2)
    image = np.asarray(px[:, :, :3], np.float32)
    if data_format == "CHW":
        image = np.transpose(image, (2, 0, 1))
    elif data_format != "HWC":
        raise ValueError("Unsupported data format: {}".format(data_format))
    return image / 255.0 if normalize else image


def load_image_triplet(path: str, normalize: bool = True):
    """reference src/datasets.py:22-46: images at t-1, t, t+1 (C x H x W each) -> (t, t-1, t+1) order."""
    images = load_image(path, normalize=normalize, data_format="CHW")
    image1, image0, image2 = np.split(images, indices_or_sections=3, axis=-1)
    return image1, image0, image2


def load_depth(path: str, data_format: str = "HW") -> np.ndarray:
    """reference src/data_utils.py:123-152: 16-bit PNG (or packed frame) / 256, non-positive values -> 0."""
    z = np.array(_decode_file(path), dtype=np.float32)
    if z.ndim != 2:
        raise KbnError("load_depth: expected a single-channel PNG or packed frame")
    z = z / 256.0
    z[z <= 0] = 0.0
    if data_format == "HW":
        pass
    elif data_format == "CHW":
        z = np.expand_dims(z, axis=0)
    elif data_format == "HWC":
        z = np.expand_dims(z, axis=-1)
    else:
        raise ValueError("Unsupported data format: {}".format(data_format))
    return z


def load_depth_with_validity_map(path: str, data_format: str = "HW"):
    """reference src/data_utils.py:87-121: (depth, validity map) of a 16-bit PNG -- sample / 256, and 1 where that is positive --
    as float32 H x W ('HW'), 1 x H x W ('CHW') or H x W x 1 ('HWC')."""
    z = load_depth(path, data_format="HW")
    v = z.astype(np.float32)
    v[z > 0] = 1.0
    if data_format == "HW":
        pass
    elif data_format == "CHW":
        z, v = np.expand_dims(z, axis=0), np.expand_dims(v, axis=0)
    elif data_format == "HWC":
        z, v = np.expand_dims(z, axis=-1), np.expand_dims(v, axis=-1)
    else:
        raise ValueError("Unsupported data format: {}".format(data_format))
    return z, v


def read_paths(filepath: str) -> List[str]:
    """reference src/data_utils.py:21-41: the lines of a newline-delimited file of paths, up to the first empty line."""
    path_list = []
    with open(filepath) as f:
        while True:
            path = f.readline().rstrip("\n")
            if path == "":      # nothing more to read, or an empty line: the reference stops at either
                break
            path_list.append(path)
    return path_list


def write_paths(filepath: str, paths: Sequence[str]) -> None:
    """reference src/data_utils.py:43-56: one path a line."""
    with open(filepath, "w") as o:
        for idx in range(len(paths)):
            o.write(paths[idx] + "\n")


# ---------------------------------------------------------------------- output side
_scratch = threading.local()    # one encode buffer per host thread, grown as needed: an OutputWriter worker allocates nothing per file


def _encode_png(kind: str, pixels: np.ndarray, width: int, height: int, level: int) -> memoryview:
    """The PNG file image of C-contiguous pixels, as a view of the calling thread's scratch buffer: valid until that thread encodes
    again.  kind: 'gray16' (H x W uint16), 'rgb8' (H x W x 3 uint8) or 'gray8' (H x W uint8).  ctypes drops the interpreter lock around the encoder."""
    lib = _lib.load()
    cap = getattr(lib, f"kbn_png_encode_{kind}_bound")(width, height)
    buf = getattr(_scratch, "buf", None)
    if buf is None or len(buf) < cap:
        buf = _scratch.buf = (C.c_ubyte * cap)()
    n = C.c_size_t()
    check(getattr(lib, f"kbn_png_encode_{kind}")(pixels.ctypes.data_as(C.c_void_p), width, height, buf, len(buf), C.byref(n), int(level)),
          f"kbn_png_encode_{kind}")
    return memoryview(buf)[:n.value]


def encode_image_png(rgb_u8: np.ndarray, level: int = 6) -> bytes:
    """H x W x 3 uint8 pixels -> the bytes of an 8-bit RGB PNG (kbn_png_encode_rgb8): the file `Image.fromarray(rgb_u8).save(path)`
    stands for in reference src/kbnet.py:1015-1016 (the same pixels; the file's bytes are not PIL's)."""
    a = np.ascontiguousarray(rgb_u8)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise KbnError(f"encode_image_png: expected an H x W x 3 uint8 array, got {a.dtype} {a.shape}")
    return bytes(_encode_png("rgb8", a, a.shape[1], a.shape[0], level))


def encode_depth_png(samples: np.ndarray, level: int = 6) -> bytes:
    """H x W uint16 samples (depth * 256) -> the bytes of a 16-bit grayscale PNG (kbn_png_encode_gray16)."""
    a = np.ascontiguousarray(samples, dtype=np.uint16)
    if a.ndim != 2:
        raise KbnError("encode_depth_png: expected an H x W array")
    return bytes(_encode_png("gray16", a, a.shape[1], a.shape[0], level))


def unpack_frames(src_packed_paths: Sequence[str], dst_png_paths: Sequence[str], workers: int = 8, level: int = 6) -> Tuple[int, int]:
    """The inverse of pack_frames: packed frames to PNG files, src_packed_paths[i] -> dst_png_paths[i], on `workers` host threads --
    decoded on the host (kbn_frame_decode, after kbn_frame_check), encoded with the native PNG encoders, written under a temporary
    name and moved into place.  8-bit RGB, 8-bit gray and 16-bit gray frames; any other format raises KbnError naming the file.
    Returns (packed bytes read, PNG bytes written)."""
    if len(src_packed_paths) != len(dst_png_paths):
        raise KbnError(f"unpack_frames: {len(src_packed_paths)} sources, {len(dst_png_paths)} destinations")
    kinds = {(3, 8): "rgb8", (1, 8): "gray8", (1, 16): "gray16"}

    def one(pair):
        src, dst = pair
        data = _read(src)
        if not is_packed_frame(data):
            raise KbnError(f"unpack_frames: {src} is not a packed frame")
        w, h, c, bits = frame_info(data[:FRAME_HEADER_BYTES])
        if (c, bits) not in kinds:
            raise KbnError(f"unpack_frames: {src} holds {c} channels of {bits} bits; 8-bit RGB, 8-bit gray and 16-bit gray become PNGs")
        png = bytes(_encode_png(kinds[(c, bits)], decode_frame(data), w, h, level))
        os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
        tmp = f"{dst}.tmp{os.getpid()}.{threading.get_ident()}"
        with open(tmp, "wb") as f:
            f.write(png)
        os.replace(tmp, dst)
        return len(data), len(png)

    with ThreadPoolExecutor(max_workers=max(1, int(workers))) as ex:
        sizes = list(ex.map(one, zip(src_packed_paths, dst_png_paths)))
    return sum(s[0] for s in sizes), sum(s[1] for s in sizes)


def depth_samples(z) -> np.ndarray:
    """What reference src/data_utils.py:165-167 stores for a depth map: np.uint32(z * 256.0), clipped to the PNG's 16 bits as PIL
    clips a mode 'I' image -- as uint16.  `z`: a numpy array (converted here) or a device tensor of any shape
    (kbn_depth_to_u16_forward, then one device-to-host copy of 2 bytes per pixel)."""
    if torch.is_tensor(z) and z.is_cuda:
        zc = z.detach().contiguous().float()
        out = torch.empty(zc.shape, device=zc.device, dtype=torch.int16)
        with torch.cuda.device(zc.device):
            check(_lib.load().kbn_depth_to_u16_forward(zc.data_ptr(), out.data_ptr(), zc.numel(),
                                                       torch.cuda.current_stream().cuda_stream), "kbn_depth_to_u16_forward")
        return out.cpu().numpy().view(np.uint16)
    a = np.asarray(z.detach().cpu().numpy() if torch.is_tensor(z) else z, dtype=np.float32) * np.float32(256.0)
    return np.clip(np.nan_to_num(a, nan=0.0), 0.0, 65535.0).astype(np.uint32).astype(np.uint16)


def save_depth(z, path: str) -> None:
    """reference src/data_utils.py:154-167: a depth map (H x W, numpy or tensor) as a 16-bit PNG holding depth * 256."""
    s = depth_samples(z)
    s = s.reshape(s.shape[-2:]) if s.ndim > 2 and int(np.prod(s.shape[:-2])) == 1 else s
    with open(path, "wb") as f:
        f.write(encode_depth_png(s))


def save_depth_batch(z: torch.Tensor, paths: Sequence[str], threads: int = 8) -> None:
    """N x 1 x H x W (or N x H x W) depth maps -> one PNG each (run_kbnet.py --save_outputs, reference src/kbnet.py:1018-1026): ONE
    device pass and copy for the batch, the files encoded and written by `threads` host threads (the encoder runs without the GIL)."""
    s = depth_samples(z)
    s = s.reshape((-1,) + s.shape[-2:])
    if s.shape[0] != len(paths):
        raise KbnError(f"save_depth_batch: {s.shape[0]} maps, {len(paths)} paths")

    def one(i):
        with open(paths[i], "wb") as f:
            f.write(encode_depth_png(s[i]))

    with ThreadPoolExecutor(max_workers=max(1, int(threads))) as ex:
        list(ex.map(one, range(len(paths))))


OUTPUT_DIRECTORIES = ("image", "output_depth", "sparse_depth", "ground_truth")     # reference src/kbnet.py:991-1001
OUTPUT_FORMATS = ("png", "packed")      # OutputWriter's file_format, inference.run_with_format's output_format
PACKED_EXTENSION = ".kbf"


def packed_filename(filename: str) -> str:
    """The name OutputWriter(file_format="packed") gives the file that would be the PNG `filename`: its extension replaced."""
    return os.path.splitext(filename)[0] + PACKED_EXTENSION


def image_export_affine(normalized_image_range) -> Tuple[float, float]:
    """(scale, shift) that turn an image normalised to this range (ops.preprocess) back into 0..255: [0, 1] -> (255, 0), the
    reference's `255 * image`; [-1, 1] -> (127.5, 127.5); [0, 255] -> (1, 0).  For the last two the reference still multiplies by
    255 and casts what no longer fits a uint8; its files hold garbage there.  Any other range: ValueError, as ops.preprocess."""
    rng = [float(v) for v in normalized_image_range]
    if rng == [0.0, 1.0]:
        return 255.0, 0.0
    if rng == [-1.0, 1.0]:
        return 127.5, 127.5
    if rng == [0.0, 255.0]:
        return 1.0, 0.0
    raise ValueError("Unsupported normalization range: {}".format(list(normalized_image_range)))


class OutputWriter:
    """The files run_kbnet.py --save_outputs stores (reference src/kbnet.py:986-1026), written WHILE the run proceeds: per frame
    image/<name> (8-bit RGB), output_depth/<name>, sparse_depth/<name> and, where given, ground_truth/<name> (16-bit gray,
    depth * 256) under `output_path`.  All four directories are made on construction, ground_truth too when it stays empty, as in
    the reference.

    submit() costs the caller one kernel launch and no wait for the device:
      1. ONE ops.export_pack launch on torch's current stream turns the three float tensors (20 bytes a pixel) into the files'
         pixels (7 bytes a pixel) in a device buffer of the writer's own;
      2. an event is recorded there; the writer's side stream waits for it and copies the 7 bytes a pixel into one of `in_flight`
         pinned host slots;
      3. `threads` (at most 16) host threads wait for the slot's copy, encode (kbn_png_encode_rgb8 / _gray16: ctypes drops the
         interpreter lock) and write the files.
    A slot -- its device buffer and its pinned buffer -- is used again only after all its files are written; that is the only wait
    submit() knows, and it is a wait for host threads.

    What was handed to submit() may be freed or overwritten by the caller as soon as it returns: the pack has READ the device
    tensors in stream order on the stream the caller goes on using (later kernels and the allocator's reuse are ordered behind
    it), everything downstream reads the writer's own packed buffer, and `ground_truth_samples` is copied into the slot before
    submit() returns.

    file_format "packed"  writes packed frames (`<name>.kbf` where "png" writes `<name>.png`) that this package's loaders
    read back, and no host thread encodes an output: after the export_pack launch two ops.pack_frames calls on the caller's stream
    encode the RGB pixels (3 planes of 8 bits) and the 2 N planes of 16 bits into the slot's device buffer; the side stream copies
    every file's SLOT (the sizes are known to the device alone, so the bound is copied: 7.6 bytes a pixel at KITTI size, beside
    the 7 of the PNG path) and the sizes; a host thread reads its file's size, runs kbn_frame_check on the bytes where they lie,
    writes them under a temporary name and moves the file into place.  Only the ground truth's host samples are encoded on the pool (encode_frame).
    `level` is ignored.  Slot reuse, back-pressure, error delivery and the guarantee below are the same.

    close() waits for everything and raises the first error a thread met; the object is a context manager.  One writer is driven
    by one thread."""

    def __init__(self, output_path: str, threads: int = 8, in_flight: int = 2, level: int = 6, normalized_image_range=(0, 1),
                 file_format: str = "png"):
        if file_format not in OUTPUT_FORMATS:
            raise KbnError(f"OutputWriter: file_format {file_format!r}: expected one of {', '.join(repr(f) for f in OUTPUT_FORMATS)}")
        self.file_format = file_format
        self.scale, self.shift = image_export_affine(normalized_image_range)
        if not -1 <= int(level) <= 9:
            raise KbnError(f"OutputWriter: zlib level {level} (-1 .. 9)")
        self.level = int(level)
        self.output_path = output_path
        self.dirpaths = {name: os.path.join(output_path, name) for name in OUTPUT_DIRECTORIES}
        for dirpath in self.dirpaths.values():
            if not os.path.exists(dirpath):
                os.makedirs(dirpath)
        self.threads = max(1, min(16, int(threads)))
        self.pool = ThreadPoolExecutor(max_workers=self.threads)
        self._slots = [{"key": None, "files": []} for _ in range(max(1, int(in_flight)))]
        self._serial = 0
        self._error: Optional[BaseException] = None
        self._copy_stream = None
        self._closed = False

    # -- a slot: [rgb | samples of the output | samples of the sparse depth] on the device and pinned, + ground truth (host only) --
    def _slot(self, device, n: int, h: int, w: int) -> dict:
        slot = self._slots[self._serial % len(self._slots)]
        self._serial += 1
        self._drain(slot)
        key = (device, n, h, w)
        if slot["key"] is None or slot["key"][0] != device or slot["key"][2:] != (h, w) or slot["key"][1] < n:
            px = n * h * w
            at_a = _align16(3 * px)
            at_b = _align16(at_a + 2 * px)
            slot.update(key=key, at=(at_a, at_b), device=torch.empty(at_b + 2 * px, dtype=torch.uint8, device=device),
                        host=torch.empty(at_b + 2 * px, dtype=torch.uint8).pin_memory(), truth=np.empty((n, h, w), dtype=np.uint16))
            slot["device"].record_stream(self._copy_stream)      # the allocator learns that the side stream reads it
        return slot

    def _drain(self, slot: dict) -> None:
        for f in slot["files"]:
            e = f.exception()
            if e is not None and self._error is None:
                self._error = e
        slot["files"] = []

    def _views(self, slot: dict, n: int, h: int, w: int, which: str):
        capacity = slot["key"][1]
        px = capacity * h * w
        at_a, at_b = slot["at"]
        flat = slot[which]
        return (flat[:3 * px].view(capacity, h, w, 3)[:n], flat[at_a:at_a + 2 * px].view(torch.int16).view(capacity, h, w)[:n],
                flat[at_b:at_b + 2 * px].view(torch.int16).view(capacity, h, w)[:n])

    def submit(self, filenames: Sequence[str], image, output_depth, sparse_depth, ground_truth_samples=None) -> None:
        """One batch: image N x 3 x H x W as ops.preprocess normalised it, output_depth and sparse_depth N x 1 x H x W (device,
        fp32); filenames: N base names; ground_truth_samples: host uint16 N x H x W, the PNG samples as they are, or None."""
        if self._closed:
            raise KbnError("OutputWriter: submit() after close()")
        for name, t in (("image", image), ("output_depth", output_depth), ("sparse_depth", sparse_depth)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise KbnError(f"OutputWriter: {name}: expected a CUDA/HIP tensor (the HIP path has no CPU fallback)")
        n, h, w = int(image.shape[0]), int(image.shape[-2]), int(image.shape[-1])
        if len(filenames) != n:
            raise KbnError(f"OutputWriter: {n} frames, {len(filenames)} file names")
        truth = None
        if ground_truth_samples is not None:
            truth = np.asarray(ground_truth_samples)
            if truth.dtype != np.uint16 or truth.shape != (n, h, w):
                raise KbnError(f"OutputWriter: ground_truth_samples is {truth.dtype} {truth.shape}, expected uint16 {(n, h, w)}")
        device = image.device
        if self.file_format == "packed":
            return self._submit_packed(filenames, image, output_depth, sparse_depth, truth, device, n, h, w)
        with torch.cuda.device(device):
            if self._copy_stream is None or self._copy_stream.device != device:
                self._copy_stream = torch.cuda.Stream(device=device)
            slot = self._slot(device, n, h, w)
            packed = self._views(slot, n, h, w, "device")
            ops.export_pack(image, output_depth, sparse_depth, scale=self.scale, shift=self.shift, out=packed)
            ready = torch.cuda.Event()
            ready.record(torch.cuda.current_stream(device))
            self._copy_stream.wait_event(ready)
            used = slot["at"][1] + 2 * slot["key"][1] * h * w if n == slot["key"][1] else None
            with torch.cuda.stream(self._copy_stream):
                if used is not None:      # a full slot: its three parts are one range, one copy
                    slot["host"][:used].copy_(slot["device"][:used], non_blocking=True)
                else:                     # a short batch in a larger slot: the used head of each part
                    for dst, src in zip(self._views(slot, n, h, w, "host"), packed):
                        dst.copy_(src, non_blocking=True)
                done = torch.cuda.Event()
                done.record(self._copy_stream)
        if truth is not None:
            np.copyto(slot["truth"][:n], truth)
        rgb, out_s, sparse_s = (t.numpy() for t in self._views(slot, n, h, w, "host"))
        jobs = []
        for i, filename in enumerate(filenames):
            jobs.append(("rgb8", rgb[i], self.dirpaths["image"], filename))
            jobs.append(("gray16", out_s[i].view(np.uint16), self.dirpaths["output_depth"], filename))
            jobs.append(("gray16", sparse_s[i].view(np.uint16), self.dirpaths["sparse_depth"], filename))
            if truth is not None:
                jobs.append(("gray16", slot["truth"][i], self.dirpaths["ground_truth"], filename))
        slot["files"] = [self.pool.submit(self._write, done, h, w, *job) for job in jobs]

    def _write(self, done, h: int, w: int, kind: str, pixels: np.ndarray, dirpath: str, filename: str) -> None:
        done.synchronize()      # the slot's copy has landed (returns at once for all but the first file of a batch)
        data = _encode_png(kind, pixels, w, h, self.level)
        with open(os.path.join(dirpath, filename), "wb") as f:
            f.write(data)

    # -- file_format "packed": a slot holds [rgb | 2 x capacity planes of samples] on the device, and the encoded files' slots +
    #    their sizes on the device and pinned --
    def _packed_slot(self, device, n: int, h: int, w: int) -> dict:
        slot = self._slots[self._serial % len(self._slots)]
        self._serial += 1
        self._drain(slot)
        if slot["key"] is None or slot["key"][0] != device or slot["key"][2:] != (h, w) or slot["key"][1] < n:
            px = n * h * w
            at_depth = _align16(3 * px)
            strides = (ops.pack_frames_stride(h, w, 3, 8), ops.pack_frames_stride(h, w, 1, 16))
            at_files = n * strides[0]
            work = max(ops.pack_frames_workspace_bytes(n, h, w, 3, 8), ops.pack_frames_workspace_bytes(2 * n, h, w, 1, 16))
            slot.update(key=(device, n, h, w), at=at_depth, strides=strides, at_files=at_files,
                        pixels=torch.empty(at_depth + 4 * px, dtype=torch.uint8, device=device),
                        device=torch.empty(at_files + 2 * n * strides[1], dtype=torch.uint8, device=device),
                        sizes=torch.empty(3 * n, dtype=torch.int64, device=device),
                        workspace=torch.empty(work, dtype=torch.uint8, device=device),
                        host=torch.empty(at_files + 2 * n * strides[1], dtype=torch.uint8).pin_memory(),
                        host_sizes=torch.empty(3 * n, dtype=torch.int64).pin_memory(), truth=np.empty((n, h, w), dtype=np.uint16))
            for name in ("device", "sizes"):
                slot[name].record_stream(self._copy_stream)      # the allocator learns that the side stream reads them
        return slot

    def _submit_packed(self, filenames, image, output_depth, sparse_depth, truth, device, n: int, h: int, w: int) -> None:
        with torch.cuda.device(device):
            if self._copy_stream is None or self._copy_stream.device != device:
                self._copy_stream = torch.cuda.Stream(device=device)
            slot = self._packed_slot(device, n, h, w)
            capacity, px = slot["key"][1], n * h * w
            s_rgb, s_depth = slot["strides"]
            rgb = slot["pixels"][:3 * px].view(n, h, w, 3)
            planes = slot["pixels"][slot["at"]:slot["at"] + 4 * px].view(torch.int16).view(2 * n, h, w)      # output depth, then sparse depth
            ops.export_pack(image, output_depth, sparse_depth, scale=self.scale, shift=self.shift, out=(rgb, planes[:n], planes[n:]))
            files = {which: slot[which][:capacity * s_rgb].view(capacity, s_rgb)[:n] for which in ("device", "host")}
            depth_files = {which: slot[which][slot["at_files"]:].view(2 * capacity, s_depth)[:2 * n] for which in ("device", "host")}
            ops.pack_frames(rgb, out=files["device"], out_bytes=slot["sizes"][:n], workspace=slot["workspace"])
            ops.pack_frames(planes, out=depth_files["device"], out_bytes=slot["sizes"][n:3 * n], workspace=slot["workspace"])
            ready = torch.cuda.Event()
            ready.record(torch.cuda.current_stream(device))
            self._copy_stream.wait_event(ready)
            with torch.cuda.stream(self._copy_stream):
                files["host"].copy_(files["device"], non_blocking=True)
                depth_files["host"].copy_(depth_files["device"], non_blocking=True)
                slot["host_sizes"][:3 * n].copy_(slot["sizes"][:3 * n], non_blocking=True)
                done = torch.cuda.Event()
                done.record(self._copy_stream)
        if truth is not None:
            np.copyto(slot["truth"][:n], truth)
        sizes = slot["host_sizes"].numpy()
        rgb_host, depth_host = files["host"].numpy(), depth_files["host"].numpy()
        jobs = []
        for i, filename in enumerate(filenames):
            name = packed_filename(filename)
            jobs.append((self._write_packed, done, rgb_host[i], sizes, i, os.path.join(self.dirpaths["image"], name)))
            jobs.append((self._write_packed, done, depth_host[i], sizes, n + i, os.path.join(self.dirpaths["output_depth"], name)))
            jobs.append((self._write_packed, done, depth_host[n + i], sizes, 2 * n + i, os.path.join(self.dirpaths["sparse_depth"], name)))
            if truth is not None:
                jobs.append((self._write_truth_packed, slot["truth"][i], os.path.join(self.dirpaths["ground_truth"], name)))
        slot["files"] = [self.pool.submit(*job) for job in jobs]

    @staticmethod
    def _place(data, path: str) -> None:
        tmp = f"{path}.tmp{os.getpid()}.{threading.get_ident()}"
        with open(tmp, "wb") as f:
            f.write(data)
        os.replace(tmp, path)

    def _write_packed(self, done, file_slot: np.ndarray, sizes: np.ndarray, index: int, path: str) -> None:
        done.synchronize()      # the slot's copies have landed: the file's bytes and its size
        size = int(sizes[index])
        if not FRAME_HEADER_BYTES <= size <= file_slot.shape[0]:
            raise KbnError(f"OutputWriter: the device encoder reports {size} bytes for {path}, its slot holds {file_slot.shape[0]}")
        data = file_slot[:size]
        check_frame(data)       # where the bytes lie
        self._place(data, path)

    def _write_truth_packed(self, samples: np.ndarray, path: str) -> None:
        self._place(encode_frame(samples), path)

    def close(self) -> None:
        """Waits for every file; raises the first error a thread met (once)."""
        if not self._closed:
            self._closed = True
            for slot in self._slots:
                self._drain(slot)
            self.pool.shutdown(wait=True)
        error, self._error = self._error, None
        if error is not None:
            raise error

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


# ------------------------------------------------------------------------- point clouds
POINT_CLOUD_EXTENSION = ".ply"
POINT_CLOUDS = ("output_depth", "sparse_depth")      # what PointCloudWriter and inference.run_with_point_clouds can backproject
POINT_CLOUD_DIRECTORIES = {"output_depth": "point_cloud", "sparse_depth": "sparse_point_cloud"}
_PLY_RECORD = {True: np.dtype([("xyz", "<f4", (3,)), ("rgb", "u1", (3,))]), False: np.dtype([("xyz", "<f4", (3,))])}      # packed: 15 and 12 bytes


def point_cloud_filename(filename: str) -> str:
    """The name PointCloudWriter gives the cloud of the frame whose PNG is `filename`: its extension replaced."""
    return os.path.splitext(filename)[0] + POINT_CLOUD_EXTENSION


def point_cloud_names(clouds) -> Tuple[str, ...]:
    """`clouds` as a tuple, once it is known to be a non-empty subset of POINT_CLOUDS without repeats; KbnError otherwise."""
    names = (clouds,) if isinstance(clouds, str) else tuple(clouds) if isinstance(clouds, (tuple, list)) else ()
    if not names or len(set(names)) != len(names) or any(name not in POINT_CLOUDS for name in names):
        raise KbnError(f"point clouds {clouds!r}: expected a non-empty selection of {', '.join(repr(c) for c in POINT_CLOUDS)}")
    return names


def ply_header(points: int, colour: bool) -> bytes:
    """The header of the binary PLY files PointCloudWriter writes: fixed ASCII text, `points` vertices of float x, y, z and, with
    `colour`, uchar red, green, blue.  The body is points x (15 or 12) bytes, packed, little-endian."""
    points = int(points)
    if points < 0:
        raise KbnError(f"ply_header: {points} points")
    lines = ["ply", "format binary_little_endian 1.0", "comment kbnet_amd point cloud: camera frame, metres", f"element vertex {points}",
             "property float x", "property float y", "property float z"]
    if colour:
        lines += ["property uchar red", "property uchar green", "property uchar blue"]
    return ("\n".join(lines + ["end_header"]) + "\n").encode("ascii")


def load_point_cloud(path: str):
    """A file PointCloudWriter wrote -> (xyz float32 M x 3, rgb uint8 M x 3 or None).  A strict reader of exactly those files: another
    header (any other PLY included), a truncated body or trailing bytes raise KbnError."""
    data = _read(path)
    end = data.find(b"end_header\n")
    lines = data[:end].split(b"\n") if end >= 0 else []
    count = lines[3][len(b"element vertex "):] if len(lines) > 3 and lines[3].startswith(b"element vertex ") else b""
    if not count.isdigit() or len(count) > 18:
        raise KbnError(f"load_point_cloud: {path} does not start with the header ply_header writes")
    points = int(count)
    for colour in (True, False):
        header = ply_header(points, colour)
        if data.startswith(header):
            break
    else:
        raise KbnError(f"load_point_cloud: {path} does not start with the header ply_header writes")
    record = _PLY_RECORD[colour]
    body = len(data) - len(header)
    if body != points * record.itemsize:
        raise KbnError(f"load_point_cloud: {path} states {points} points of {record.itemsize} bytes, its body holds {body} bytes")
    vertices = np.frombuffer(data, dtype=record, count=points, offset=len(header))
    return np.ascontiguousarray(vertices["xyz"]), (np.ascontiguousarray(vertices["rgb"]) if colour else None)


class PointCloudWriter:
    """Metric point clouds of a run, written WHILE it proceeds: per frame and requested cloud a binary little-endian PLY file (ply_header;
    load_point_cloud reads it back) of the pixels whose depth is finite, above 0 and inside `depth_range`, in row-major pixel order,
    in the camera frame, in metres, coloured with the image file's pixels.  `clouds` is a non-empty selection of "output_depth" (the
    network's depth: output_path/point_cloud/<name>.ply) and "sparse_depth" (the points that went in:
    output_path/sparse_point_cloud/<name>.ply); their directories are made on construction.  depth_range: (min, max), closed; None
    keeps every finite depth above 0.

    submit() costs the caller two or three launches of three kernels and no wait for the device:
      1. ONE ops.intrinsics_inverse call and ONE ops.point_cloud call per requested cloud, on torch's current stream, write the
         files' vertex records into a device buffer of the writer's own, and their numbers;
      2. an event is recorded there; the writer's side stream waits for it and copies every frame's SLOT and the counts into one of
         `in_flight` pinned host slots.  Only the device knows how many points a frame keeps, so the bound is copied, as in
         OutputWriter's packed path: 15 bytes a pixel and cloud, against the 7 of the PNG path, whatever the density;
      3. `threads` (at most 16) host threads wait for the slot's copy, then write the header and count x 15 bytes under a temporary
         name and move the file into place.
    Slot reuse, back-pressure, error delivery, close() and the context manager are OutputWriter's, and so is the guarantee: what was
    handed to submit() may be freed or overwritten as soon as it returns.  One writer is driven by one thread."""

    RECORD = 15

    def __init__(self, output_path: str, clouds=("output_depth",), threads: int = 8, in_flight: int = 2, normalized_image_range=(0, 1),
                 depth_range=None):
        self.clouds = point_cloud_names(clouds)
        self.scale, self.shift = image_export_affine(normalized_image_range)
        self.min_depth, self.max_depth = (0.0, float("inf")) if depth_range is None else (float(v) for v in depth_range)
        if not self.min_depth <= self.max_depth:
            raise KbnError(f"PointCloudWriter: depth_range {depth_range!r}: expected (min, max) with min <= max, or None")
        self.output_path = output_path
        self.dirpaths = {name: os.path.join(output_path, POINT_CLOUD_DIRECTORIES[name]) for name in self.clouds}
        for dirpath in self.dirpaths.values():
            os.makedirs(dirpath, exist_ok=True)
        self.threads = max(1, min(16, int(threads)))
        self.pool = ThreadPoolExecutor(max_workers=self.threads)
        self._slots = [{"key": None, "files": []} for _ in range(max(1, int(in_flight)))]
        self._serial = 0
        self._error: Optional[BaseException] = None
        self._copy_stream = None
        self._closed = False

    # OutputWriter's helpers, shared: a slot's finished files and their first error, a file placed under a temporary name, the end
    _drain = OutputWriter._drain
    _place = staticmethod(OutputWriter._place)
    close = OutputWriter.close
    __enter__ = OutputWriter.__enter__
    __exit__ = OutputWriter.__exit__

    # -- a slot: len(clouds) x capacity file slots of `stride` bytes and as many counts, on the device and pinned --
    def _slot(self, device, n: int, h: int, w: int) -> dict:
        slot = self._slots[self._serial % len(self._slots)]
        self._serial += 1
        self._drain(slot)
        if slot["key"] is None or slot["key"][0] != device or slot["key"][2:] != (h, w) or slot["key"][1] < n:
            stride = _align16(ops.point_cloud_stride(h, w, True))
            rows = len(self.clouds) * n
            slot.update(key=(device, n, h, w), stride=stride,
                        device=torch.empty((rows, stride), dtype=torch.uint8, device=device),
                        counts=torch.empty(rows, dtype=torch.int64, device=device),
                        workspace=torch.empty(ops.point_cloud_workspace_bytes(n, h, w), dtype=torch.uint8, device=device),
                        host=torch.empty((rows, stride), dtype=torch.uint8).pin_memory(),
                        host_counts=torch.empty(rows, dtype=torch.int64).pin_memory())
            for name in ("device", "counts"):
                slot[name].record_stream(self._copy_stream)      # the allocator learns that the side stream reads them
        return slot

    def submit(self, filenames: Sequence[str], image, output_depth, sparse_depth, intrinsics) -> None:
        """One batch: image N x 3 x H x W as ops.preprocess normalised it, output_depth and sparse_depth N x 1 x H x W, intrinsics
        N x 3 x 3 (device, fp32); filenames: N base names, whose extension is replaced by POINT_CLOUD_EXTENSION.  A depth that is
        not among the writer's clouds may be None."""
        if self._closed:
            raise KbnError("PointCloudWriter: submit() after close()")
        depths = {"output_depth": output_depth, "sparse_depth": sparse_depth}
        for name, t in [("image", image), ("intrinsics", intrinsics)] + [(name, depths[name]) for name in self.clouds]:
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise KbnError(f"PointCloudWriter: {name}: expected a CUDA/HIP tensor (the HIP path has no CPU fallback)")
        n, h, w = int(image.shape[0]), int(image.shape[-2]), int(image.shape[-1])
        if len(filenames) != n:
            raise KbnError(f"PointCloudWriter: {n} frames, {len(filenames)} file names")
        device = image.device
        with torch.cuda.device(device):
            if self._copy_stream is None or self._copy_stream.device != device:
                self._copy_stream = torch.cuda.Stream(device=device)
            slot = self._slot(device, n, h, w)
            capacity = slot["key"][1]
            rows = [slice(c * capacity, c * capacity + n) for c in range(len(self.clouds))]      # of cloud c, in every buffer
            kinv = ops.intrinsics_inverse(intrinsics)
            for name, r in zip(self.clouds, rows):
                ops.point_cloud(depths[name], kinv, image, min_depth=self.min_depth, max_depth=self.max_depth, scale=self.scale,
                                shift=self.shift, out=slot["device"][r], out_points=slot["counts"][r], workspace=slot["workspace"])
            ready = torch.cuda.Event()
            ready.record(torch.cuda.current_stream(device))
            self._copy_stream.wait_event(ready)
            with torch.cuda.stream(self._copy_stream):
                for r in rows:
                    slot["host"][r].copy_(slot["device"][r], non_blocking=True)
                    slot["host_counts"][r].copy_(slot["counts"][r], non_blocking=True)
                done = torch.cuda.Event()
                done.record(self._copy_stream)
        files, counts = slot["host"].numpy(), slot["host_counts"].numpy()
        jobs = []
        for i, filename in enumerate(filenames):
            for name, r in zip(self.clouds, rows):
                jobs.append((done, files[r.start + i], counts, r.start + i, h * w, os.path.join(self.dirpaths[name], point_cloud_filename(filename))))
        slot["files"] = [self.pool.submit(self._write, *job) for job in jobs]

    def _write(self, done, file_slot: np.ndarray, counts: np.ndarray, index: int, pixels: int, path: str) -> None:
        done.synchronize()      # the slot's copies have landed: the records and their number
        points = int(counts[index])
        if not 0 <= points <= pixels:
            raise KbnError(f"PointCloudWriter: the device reports {points} points for {path}, the frame has {pixels} pixels")
        self._place(b"".join((ply_header(points, True), memoryview(file_slot[:points * self.RECORD]))), path)


# ------------------------------------------------------------------- batched device loader
class InferenceFrameLoader:
    """Iterates `(image N x 3 x H x W in 0..255, sparse_depth N x 1 x H x W, intrinsics N x 3 x 3)` device
    batches over the files `datasets.KBNetInferenceDataset` would read (same constructor arguments,
    reference src/datasets.py:229-257), in order, the last batch possibly short.  All frames must have
    one size.  Batch i+1 is decoded and copied while the caller works on batch i: `prefetch` batches are in flight, each in one
    of `prefetch + 1` staging sets (`_Staging`) that PNG and packed batches share; files are told apart by their first bytes, read
    once a path.  Of a sequence entry `previous<TAB>current<TAB>next` only `current`, a file one frame wide, is read --
    PNG or packed -- whatever use_image_triplet says; a batch is all triplet files or all sequence entries."""

    def __init__(self, image_paths: Sequence[str], sparse_depth_paths: Sequence[str],
                 intrinsics_paths: Sequence[str], use_image_triplet: bool = True, batch_size: int = 8,
                 device: Optional[torch.device] = None, workers: int = 8, prefetch: int = 4):
        self.n_sample = len(image_paths)
        for paths in (sparse_depth_paths, intrinsics_paths):
            assert len(paths) == self.n_sample
        if device is None or torch.device(device).type != "cuda":
            raise KbnError("InferenceFrameLoader: a CUDA/HIP device is required (no CPU fallback)")
        self.image_paths, self.sparse_depth_paths = list(image_paths), list(sparse_depth_paths)
        self.intrinsics_paths = list(intrinsics_paths)
        self.use_image_triplet = use_image_triplet
        self.batch_size = int(batch_size)
        self.device = torch.device(device)
        self.workers = max(1, int(workers))                      # decode threads per batch (inside the library)
        self.pool = ThreadPoolExecutor(max_workers=min(16, self.workers))   # file reads
        self.copy_stream = torch.cuda.Stream(device=self.device)
        # `prefetch` batches are decoded concurrently (one PNG is one serial inflate stream, so the decode
        # parallelism is batch_size x prefetch), each in its own set of pinned staging tensors
        self.prefetch = max(1, int(prefetch))
        self._driver = ThreadPoolExecutor(max_workers=self.prefetch)
        self._staging = _Staging(self.prefetch + 1, self.batch_size, self.device, self.copy_stream)
        self._file_header = _FileHeaders().__getitem__

    def __len__(self):
        return (self.n_sample + self.batch_size - 1) // self.batch_size

    # -- one batch: lay out, fill a pinned staging set (decode on the pool, or read packed files), async H2D + unpack on the copy stream --
    def _submit(self, b: int):
        lo, hi = b * self.batch_size, min((b + 1) * self.batch_size, self.n_sample)
        idx = list(range(lo, hi))
        entries = _batch_entries([self.image_paths[i] for i in idx], "InferenceFrameLoader")
        # a sequence entry: `current` is the frame, a file one frame wide; nothing else of the sample is read
        triplet = self.use_image_triplet and entries is None
        paths = ([self.image_paths[i] for i in idx] if entries is None else [e[1] for e in entries]) + [self.sparse_depth_paths[i] for i in idx]
        heads = [self._file_header(path) for path in paths]
        if _one_kind(paths, [packed for _, packed in heads], "InferenceFrameLoader"):
            return self._submit_packed(b, idx, paths, [info for info, _ in heads], entries is not None)
        files = list(self.pool.map(_read, paths))
        nb = len(idx)
        wraw, hraw, c, bits = png_info(files[0])
        wd, hd, cd, dbits = png_info(files[nb])
        if bits != 8 or cd != 1:
            raise KbnError("InferenceFrameLoader: expected 8-bit images and single-channel depth PNGs")
        width = wraw // 3 if triplet else wraw
        if (hd, wd) != (hraw, width):
            raise KbnError(f"depth map is {hd} x {wd}, image is {hraw} x {width}")
        for j in range(nb):
            if png_info(files[j]) != (wraw, hraw, c, 8) or png_info(files[nb + j]) != (wd, hd, 1, dbits):
                raise KbnError("InferenceFrameLoader: all frames of a run must have one size and format")
        # frames of one size: dense in the flat buffers, which the device then views as nb x hraw x wraw x c and nb x hd x wd
        sizes = [hraw * wraw * c] * nb + [hd * wd * (dbits // 8)] * nb
        at = [j * sizes[0] for j in range(nb)] + [j * sizes[nb] for j in range(nb)]
        st = self._staging.acquire(b % (self.prefetch + 1), nb * sizes[0], nb * sizes[nb], nb)
        _load_intrinsics(st, [self.intrinsics_paths[i] for i in idx])
        # one library call decodes the whole batch on its own threads (images first: they are the long poles)
        decode_png_batch(files, [view[a:a + size] for view, a, size in _places(st, at, sizes)], threads=self.workers)
        return self._staging.submit(st, nb * sizes[0], nb * sizes[nb], nb, lambda img_d, dep_d, k_d: tuple(ops.unpack_frames(
            img_d.view(nb, hraw, wraw, c), dep_d.view(torch.int16 if dbits == 16 else torch.uint8).view(nb, hd, wd),
            width=width, x_offset=width if triplet else 0)) + (k_d,))

    def _submit_packed(self, b: int, idx, paths, heads, single: bool = False):
        """_submit for a batch of packed frames: the files go as they are into pinned staging, each at a 16-byte-aligned
        offset, pass kbn_frame_check there, cross PCIe packed, and ONE ops.unpack_packed_frames launch decodes the middle thirds.
        `single`: the image files are the `current` frames of sequence entries, one frame wide; ops.unpack_packed_sequence_frames
        decodes them, all three places of a sample's record being that one file."""
        if not self.use_image_triplet and not single:
            raise KbnError("InferenceFrameLoader: packed images are decoded as triplets; use PNG files with use_image_triplet=False")
        nb = len(idx)
        wraw, hraw, c, bits = heads[0]
        wd, hd, cd, dbits = heads[nb]
        if bits != 8 or cd != 1:
            raise KbnError("InferenceFrameLoader: expected 8-bit images and single-channel depth maps")
        if wraw % 3 and not single:
            raise ValueError("array split does not result in an equal division")     # np.split in the reference's load_image_triplet
        width = wraw if single else wraw // 3
        if (hd, wd) != (hraw, width):
            raise KbnError(f"depth map is {hd} x {wd}, image is {hraw} x {width}")
        if any(h != heads[0] for h in heads[:nb]) or any(h != heads[nb] for h in heads[nb:]):
            raise KbnError("InferenceFrameLoader: all frames of a run must have one size and format")
        sizes = [os.path.getsize(path) for path in paths]
        at, total = _layout(sizes)
        st = self._staging.acquire(b % (self.prefetch + 1), total[0], total[1], nb)
        _load_intrinsics(st, [self.intrinsics_paths[i] for i in idx])
        _read_packed_into(self.pool, _packed_jobs(st, paths, at, sizes, heads))
        if single:
            frames = [(at[j], sizes[j]) * 3 + (at[nb + j], sizes[nb + j], hraw, width, 0, 0) for j in range(nb)]
            return self._staging.submit(st, total[0], total[1], nb, lambda img_d, dep_d, k_d: ops.unpack_packed_sequence_frames(
                img_d, dep_d, frames, (hraw, width), channels=c, depth_bits=dbits, middle_only=True) + (k_d,))
        frames = [(at[j], sizes[j], at[nb + j], sizes[nb + j], hraw, width, 0, 0) for j in range(nb)]
        return self._staging.submit(st, total[0], total[1], nb, lambda img_d, dep_d, k_d: ops.unpack_packed_frames(
            img_d, dep_d, frames, (hraw, width), channels=c, depth_bits=dbits, middle_only=True) + (k_d,))

    def __iter__(self):
        nb = len(self)
        pending = [self._driver.submit(self._submit, b) for b in range(min(self.prefetch, nb))]
        for b in range(nb):
            batch, done = pending.pop(0).result()
            if b + self.prefetch < nb:
                pending.append(self._driver.submit(self._submit, b + self.prefetch))
            yield _hand_over(self.device, done, batch)


def _hand_over(device, done, tensors):
    """A batch produced on a loader's copy stream, for the consumer's current stream: that stream waits for the batch's event, and
    the caching allocator learns that it uses the tensors (they were allocated on the copy stream)."""
    cur = torch.cuda.current_stream(device)
    cur.wait_event(done)
    for t in tensors:
        t.record_stream(cur)
    return tensors


# --------------------------------------------------------------------------- the training set
def draw_crop(o_height: int, o_width: int, shape, crop_type=("none",)) -> Tuple[int, int]:
    """(y_start, x_start) of the reference's random_crop (src/datasets.py:92-141) for an o_height x o_width frame: the same
    np.random calls in the same order, so the same np.random.seed gives the reference's crops.  The centre by default;
    'horizontal': randint over the anchors 0, 0.5, 1 when 'anchored', else over [0, d_width); 'bottom' takes the lowest crop and
    draws nothing; otherwise 'vertical' moves 30 % of the crops, over the anchors 0.5, 1 or over [0, d_height).  As in the
    reference an unanchored crop at the raw size raises NumPy's ValueError (randint(0, 0)).  Unlike the reference, which returns a
    short slice, a crop larger than the frame raises KbnError."""
    n_height, n_width = (int(v) for v in shape)
    d_height, d_width = int(o_height) - n_height, int(o_width) - n_width
    if d_height < 0 or d_width < 0:
        raise KbnError(f"draw_crop: a {n_height} x {n_width} crop does not fit a {o_height} x {o_width} frame")
    y_start, x_start = d_height // 2, d_width // 2
    if "horizontal" in crop_type:
        if "anchored" in crop_type:
            widths = [anchor * d_width for anchor in (0.0, 0.50, 1.0)]
            x_start = int(widths[np.random.randint(low=0, high=len(widths))])
        else:
            x_start = np.random.randint(low=0, high=d_width)
    if "bottom" in crop_type:
        y_start = d_height
    elif "vertical" in crop_type and np.random.rand() <= 0.30:
        if "anchored" in crop_type:
            heights = [anchor * d_height for anchor in (0.50, 1.0)]
            y_start = int(heights[np.random.randint(low=0, high=len(heights))])
        else:
            y_start = np.random.randint(low=0, high=d_height)
    return int(y_start), int(x_start)


def draw_crops(sizes, shape, crop_type=("none",), keep=None) -> List[Tuple[int, int]]:
    """draw_crop for every (height, width) of `sizes`, in order: the crops of one batch.  `keep` (first, last): all of them are
    drawn -- np.random advances as for the whole batch -- and those of sizes[first:last] are returned: what a rank of a
    data-parallel run keeps of its global batch's draws (TrainingFrameLoader(crops="global"))."""
    starts = [draw_crop(hh, ww, shape, crop_type) for hh, ww in sizes]
    return starts if keep is None else starts[int(keep[0]):int(keep[1])]


def _crop_intrinsics(intrinsics: np.ndarray, y_start: int, x_start: int) -> np.ndarray:
    """The reference's expression (src/datasets.py:152-154), evaluated as NumPy evaluates it there (the list becomes a float64
    array; adding 0.0 to the other seven entries turns a -0.0 into 0.0); the caller casts to float32."""
    return intrinsics + [[0.0, 0.0, -x_start],
                         [0.0, 0.0, -y_start],
                         [0.0, 0.0, 0.0]]


def random_crop(inputs, shape, intrinsics=None, crop_type=["none"]):
    """reference src/datasets.py:74-158: every C x H x W array of `inputs` cropped to `shape` at draw_crop's position (the first
    array gives the frame's size) and, if given, the 3 x 3 intrinsics moved with it."""
    _, o_height, o_width = inputs[0].shape
    y_start, x_start = draw_crop(o_height, o_width, shape, crop_type)
    y_end, x_end = y_start + shape[0], x_start + shape[1]
    outputs = [T[:, y_start:y_end, x_start:x_end] for T in inputs]
    if intrinsics is not None:
        return outputs, _crop_intrinsics(intrinsics, y_start, x_start)
    return outputs


def _align16(v: int) -> int:
    return (v + 15) & ~15


def shard_batches(order: Sequence[int], batch_size: int, rank: int, world: int) -> List[list]:
    """One rank's part of an epoch: each global batch order[lo:lo + batch_size] split with dist.shard_bounds, so the ranks' shards
    of a batch concatenate to it in rank order.  One entry a global batch; where the last batch holds fewer samples than there are
    ranks, the entries of the last ranks are empty."""
    out = []
    for lo in range(0, len(order), batch_size):
        batch = list(order[lo:lo + batch_size])
        first, last = shard_bounds(len(batch), rank, world)
        out.append(batch[first:last])
    return out


class TrainingFrameLoader:
    """Iterates `(image0, image1, image2, sparse_depth0, intrinsics)` device batches -- images N x 3 x h x w in 0..255, depth
    N x 1 x h x w, intrinsics N x 3 x 3 -- over the files `datasets.KBNetTrainingDataset` reads (the same first five constructor
    arguments, reference src/datasets.py:181-197): what the reference's
    `DataLoader(KBNetTrainingDataset(...), batch_size, shuffle, drop_last=False)` yields after `.to(device)` (src/kbnet.py:134-144).

    Each `iter()` is one epoch.  Its order is drawn when it starts: file order, or with `shuffle` what
    `torch.utils.data.RandomSampler(range(n), generator=generator)` yields.  The crops are drawn with `draw_crop` from np.random
    on the ITERATING thread, batch by batch in epoch order and sample by sample inside a batch, just before the batch goes to the
    pool: they do not depend on the pool's timing, and under np.random.seed(s) with shuffle=False the batches are the reference
    dataset's samples in index order.  Raw sizes come from the files' headers (the first 33 bytes of a PNG, the first 32 of a packed
    frame, read once).

    The pipeline is InferenceFrameLoader's: files are read by a thread pool, decoded by the library (`decode_png_batch`) straight
    into PINNED staging -- frames may differ in size, so each sits at its own 16-byte-aligned offset of a flat buffer -- the used
    prefix of each buffer crosses PCIe as raw bytes in one asynchronous copy on a side stream, and `ops.unpack_train_frames`
    splits, crops and converts there.  A batch of packed frames (module docstring; all of a batch's files or none) skips the decode: the
    files themselves go to pinned staging, pass `kbn_frame_check` there, and `ops.unpack_packed_frames` decodes them on the device.
    An image entry may be a sequence entry `previous<TAB>current<TAB>next` (module docstring) in place of a triplet file: its
    three frames must have one size and format and its depth map a frame's size, it is planned and cropped as the triplet file of those
    frames would be (one seed, the same batches), every distinct file of the batch is read once, and `ops.unpack_sequence_frames` /
    `ops.unpack_packed_sequence_frames` build the tensors.  A batch is all triplet files or all sequence entries.
    `prefetch` batches are in flight, each in one of the `prefetch + 1` staging sets the two kinds share (`_Staging`: a set is grown
    when a batch needs more, after the copies that last used it).  Without a crop (`shape` None or not positive) the frames of
    a batch must have one size.  An error found while a batch is prepared is raised when that batch is due.  One epoch at a time:
    `iter()` first waits for what an epoch that was left early still has in flight.

    Data-parallel training (`rank`, `world`; kb.dist.GradientAverager): every rank iterates the same `len()` GLOBAL batches and is
    handed its shard of each (`shard_batches`), `global_batch_size(b)` frames in all.  The epoch's order is drawn as above on every
    rank and, when a process group exists, replaced by rank 0's (one broadcast_object_list an epoch), so the ranks need no equally
    seeded generators.  A rank whose shard of a short last batch is empty is handed the five tensors with zero frames; nothing is
    launched for them.

    `crops`: whose crops a rank draws.  "own" (the default): those of its own samples only -- the ranks' batches are then not the
    one-process batch under any seeds.  "global": the iterating thread calls `draw_crop` for EVERY sample of the global batch, in
    batch order, and keeps its own (the other samples cost their two 33-byte PNG headers, read once); a rank with an empty shard
    draws too.  Ranks that start from one np.random state then draw the same crops, and their batches concatenate, in rank order,
    to the batch one process builds under that state: kb.training.train_ranks(rank, world) uses it.  np.random is shared with whatever
    else the thread draws between two batches (Transforms.draw), and `prefetch` decides how many batches' crops are drawn ahead
    of those draws, so the ranks AND the one-process run they are compared with must use the same `prefetch`.

    For the same reason an epoch that is left between two batches and continued elsewhere (kb.training.train_resumable) needs more
    than np.random's state: `state_dict()` holds the epoch's order, the next batch's index and the plans -- crops included -- of the
    batches already in flight, and after `load_state_dict(state)` the next `iter()` yields the rest of that epoch.  With `world` ranks
    and crops="global" (kb.training.train_ranks_resumable) the state is the global one -- the plans of whole global batches, equal
    on every rank -- and every rank continues from rank 0's, taking its shard of each stored plan."""

    def __init__(self, image_paths: Sequence[str], sparse_depth_paths: Sequence[str], intrinsics_paths: Sequence[str],
                 shape=None, random_crop_type=["none"], batch_size: int = 8, shuffle: bool = True,
                 device: Optional[torch.device] = None, workers: int = 8, prefetch: int = 4, generator=None, rank: int = 0,
                 world: int = 1, crops: str = "own"):
        what = "TrainingFrameLoader"
        if crops not in ("own", "global"):
            raise KbnError(f"{what}: crops {crops!r}: 'own' or 'global'")
        self.crops = crops
        if int(world) < 1 or not 0 <= int(rank) < int(world):
            raise KbnError(f"{what}: rank {rank} of world {world}")
        self.rank, self.world = int(rank), int(world)
        self.n_sample = len(image_paths)
        if len(sparse_depth_paths) != self.n_sample or len(intrinsics_paths) != self.n_sample:
            raise KbnError(f"{what}: {self.n_sample} image, {len(sparse_depth_paths)} sparse depth and {len(intrinsics_paths)} intrinsics paths")
        if device is None or torch.device(device).type != "cuda":
            raise KbnError(f"{what}: a CUDA/HIP device is required (no CPU fallback)")
        if int(batch_size) < 1:
            raise KbnError(f"{what}: batch_size {batch_size}")
        self.image_paths, self.sparse_depth_paths = list(image_paths), list(sparse_depth_paths)
        self.intrinsics_paths = list(intrinsics_paths)
        self.shape = shape
        self.random_crop_type = random_crop_type
        self.batch_size = int(batch_size)
        self.shuffle = bool(shuffle)
        self.generator = generator
        self.device = torch.device(device)
        self.workers = max(1, min(16, int(workers)))             # file-read threads, and decode threads per batch (inside the library)
        self.pool = ThreadPoolExecutor(max_workers=self.workers)
        self.copy_stream = torch.cuda.Stream(device=self.device)
        self.prefetch = max(1, int(prefetch))                    # batches decoded concurrently, each in its own staging set
        self._driver = ThreadPoolExecutor(max_workers=min(16, self.prefetch))
        self._staging = _Staging(self.prefetch + 1, self.batch_size, self.device, self.copy_stream)
        self._file_header = _FileHeaders().__getitem__
        self._pending: list = []
        self._serial = 0                                         # batches submitted so far: picks the staging set
        self._order: Optional[list] = None                       # the running epoch's order, the batch iter() hands out next and the
        self._next = 0                                           # plans of the batches enqueued beyond it: what state_dict() holds
        self._plans: list = []
        self._resume: Optional[dict] = None                      # load_state_dict()'s state, for the next iter()

    @property
    def do_random_crop(self) -> bool:
        return self.shape is not None and all([x > 0 for x in self.shape])      # reference src/datasets.py:193-194

    def __len__(self):
        return (self.n_sample + self.batch_size - 1) // self.batch_size

    def global_batch_size(self, b: int) -> int:
        """The frames of global batch b over all ranks (the n_global of GradientAverager.average)."""
        if not 0 <= b < len(self):
            raise KbnError(f"TrainingFrameLoader: batch {b} of {len(self)}")
        return min(self.batch_size, self.n_sample - b * self.batch_size)

    # -- on the iterating thread: the batch's raw sizes, its checks and its crops --
    def _header(self, i: int, fields=None):
        """(header of sample i's image, header of its depth map); `fields`, a sequence entry's three paths: the one header its frames
        must share."""
        if fields is None:
            return tuple(self._file_header(path)[0] for path in (self.image_paths[i], self.sparse_depth_paths[i]))
        heads = [self._file_header(path)[0] for path in fields]
        for path, head in zip(fields, heads):
            if head != heads[0]:
                raise KbnError(f"TrainingFrameLoader: the three frames of a sample must have one size and format: {path} is {head[1]} x {head[0]} with "
                               f"{head[2]} channels of {head[3]} bits, {fields[0]} is {heads[0][1]} x {heads[0][0]} with {heads[0][2]} of {heads[0][3]}")
        return heads[0], self._file_header(self.sparse_depth_paths[i])[0]

    def _plan(self, idx: Sequence[int]):
        """[(sample, raw height, raw width of a third, y_start, x_start)], (h, w), channels, depth bits, whether it is cropped.
        With crops="global" `idx` is a global batch, checked and drawn for as a whole; _enqueue_planned takes the rank's slice.
        A sequence entry is planned as the triplet file of its three frames would be: its raw width is 3 W."""
        entries = _batch_entries([self.image_paths[i] for i in idx], "TrainingFrameLoader")
        heads = [self._header(i) for i in idx] if entries is None else [self._header(i, fields) for i, fields in zip(idx, entries)]
        if entries is not None:
            heads = [((3 * w, h, ci, bi), depth) for (w, h, ci, bi), depth in heads]
        (_, _, c, bits), (_, _, cd, dbits) = heads[0]
        if bits != 8 or cd != 1:
            raise KbnError(f"TrainingFrameLoader: expected 8-bit images and single-channel depth PNGs ({self.image_paths[idx[0]]}, {self.sparse_depth_paths[idx[0]]})")
        sizes = []
        for i, ((wraw, hraw, ci, bi), (wd, hd, cdi, dbi)) in zip(idx, heads):
            if (ci, bi, cdi, dbi) != (c, 8, 1, dbits):
                raise KbnError(f"TrainingFrameLoader: the frames of a batch must have one format: {self.image_paths[i]} has {ci} channels of {bi} bits "
                               f"and {cdi}-channel depth of {dbi} bits, {self.image_paths[idx[0]]} has {c} of 8 and 1 of {dbits}")
            if wraw % 3:
                raise ValueError("array split does not result in an equal division")     # np.split in the reference's load_image_triplet
            if (hd, wd) != (hraw, wraw // 3):
                raise KbnError(f"TrainingFrameLoader: depth map {self.sparse_depth_paths[i]} is {hd} x {wd}, image {self.image_paths[i]} is {hraw} x {wraw // 3}")
            sizes.append((hraw, wraw // 3))
        if self.do_random_crop:
            shape = (int(self.shape[0]), int(self.shape[1]))
            starts = draw_crops(sizes, shape, self.random_crop_type)
        else:
            shape = sizes[0]
            for i, size in zip(idx, sizes):
                if size != shape:
                    raise KbnError(f"TrainingFrameLoader: without a crop shape the frames of a batch must have one size: {self.image_paths[i]} is "
                                   f"{size[0]} x {size[1]}, {self.image_paths[idx[0]]} is {shape[0]} x {shape[1]}")
            starts = [(0, 0)] * len(idx)
        frames = [(i, hh, ww, y, x) for i, (hh, ww), (y, x) in zip(idx, sizes, starts)]
        return frames, shape, c, dbits, self.do_random_crop

    # -- on a driver thread: lay out, fill a pinned staging set (decode, or read packed files), async H2D + unpack on the copy stream --
    def _submit(self, slot: int, plan, shape, c: int, dbits: int, cropped: bool):
        nb = len(plan)
        idx = [p[0] for p in plan]
        starts = [(y, x) for _, _, _, y, x in plan] if cropped else None
        entries = _batch_entries([self.image_paths[i] for i in idx], "TrainingFrameLoader")
        if entries is not None:
            return self._submit_sequence(slot, plan, shape, c, dbits, starts, entries)
        paths = [self.image_paths[i] for i in idx] + [self.sparse_depth_paths[i] for i in idx]
        if _one_kind(paths, [self._file_header(path)[1] for path in paths], "TrainingFrameLoader"):      # read already unless the plan comes from load_state_dict
            return self._submit_packed(slot, plan, shape, c, dbits, starts, paths)
        files = list(self.pool.map(_read, paths))
        for j, (i, hraw, w, y, x) in enumerate(plan):
            if png_info(files[j]) != (3 * w, hraw, c, 8) or png_info(files[nb + j]) != (w, hraw, 1, dbits):
                raise KbnError(f"TrainingFrameLoader: {self.image_paths[i]} or {self.sparse_depth_paths[i]} changed since its header was read")
        sizes = [hraw * 3 * w * c for _, hraw, w, _, _ in plan] + [hraw * w * (dbits // 8) for _, hraw, w, _, _ in plan]
        at, total = _layout(sizes)
        st = self._staging.acquire(slot, total[0], total[1], nb)
        _load_intrinsics(st, [self.intrinsics_paths[i] for i in idx], starts)
        # one library call decodes the whole batch on its own threads (images first: they are the long poles)
        decode_png_batch(files, [view[a:a + size] for view, a, size in _places(st, at, sizes)], threads=self.workers)
        frames = [(at[j], at[nb + j], hraw, w, y, x) for j, (_, hraw, w, y, x) in enumerate(plan)]
        return self._staging.submit(st, total[0], total[1], nb, lambda img_d, dep_d, k_d: ops.unpack_train_frames(
            img_d, dep_d, frames, shape, channels=c, depth_bits=dbits) + (k_d,))

    def _submit_packed(self, slot: int, plan, shape, c: int, dbits: int, starts, paths):
        """_submit for a batch of packed frames: nothing is decoded on the host.  Every file is read straight into its
        16-byte-aligned place of the pinned staging buffer and passes kbn_frame_check there; the packed bytes cross PCIe in one
        asynchronous copy per buffer, and ONE ops.unpack_packed_frames launch decodes, splits, crops and converts."""
        nb = len(plan)
        sizes = [os.path.getsize(path) for path in paths]
        at, total = _layout(sizes)
        st = self._staging.acquire(slot, total[0], total[1], nb)
        _load_intrinsics(st, [self.intrinsics_paths[p[0]] for p in plan], starts)
        want = [(3 * w, hraw, c, 8) for _, hraw, w, _, _ in plan] + [(w, hraw, 1, dbits) for _, hraw, w, _, _ in plan]
        _read_packed_into(self.pool, _packed_jobs(st, paths, at, sizes, want))
        frames = [(at[j], sizes[j], at[nb + j], sizes[nb + j], hraw, w, y, x) for j, (_, hraw, w, y, x) in enumerate(plan)]
        return self._staging.submit(st, total[0], total[1], nb, lambda img_d, dep_d, k_d: ops.unpack_packed_frames(
            img_d, dep_d, frames, shape, channels=c, depth_bits=dbits) + (k_d,))

    def _submit_sequence(self, slot: int, plan, shape, c: int, dbits: int, starts, entries):
        """_submit for a batch of sequence entries, PNG or packed: every DISTINCT image file of the batch -- `current`
        repeats in a `p<TAB>p<TAB>p` entry, neighbouring samples share frames -- is read, and decoded or checked, once, into a place
        of its own in pinned staging; a sample's record points at its three.  ONE ops.unpack_sequence_frames or
        ops.unpack_packed_sequence_frames launch crops and converts."""
        nb = len(plan)
        place, want = {}, []      # image file -> its index among the batch's image files; the header it was planned with
        for (_, hraw, w, _, _), fields in zip(plan, entries):
            for path in fields:
                if path not in place:
                    place[path] = len(want)
                    want.append((w, hraw, c, 8))
        ni = len(want)
        paths = list(place) + [self.sparse_depth_paths[p[0]] for p in plan]
        want += [(w, hraw, 1, dbits) for _, hraw, w, _, _ in plan]
        packed = _one_kind(paths, [self._file_header(path)[1] for path in paths], "TrainingFrameLoader")
        if packed:
            sizes = [os.path.getsize(path) for path in paths]
        else:
            files = list(self.pool.map(_read, paths))
            for path, data, header in zip(paths, files, want):
                if png_info(data) != header:
                    raise KbnError(f"TrainingFrameLoader: {path} changed since its header was read")
            sizes = [hh * ww * cc * (bb // 8) for ww, hh, cc, bb in want]
        at, total = _layout(sizes, ni)
        st = self._staging.acquire(slot, total[0], total[1], nb)
        _load_intrinsics(st, [self.intrinsics_paths[p[0]] for p in plan], starts)
        if packed:
            _read_packed_into(self.pool, _packed_jobs(st, paths, at, sizes, want, ni))
            frames = [sum(((at[place[path]], sizes[place[path]]) for path in fields), ()) + (at[ni + j], sizes[ni + j], hraw, w, y, x)
                      for j, ((_, hraw, w, y, x), fields) in enumerate(zip(plan, entries))]
            unpack = ops.unpack_packed_sequence_frames
        else:
            decode_png_batch(files, [view[a:a + size] for view, a, size in _places(st, at, sizes, ni)], threads=self.workers)
            frames = [tuple(at[place[path]] for path in fields) + (at[ni + j], hraw, w, y, x)
                      for j, ((_, hraw, w, y, x), fields) in enumerate(zip(plan, entries))]
            unpack = ops.unpack_sequence_frames
        return self._staging.submit(st, total[0], total[1], nb, lambda img_d, dep_d, k_d: unpack(
            img_d, dep_d, frames, shape, channels=c, depth_bits=dbits) + (k_d,))

    def _enqueue(self, idx: Sequence[int], batch=None, first: int = 0, plan=None):
        """The batch's draws, now and here; the rest on a driver thread.  What goes wrong either way is kept for the batch's turn.
        `batch`, `first`: with crops="global" the global batch and where `idx` starts in it.  `plan`: what _plan returned for this
        batch -- the GLOBAL batch with crops="global" -- in an earlier session (load_state_dict): nothing is drawn."""
        future = self._enqueue_planned(idx, batch, first, plan)
        self._plans.append(getattr(future, "plan", None))
        return future

    def _enqueue_planned(self, idx: Sequence[int], batch, first: int, plan):
        """The future's `plan` is what state_dict() stores: the plan of the whole global batch with crops="global" -- the same on
        every rank, an empty shard's included -- of which this rank submits its slice; the plan of `idx` otherwise."""
        error, whole = None, None
        if batch is not None:      # the whole batch's draws, on every rank, before anything else: an empty shard draws too
            try:
                whole = self._plan(batch) if plan is None else plan
                plan = (whole[0][first:first + len(idx)],) + tuple(whole[1:])
            except Exception as e:      # noqa: BLE001  (raised again by .result() when the batch is due)
                error = e
        if not idx and error is None:      # this rank's shard of a short last batch: zero frames, no staging set, nothing launched
            h, w = (int(self.shape[0]), int(self.shape[1])) if self.do_random_crop else (0, 0)
            empty: Future = Future()
            empty.set_result((tuple(torch.empty(s, dtype=torch.float32, device=self.device)
                                    for s in ((0, 3, h, w), (0, 3, h, w), (0, 3, h, w), (0, 1, h, w), (0, 3, 3))), None))
            empty.plan = whole
            return empty
        slot = self._serial % (self.prefetch + 1)
        self._serial += 1
        if plan is None and error is None:
            try:
                plan = self._plan(idx)
            except Exception as e:      # noqa: BLE001  (raised again by .result() when the batch is due)
                error = e
        if error is not None:
            failed: Future = Future()
            failed.set_exception(error)
            return failed
        future = self._driver.submit(self._submit, slot, *plan)
        future.plan = plan if whole is None else whole
        return future

    def state_dict(self) -> dict:
        """Where the running epoch stands, between two batches: the epoch's order, the index of the batch iter() hands out next and
        the finished plans (_plan's frames with their crop origins, shape and format) of the batches already enqueued beyond it --
        their crops were drawn from np.random ahead of whatever the iterating thread drew since, so np.random's state alone does not
        bring them back.  Empty before the first epoch and after an epoch's last batch.  Plain Python numbers only.

        A sharded loader (world > 1) with crops="global" holds the GLOBAL state: the plans are those of the whole global batches,
        so ranks that drew alike return equal dicts (a rank whose shard of a short last batch is empty too), and any rank's state
        continues every rank.  With crops="own" a sharded loader raises KbnError: its ranks' draws are not one state."""
        if self.world > 1 and self.crops != "global":
            raise KbnError("TrainingFrameLoader: state_dict of a sharded loader (world > 1) needs crops='global': with crops='own' every "
                           "rank draws for its own samples, and no one state continues them all")
        if self._order is None or self._next >= len(self):
            return {}
        if any(plan is None for plan in self._plans):
            raise KbnError("TrainingFrameLoader: state_dict: a batch in flight could not be planned (its error is raised when it is due)")
        plans = [([tuple(int(v) for v in frame) for frame in frames], [int(shape[0]), int(shape[1])], int(c), int(dbits), bool(cropped))
                 for frames, shape, c, dbits, cropped in self._plans]
        return {"order": [int(i) for i in self._order], "next": int(self._next), "plans": plans, "n_sample": self.n_sample,
                "batch_size": self.batch_size}

    def load_state_dict(self, state: dict) -> None:
        """The next iter() continues the epoch `state` (a state_dict()) was taken in: the stored order (nothing is drawn from torch's
        generator), from batch `next` on; the stored plans are submitted as they are and crops are drawn only for the batches beyond
        them, in the order the uninterrupted iteration draws them.  An empty state: the next iter() is an ordinary one.  KbnError for
        a state of another path count, batch size or prefetch depth.  A sharded loader with crops="global" takes the global state
        (state_dict) and submits its dist.shard_bounds share of each stored plan; with crops="own" it raises KbnError.  The state does
        not say at which `world` it was taken: whoever stores it keeps that beside it (kb.training's argument record does)."""
        what = "TrainingFrameLoader: load_state_dict"
        if self.world > 1 and self.crops != "global":
            raise KbnError(f"{what} of a sharded loader (world > 1) needs crops='global'")
        if not state:
            self._resume = None
            return
        order, nxt, plans = [int(i) for i in state["order"]], int(state["next"]), list(state["plans"])
        if int(state["n_sample"]) != self.n_sample or sorted(order) != list(range(self.n_sample)):
            raise KbnError(f"{what}: the state orders {state['n_sample']} samples, this loader has {self.n_sample} paths")
        if int(state["batch_size"]) != self.batch_size:
            raise KbnError(f"{what}: the state's batch size is {state['batch_size']}, this loader's {self.batch_size}")
        if not 0 < nxt < len(self):
            raise KbnError(f"{what}: next batch {nxt} of {len(self)}")
        if len(plans) != min(self.prefetch, len(self) - nxt):
            raise KbnError(f"{what}: the state holds the plans of {len(plans)} batches, a prefetch of {self.prefetch} has "
                           f"{min(self.prefetch, len(self) - nxt)} in flight before batch {nxt} of {len(self)}")
        for b, (frames, shape, c, dbits, cropped) in enumerate(plans, nxt):
            if [int(f[0]) for f in frames] != order[b * self.batch_size:(b + 1) * self.batch_size]:
                raise KbnError(f"{what}: the plan of batch {b} does not hold the samples of the state's order")
        self._resume = {"order": order, "next": nxt,
                        "plans": [([tuple(int(v) for v in f) for f in frames], (int(shape[0]), int(shape[1])), int(c), int(dbits), bool(cropped))
                                  for frames, shape, c, dbits, cropped in plans]}

    def __iter__(self):
        for f in self._pending:      # batches of an epoch that was left early still own staging sets
            f.exception()
        self._plans = []
        if self._resume is not None:      # the rest of an epoch another session began (load_state_dict): its order, its plans
            resume, self._resume = self._resume, None
            self._order, first = resume["order"], resume["next"]
            batches = self._batches(self._order)
            plans = resume["plans"] + [None] * self.prefetch      # a batch without a stored plan is drawn for
            self._pending = pending = [self._enqueue(*batches[first + j], plan=plans[j])
                                       for j in range(min(self.prefetch, len(batches) - first))]
            return self._epoch(batches, pending, first)
        if self.shuffle:
            order = list(torch.utils.data.RandomSampler(range(self.n_sample), generator=self.generator))
        else:
            order = list(range(self.n_sample))
        if self.world > 1 and torch.distributed.is_available() and torch.distributed.is_initialized():
            shared = [[int(i) for i in order]]
            torch.distributed.broadcast_object_list(shared, src=0)
            order = shared[0]
        self._order = order
        batches = self._batches(order)
        self._pending = pending = [self._enqueue(*batches[b]) for b in range(min(self.prefetch, len(batches)))]
        return self._epoch(batches, pending)

    def _batches(self, order):
        """_enqueue's arguments for every batch of an epoch in `order`: this rank's shard, and with crops="global" the global
        batch and the shard's place in it."""
        batches = shard_batches(order, self.batch_size, self.rank, self.world)
        if self.crops == "global":
            return [(shard, list(order[b * self.batch_size:(b + 1) * self.batch_size]),
                     shard_bounds(self.global_batch_size(b), self.rank, self.world)[0]) for b, shard in enumerate(batches)]
        return [(shard,) for shard in batches]

    def _epoch(self, batches, pending, first: int = 0):
        self._next = first
        for b in range(first, len(batches)):
            batch, done = pending.pop(0).result()
            self._plans.pop(0)
            if b + self.prefetch < len(batches):
                pending.append(self._enqueue(*batches[b + self.prefetch]))
            self._next = b + 1
            yield batch if done is None else _hand_over(self.device, done, batch)
