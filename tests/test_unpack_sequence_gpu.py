"""GPU: kbn_unpack_sequence_frames_forward and kbn_unpack_packed_sequence_frames_forward against NumPy slices of the source
arrays -- the reference's semantics (load_image_triplet's thirds are the three frames, random_crop's slices, uint8 -> float32,
depth / 256), never against another kernel.  Packed files are built with encode_frame.

    python -m pytest tests/test_unpack_sequence_gpu.py -m gpu -q

Every comparison is exact.  The outputs of a call are carved out of one sentinel-filled buffer with guard floats between them, so a
write outside an output shows, as does an output that was to stay unwritten.  Shapes are the smallest at which each path can go
wrong: frames of 9 x 17 and 8 x 16 (two 8-row groups with a ragged second, two 16-sample segments with a ragged second, and the
exact fit) in one launch."""
import ctypes as C

import numpy as np
import pytest
import torch

import kbnet_amd as kb

pytestmark = pytest.mark.gpu

SENTINEL = -7.0      # no output value: images are 0 .. 255, depths >= 0
GUARD = 8            # floats between two outputs (a multiple of 4: the outputs keep their alignment)
KINDS = ("raw", "packed")
FORMATS = [(c, bits) for c in (1, 3, 4) for bits in (8, 16)]
MAX = kb._lib.KBN_UNPACK_SEQUENCE_MAX_FRAMES


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _frame(rng, h, w, c):
    return rng.integers(0, 256, size=(h, w) if c == 1 else (h, w, c), dtype=np.uint8)


def _depth(rng, h, w, bits):
    z = rng.integers(0, 1 << bits, size=(h, w)).astype(np.uint16 if bits == 16 else np.uint8)
    z[rng.uniform(size=(h, w)) < 0.5] = 0      # sparse, as the real maps are
    return z


def _sample(rng, h, w, c, bits):
    """(previous, current, next, depth) of one sample: four arrays of their own."""
    return (_frame(rng, h, w, c), _frame(rng, h, w, c), _frame(rng, h, w, c), _depth(rng, h, w, bits))


def _buffers(kind, samples, dev):
    """The two device buffers and where every distinct array lies in them: id(array) -> (offset, bytes).  Raw frames sit at odd
    byte offsets (any alignment is allowed there), depth maps at even ones, packed files at multiples of 16."""
    place, blobs, total = {}, ([], []), [0, 0]
    for sample in samples:
        for k, array in enumerate(sample):
            if id(array) in place:
                continue
            which = int(k == 3)
            data = kb.loader.encode_frame(array) if kind == "packed" else array.tobytes()
            pad = (-total[which]) % 16 if kind == "packed" else (1 if which == 0 else 2)
            blobs[which].append(b"\xa5" * pad + data)
            place[id(array)] = (total[which] + pad, len(data))
            total[which] += pad + len(data)
    tensors = []
    for blob in blobs:
        host = np.frombuffer(b"".join(blob) + b"\xa5" * 64, dtype=np.uint8).copy()      # the tail: room for a record that lies about a size
        tensors.append(torch.from_numpy(host).to(dev))
    return tensors[0], tensors[1], place


def _run(kind, samples, starts, shape, c, bits, dev, shift=0, middle_only=False, lie=None):
    """One call of the entry point of `kind` on `samples` with the crops `starts`; -> {name: N x . x h x w host array}, and asserts
    that every float outside the outputs is still the sentinel.  shift: floats by which every output is moved off its 16-byte
    alignment.  lie(i, k, size) -> the size the record gives file k (0 .. 2 image, 3 depth) of sample i (packed only)."""
    n, (h, w) = len(samples), shape
    images, depths, place = _buffers(kind, samples, dev)
    if kind == "raw":
        table = (kb._lib.SequenceFrame * n)()
    else:
        table = (kb._lib.PackedSequenceFrame * n)()
    for i, (sample, (y, x)) in enumerate(zip(samples, starts)):
        rec = table[i]
        for k in range(3):
            rec.image_offset[k] = place[id(sample[k])][0]
            if kind == "packed":
                size = place[id(sample[k])][1]
                rec.image_bytes[k] = size if lie is None else lie(i, k, size)
        rec.depth_offset = place[id(sample[3])][0]
        if kind == "packed":
            size = place[id(sample[3])][1]
            rec.depth_bytes = size if lie is None else lie(i, 3, size)
        rec.height, rec.width = sample[1].shape[0], sample[1].shape[1]
        rec.y_start, rec.x_start = y, x
    names = ("image0", "depth") if middle_only else ("image0", "image1", "image2", "depth")
    sizes = {name: n * (1 if name == "depth" else 3) * h * w for name in names}
    at, cursor = {}, GUARD + shift
    for name in names:
        at[name] = cursor
        cursor = (cursor + sizes[name] + GUARD + 3) // 4 * 4 + shift
    flat = torch.full((cursor + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    assert flat.data_ptr() % 16 == 0
    ptr = {name: flat.data_ptr() + 4 * at[name] for name in names}
    fn = getattr(kb._lib.load(), "kbn_unpack_sequence_frames_forward" if kind == "raw" else "kbn_unpack_packed_sequence_frames_forward")
    rc = fn(images.data_ptr(), images.numel(), depths.data_ptr(), depths.numel(), table, n, h, w, c, bits, ptr["image0"], ptr.get("image1"),
            ptr.get("image2"), ptr["depth"], torch.cuda.current_stream(dev).cuda_stream)
    assert rc == kb._lib.KBN_OK, rc
    torch.cuda.synchronize(dev)      # a device error would surface here
    host = flat.cpu().numpy()
    outside = np.ones(host.shape, dtype=bool)
    out = {}
    for name in names:
        outside[at[name]:at[name] + sizes[name]] = False
        out[name] = host[at[name]:at[name] + sizes[name]].reshape(n, -1, h, w)
    assert np.all(host[outside] == SENTINEL), "a write outside the outputs"
    return out


def _pixels(frame, y, x, h, w):
    """What the reference makes of a frame's crop: 3 x h x w float32 in 0 .. 255, gray replicated, alpha dropped."""
    assert 0 <= y and y + h <= frame.shape[0] and 0 <= x and x + w <= frame.shape[1], "the test's own crop leaves its frame"
    px = frame[y:y + h, x:x + w]
    if px.ndim == 2:
        px = np.repeat(px[:, :, None], 3, axis=2)
    return np.transpose(px[:, :, :3], (2, 0, 1)).astype(np.float32)


def _expected(samples, starts, shape, middle_only=False):
    h, w = shape
    want = {"image0": np.stack([_pixels(s[1], y, x, h, w) for s, (y, x) in zip(samples, starts)]),
            "depth": np.stack([(s[3][y:y + h, x:x + w].astype(np.float32) / np.float32(256.0))[None] for s, (y, x) in zip(samples, starts)])}
    if not middle_only:
        want["image1"] = np.stack([_pixels(s[0], y, x, h, w) for s, (y, x) in zip(samples, starts)])
        want["image2"] = np.stack([_pixels(s[2], y, x, h, w) for s, (y, x) in zip(samples, starts)])
    return want


def _check(got, want):
    assert set(got) == set(want)
    for name in want:
        assert got[name].shape == want[name].shape and np.array_equal(got[name], want[name]), name


# (crop, origin in the 9 x 17 frame, origin in the 8 x 16 frame)
CROPS = {
    "crosses the group and the segment boundary; the far corner of both frames": ((5, 6), (4, 11), (3, 10)),
    "the 16-byte-store path": ((5, 8), (0, 8), (0, 8)),
    "the near corner, scalar": ((3, 5), (0, 0), (0, 0)),
    "one pixel at the far corner": ((1, 1), (8, 16), (7, 15)),
}


@pytest.mark.parametrize("c, bits", FORMATS)
@pytest.mark.parametrize("kind", KINDS)
def test_two_frame_sizes_in_one_launch(dev, kind, c, bits):
    rng = np.random.default_rng(100 * c + bits)
    samples = [_sample(rng, 9, 17, c, bits), _sample(rng, 8, 16, c, bits)]
    for shape, first, second in CROPS.values():
        _check(_run(kind, samples, [first, second], shape, c, bits, dev), _expected(samples, [first, second], shape))
    # the full frame, each size in a launch of its own (a launch has one crop shape)
    for sample in samples:
        shape = sample[1].shape[:2]
        _check(_run(kind, [sample], [(0, 0)], shape, c, bits, dev), _expected([sample], [(0, 0)], shape))


@pytest.mark.parametrize("kind", KINDS)
def test_outputs_off_their_alignment_take_the_scalar_path(dev, kind):
    rng = np.random.default_rng(7)
    samples = [_sample(rng, 9, 17, 3, 16), _sample(rng, 8, 16, 3, 16)]
    starts, shape = [(0, 8), (0, 8)], (5, 8)      # width % 4 == 0: only the alignment decides
    _check(_run(kind, samples, starts, shape, 3, 16, dev, shift=1), _expected(samples, starts, shape))


@pytest.mark.parametrize("kind", KINDS)
def test_one_more_sample_than_a_launch_carries(dev, kind):
    """MAX + 1 tiny samples: two launches, and the second's one sample lands at batch index MAX."""
    rng = np.random.default_rng(11)
    samples = [_sample(rng, 3, 5, 3, 16) for _ in range(MAX + 1)]
    starts = [(i % 2, i % 3) for i in range(MAX + 1)]
    _check(_run(kind, samples, starts, (2, 3), 3, 16, dev), _expected(samples, starts, (2, 3)))


@pytest.mark.parametrize("c, bits", [(3, 16), (1, 8)])
@pytest.mark.parametrize("kind", KINDS)
def test_coinciding_and_shared_frames(dev, kind, c, bits):
    """p<TAB>p<TAB>p: one frame at all three places of a sample; and neighbouring samples of a sequence that share frames."""
    rng = np.random.default_rng(13)
    frames = [_frame(rng, 9, 17, c) for _ in range(4)]
    depths = [_depth(rng, 9, 17, bits) for _ in range(3)]
    samples = [(frames[0], frames[0], frames[0], depths[0]), (frames[0], frames[1], frames[2], depths[1]),
               (frames[1], frames[2], frames[3], depths[2])]
    starts, shape = [(4, 11), (0, 0), (2, 7)], (5, 6)
    got = _run(kind, samples, starts, shape, c, bits, dev)
    _check(got, _expected(samples, starts, shape))
    assert np.array_equal(got["image0"][0], got["image1"][0]) and np.array_equal(got["image0"][0], got["image2"][0])


@pytest.mark.parametrize("c", [1, 3])
def test_packed_middle_only_decodes_current_alone(dev, c):
    """image1 = image2 = NULL: image0 and the depth are right, and nothing else in the buffer they were carved from is written."""
    rng = np.random.default_rng(17)
    samples = [_sample(rng, 9, 17, c, 16), _sample(rng, 8, 16, c, 16)]
    starts, shape = [(4, 11), (3, 10)], (5, 6)
    _check(_run("packed", samples, starts, shape, c, 16, dev, middle_only=True), _expected(samples, starts, shape, middle_only=True))


@pytest.mark.parametrize("kind", KINDS)
def test_a_crop_wider_than_a_tile(dev, kind):
    """245 columns from column 3 of a 250-column frame: the packed decoder's second tile of 240 columns, at a phase that is not 0."""
    rng = np.random.default_rng(19)
    samples = [_sample(rng, 3, 250, 1, 16)]
    _check(_run(kind, samples, [(1, 3)], (2, 245), 1, 16, dev), _expected(samples, [(1, 3)], (2, 245)))


def test_a_packed_file_whose_size_disagrees_with_its_record(dev):
    """The `next` file of sample 0 is a valid file, but its record claims 16 bytes more (still inside the buffer): the kernel finds
    header and record at odds and leaves every unit of that file unwritten; all other outputs are right and no device error is
    raised.  One call, one bad file."""
    rng = np.random.default_rng(23)
    samples = [_sample(rng, 9, 17, 3, 16), _sample(rng, 8, 16, 3, 16)]
    starts, shape = [(4, 11), (3, 10)], (5, 6)
    got = _run("packed", samples, starts, shape, 3, 16, dev, lie=lambda i, k, size: size + 16 if (i, k) == (0, 2) else size)
    want = _expected(samples, starts, shape)
    assert np.all(got["image2"][0] == SENTINEL), "the units of the file that disagrees stay unwritten"
    want["image2"][0] = SENTINEL
    _check(got, want)


@pytest.mark.parametrize("kind", KINDS)
def test_ops_wrappers_return_the_same_tensors(dev, kind):
    """kb.ops.unpack_sequence_frames / unpack_packed_sequence_frames: the frame tuples, the outputs' order, middle_only."""
    rng = np.random.default_rng(29)
    samples = [_sample(rng, 9, 17, 3, 16), _sample(rng, 8, 16, 3, 16)]
    starts, shape = [(4, 9), (0, 8)], (5, 8)
    images, depths, place = _buffers(kind, samples, dev)
    want = _expected(samples, starts, shape)
    if kind == "raw":
        frames = [tuple(place[id(s[k])][0] for k in range(4)) + s[1].shape[:2] + start for s, start in zip(samples, starts)]
        got = kb.ops.unpack_sequence_frames(images, depths, frames, shape, channels=3, depth_bits=16)
    else:
        frames = [sum((place[id(s[k])] for k in range(4)), ()) + s[1].shape[:2] + start for s, start in zip(samples, starts)]
        got = kb.ops.unpack_packed_sequence_frames(images, depths, frames, shape, channels=3, depth_bits=16)
        image0, depth = kb.ops.unpack_packed_sequence_frames(images, depths, frames, shape, channels=3, depth_bits=16, middle_only=True)
        assert np.array_equal(image0.cpu().numpy(), want["image0"]) and np.array_equal(depth.cpu().numpy(), want["depth"])
    for name, t in zip(("image0", "image1", "image2", "depth"), got):
        assert np.array_equal(t.cpu().numpy(), want[name]), name
