"""GPU: the device decoder of the packed frame store.  ops.unpack_packed_frames against ops.unpack_train_frames /
ops.unpack_frames on the same frames' raw bytes and against NumPy slices; both loaders over packed files against themselves over
the PNG files the packed ones were made from.  The packed files are made by kbn_frame_encode (compared byte for byte with
the NumPy encoder in tests/test_frame_pack_cpu.py) or, for the format's sake, by hand (tests/frame_pack_oracle.py: header bytes wider
than needed, nonzero pad bits, random field bits); every one passes kbn_frame_check before its bytes go to the device."""
import filecmp
import functools
import os
import struct

import numpy as np
import pytest
import torch

import frame_pack_oracle as orc
import kbnet_amd as kb
import run_cases as rc
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu
KbnError = kb._lib.KbnError
TRAIN_IO = os.path.join(GOLDEN_DIR, "train_io")
IO = os.path.join(GOLDEN_DIR, "io")
T_IMAGES = [os.path.join(TRAIN_IO, f"triplet_{i}.png") for i in range(4)]
T_DEPTHS = [os.path.join(TRAIN_IO, f"depth_{i}.png") for i in range(4)]
T_KS = [os.path.join(TRAIN_IO, f"k_{i}.npy") for i in range(4)]


def read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need a visible MI355X (run with -m gpu on a GPU box)")
    kb._lib.load()
    return torch.device("cuda:0")


RAW = [kb.loader.decode_png(read(p)) for p in T_IMAGES]      # H x 3W x 3 uint8: thirds of 24 x 40, 26 x 44, 25 x 43, 24 x 40
DEP = [kb.loader.decode_png(read(p)) for p in T_DEPTHS]      # H x W uint16


def stage_files(files, lead=0):
    """Ready-made packed files in one buffer, each at a 16-byte-aligned offset (the first at `lead`): (bytes, [(offset, size)]).
    Every file passes kbn_frame_check first: nothing the host refuses goes to the device."""
    flat, places = bytearray(lead), []
    for data in files:
        kb.loader.check_frame(bytes(data))
        flat += b"\xee" * (-len(flat) % 16)
        places.append((len(flat), len(data)))
        flat += data
    return np.frombuffer(bytes(flat), dtype=np.uint8), places


def stage(arrays, lead=0):
    """stage_files of the encoder's files of `arrays`."""
    return stage_files([kb.loader.encode_frame(a) for a in arrays], lead)


def stage_raw(arrays):
    flat, places = bytearray(), []
    for a in arrays:
        flat += b"\xee" * (-len(flat) % 16)
        places.append(len(flat))
        flat += np.ascontiguousarray(a).tobytes()
    return np.frombuffer(bytes(flat), dtype=np.uint8), places


def both(dev, raws, deps, starts, shape, channels=3, depth_bits=16, lead=0):
    """(packed decoder's four tensors, raw-byte kernel's four tensors) for the same frames and crops."""
    pi, pip = stage(raws, lead)
    pd, pdp = stage(deps, lead)
    ri, rip = stage_raw(raws)
    rd, rdp = stage_raw(deps)
    sizes = [(d.shape[0], d.shape[1]) for d in deps]
    packed = kb.ops.unpack_packed_frames(torch.from_numpy(pi.copy()).to(dev), torch.from_numpy(pd.copy()).to(dev),
                                         [(a, n, b, m, h, w, y, x) for (a, n), (b, m), (h, w), (y, x) in zip(pip, pdp, sizes, starts)], shape,
                                         channels=channels, depth_bits=depth_bits)
    plain = kb.ops.unpack_train_frames(torch.from_numpy(ri.copy()).to(dev), torch.from_numpy(rd.copy()).to(dev),
                                       [(a, b, h, w, y, x) for a, b, (h, w), (y, x) in zip(rip, rdp, sizes, starts)], shape,
                                       channels=channels, depth_bits=depth_bits)
    return packed, plain


def both_files(dev, image_files, depth_files, starts, shape, channels=3, depth_bits=16):
    """both() for ready-made files: (packed decoder's tensors from the files, raw-byte kernel's tensors from the samples the HOST
    decoder gives for the same files, those samples)."""
    raws, deps = [kb.loader.decode_frame(f) for f in image_files], [kb.loader.decode_frame(f) for f in depth_files]
    pi, pip = stage_files(image_files)
    pd, pdp = stage_files(depth_files)
    ri, rip = stage_raw(raws)
    rd, rdp = stage_raw(deps)
    sizes = [(d.shape[0], d.shape[1]) for d in deps]
    packed = kb.ops.unpack_packed_frames(torch.from_numpy(pi.copy()).to(dev), torch.from_numpy(pd.copy()).to(dev),
                                         [(a, n, b, m, h, w, y, x) for (a, n), (b, m), (h, w), (y, x) in zip(pip, pdp, sizes, starts)], shape,
                                         channels=channels, depth_bits=depth_bits)
    plain = kb.ops.unpack_train_frames(torch.from_numpy(ri.copy()).to(dev), torch.from_numpy(rd.copy()).to(dev),
                                       [(a, b, h, w, y, x) for a, b, (h, w), (y, x) in zip(rip, rdp, sizes, starts)], shape,
                                       channels=channels, depth_bits=depth_bits)
    return packed, plain, raws, deps


def slices(raw, dep, y, x, h, w):
    """NumPy: the three thirds (t, t-1, t+1) as 3 x h x w float32 and the depth / 256."""
    if raw.ndim == 2:
        raw = np.repeat(raw[:, :, None], 3, axis=2)
    W = raw.shape[1] // 3
    out = [np.ascontiguousarray(raw[y:y + h, t * W + x:t * W + x + w, :3].transpose(2, 0, 1)).astype(np.float32) for t in (1, 0, 2)]
    return out + [(dep[y:y + h, x:x + w].astype(np.float32) / np.float32(256.0))[None]]


def assert_same(packed, plain, raws, deps, starts, shape, what=""):
    for name, a, b in zip(("image0", "image1", "image2", "depth"), packed, plain):
        assert torch.equal(a, b), (what, name)
    host = [t.cpu().numpy() for t in packed]
    for i, (raw, dep, (y, x)) in enumerate(zip(raws, deps, starts)):
        for name, got, want in zip(("image0", "image1", "image2", "depth"), host, slices(raw, dep, y, x, *shape)):
            assert np.array_equal(got[i], want), (what, i, name)


@pytest.mark.parametrize("shape", [(16, 24), (13, 21), (15, 22)], ids=["16x24-vector", "13x21-scalar", "15x22-scalar"])
def test_packed_decoder_equals_the_raw_byte_kernel_at_every_crop_origin(dev, shape):
    """Four frames of three raw sizes in one launch (W = 43 puts the thirds at columns 43 and 86, inside segments): y_start on, before
    and behind a group boundary and at the last row that fits, x_start on, before and behind a segment boundary and at the last
    column that fits -- per frame, clamped to what its size allows."""
    h, w = shape
    for y in (0, 7, 8, 9, 10 ** 6):
        for x in (0, 3, 15, 16, 17, 10 ** 6):
            starts = [(min(y, d.shape[0] - h), min(x, d.shape[1] - w)) for d in DEP]
            packed, plain = both(dev, RAW, DEP, starts, shape)
            assert_same(packed, plain, RAW, DEP, starts, shape, (y, x))
    assert {d.shape[0] - h for d in DEP} >= {24 - h, 26 - h} and max(d.shape[0] - h for d in DEP) >= 9


def test_full_size_crop_and_the_same_bits_twice(dev):
    raws, deps = [RAW[0], RAW[3]], [DEP[0], DEP[3]]
    starts = [(0, 0), (0, 0)]
    packed, plain = both(dev, raws, deps, starts, (24, 40))
    assert_same(packed, plain, raws, deps, starts, (24, 40))
    again, _ = both(dev, raws, deps, starts, (24, 40))
    for a, b in zip(packed, again):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("depth_bits", [8, 16])
@pytest.mark.parametrize("channels", [1, 3, 4])
def test_channels_and_depth_widths(dev, channels, depth_bits):
    """Gray is replicated, alpha dropped; 8- and 16-bit depth.  19 x 21 thirds: a short last group, thirds at columns 21 and 42."""
    g = np.random.Generator(np.random.Philox(channels * 100 + depth_bits))
    raws = [g.integers(0, 256, size=(19, 63) if channels == 1 else (19, 63, channels), dtype=np.uint8) for _ in range(2)]
    raws[1] = (raws[1] // 16 + np.arange(63).reshape((1, 63) + (1,) * (raws[1].ndim - 2))).astype(np.uint8)      # smooth: narrow fields
    top = (1 << depth_bits) - 1
    deps = [np.where(g.random((19, 21)) < 0.3, g.integers(1, top + 1, size=(19, 21)), 0).astype(np.uint16 if depth_bits == 16 else np.uint8)
            for _ in range(2)]
    deps[0][5, 5], deps[0][5, 6], deps[0][6, 5] = top, 0, 0
    for shape, starts in (((13, 17), [(5, 3), (6, 4)]), ((19, 21), [(0, 0), (0, 0)]), ((8, 16), [(8, 5), (11, 0)])):
        packed, plain = both(dev, raws, deps, starts, shape, channels=channels, depth_bits=depth_bits)
        assert_same(packed, plain, raws, deps, starts, shape, shape)


# ------------------------------------------------------------------------------------- files no encoder of ours writes
# The format is the contract: any file kbn_frame_check accepts, canonical or not, decodes on the device to what the host decoder and
# the NumPy oracle make of it.  Thirds of 25 x 43 (raw width 129: thirds begin inside segments, a short last group of one row, a short
# last segment of one sample) and of 19 x 21 (raw width 63).
@functools.lru_cache(maxsize=None)
def hand_made(choice, w, h, c, bits):
    data, samples = orc.hand_made(choice, w, h, c, bits, seed=3)
    assert np.array_equal(orc.decode(data), samples) and data != kb.loader.encode_frame(samples)
    return data, samples


@pytest.mark.parametrize("depth_bits", [8, 16])
@pytest.mark.parametrize("channels", [1, 3, 4])
@pytest.mark.parametrize("choice", orc.WIDTH_CHOICES)
def test_hand_made_files_decode_on_the_device_as_on_the_host(dev, choice, channels, depth_bits):
    """Image and depth file both hand-made, by each of the four width choices: crops (13, 21) from (6, 4) and (9, 17), clamped to the
    smaller frame; (16, 24) from (8, 16), the 16-byte store path; the full frames.  Every launch twice: the same bits."""
    image = {hw: hand_made(choice, 3 * hw[1], hw[0], channels, 8) for hw in ((25, 43), (19, 21))}
    depth = {hw: hand_made(choice, hw[1], hw[0], 1, depth_bits) for hw in ((25, 43), (19, 21))}
    big, small = (25, 43), (19, 21)
    launches = [((13, 21), [big, small, big, small], [(6, 4), (6, 0), (9, 17), (0, 0)]),
                ((16, 24), [big], [(8, 16)]),
                ((25, 43), [big, big], [(0, 0), (0, 0)]),
                ((19, 21), [small], [(0, 0)])]
    for shape, frames, starts in launches:
        ifiles, dfiles = [image[hw][0] for hw in frames], [depth[hw][0] for hw in frames]
        packed, plain, raws, deps = both_files(dev, ifiles, dfiles, starts, shape, channels=channels, depth_bits=depth_bits)
        for hw, raw, dep in zip(frames, raws, deps):      # the host decoder gave the oracle's samples
            assert np.array_equal(raw, image[hw][1]) and np.array_equal(dep, depth[hw][1])
        assert_same(packed, plain, raws, deps, starts, shape, (choice, shape))
        again = both_files(dev, ifiles, dfiles, starts, shape, channels=channels, depth_bits=depth_bits)[0]
        for a, b in zip(packed, again):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (choice, shape)


@pytest.mark.parametrize("choice", orc.WIDTH_CHOICES[:3])
def test_a_canonical_and_a_hand_made_file_of_one_frame_in_one_launch(dev, choice):
    """Frame 0 the encoder's files, frame 1 hand-made files of the same samples: identical outputs."""
    ifile, raw = hand_made(choice, 129, 25, 3, 8)
    dfile, dep = hand_made(choice, 43, 25, 1, 16)
    canonical = kb.loader.encode_frame(raw), kb.loader.encode_frame(dep)
    assert canonical[0] != ifile and canonical[1] != dfile
    for shape, start in (((13, 21), (9, 17)), ((16, 24), (8, 16)), ((25, 43), (0, 0))):
        packed, plain, raws, deps = both_files(dev, [canonical[0], ifile], [canonical[1], dfile], [start, start], shape)
        assert_same(packed, plain, raws, deps, [start, start], shape, (choice, shape))
        for t in packed:
            assert torch.equal(t[0].view(torch.int32), t[1].view(torch.int32)), (choice, shape)


def test_a_third_narrower_than_a_segment(dev):
    """W = 5: all three thirds lie in the triplet's only segment."""
    g = np.random.Generator(np.random.Philox(55))
    raws = [g.integers(0, 256, size=(9, 15, 3), dtype=np.uint8)]
    deps = [g.integers(0, 65536, size=(9, 5), dtype=np.uint16)]
    for shape, starts in (((9, 5), [(0, 0)]), ((3, 2), [(6, 3)]), ((1, 1), [(8, 4)])):
        packed, plain = both(dev, raws, deps, starts, shape)
        assert_same(packed, plain, raws, deps, starts, shape, shape)


def test_a_crop_wider_than_one_tile(dev):
    """The kernel walks a row in tiles of 240 output columns: 250 and 484 columns take two and three, at an odd phase."""
    g = np.random.Generator(np.random.Philox(77))
    raws = [(g.integers(0, 8, size=(10, 3 * 491, 3)) + np.arange(3 * 491).reshape(1, -1, 1)).astype(np.uint8)]
    deps = [np.where(g.random((10, 491)) < 0.05, g.integers(1, 65536, size=(10, 491)), 0).astype(np.uint16)]
    for shape, starts in (((9, 250), [(1, 7)]), ((10, 484), [(0, 5)]), ((3, 241), [(7, 250)])):
        packed, plain = both(dev, raws, deps, starts, shape)
        assert_same(packed, plain, raws, deps, starts, shape, shape)


def test_middle_third_only_equals_unpack_frames(dev):
    """image1 = image2 = NULL, the inference loader's form, against ops.unpack_frames on the decoded bytes."""
    raws, deps = [RAW[0], RAW[3]], [DEP[0], DEP[3]]
    pi, pip = stage(raws)
    pd, pdp = stage(deps)
    frames = [(a, n, b, m, 24, 40, 0, 0) for (a, n), (b, m) in zip(pip, pdp)]
    image, depth = kb.ops.unpack_packed_frames(torch.from_numpy(pi.copy()).to(dev), torch.from_numpy(pd.copy()).to(dev), frames, (24, 40),
                                               middle_only=True)
    want_image, want_depth = kb.ops.unpack_frames(torch.from_numpy(np.stack(raws)).to(dev), torch.from_numpy(np.stack(deps).view(np.int16)).to(dev),
                                                  width=40, x_offset=40)
    assert torch.equal(image, want_image) and torch.equal(depth, want_depth)
    for i in range(2):
        assert np.array_equal(image[i].cpu().numpy(), slices(raws[i], deps[i], 0, 0, 24, 40)[0])


def test_payloads_at_every_residue(dev):
    """Files at 16-byte-aligned offsets that are no multiples of 32 or 64, and (group, plane) payloads that begin at every residue
    mod 4: the decoder's field reads are byte reads, no alignment is assumed.  Noise of 0 to 7 bits by column on a ramp makes
    segments of many sizes."""
    g = np.random.Generator(np.random.Philox(4))
    raws = [((g.integers(0, 256, size=(h, 3 * w, 3)) >> (np.arange(3 * w) % 9).reshape(1, -1, 1)) + np.arange(3 * w).reshape(1, -1, 1)).astype(np.uint8)
            for h, w in ((24, 40), (26, 44), (25, 43))]
    deps = [np.where(g.random(r.shape[:2]) < 0.2, g.integers(1, 65536, size=r.shape[:2]), 0).astype(np.uint16)[:, :r.shape[1] // 3] for r in raws]
    residues = set()
    for raw in raws:
        data = kb.loader.encode_frame(raw)
        groups = -(-raw.shape[0] // 8)
        start = (32 + 4 * (groups * 3 + 1) + 15) // 16 * 16
        residues |= {(start + t) % 4 for t in struct.unpack(f"<{groups * 3}I", data[32:32 + 12 * groups])}
    assert residues == {0, 1, 2, 3}
    starts = [(d.shape[0] - 16, d.shape[1] - 24) for d in deps]
    for lead in (0, 16, 48, 80):
        packed, plain = both(dev, raws, deps, starts, (16, 24), lead=lead)
        assert_same(packed, plain, raws, deps, starts, (16, 24), lead)


def test_more_frames_than_a_launch_carries(dev):
    """67 frames of 8 x 12: two launches, the second with three records."""
    g = np.random.Generator(np.random.Philox(67))
    raws = [g.integers(0, 256, size=(8, 36, 3), dtype=np.uint8) for _ in range(67)]
    deps = [g.integers(0, 65536, size=(8, 12), dtype=np.uint16) for _ in range(67)]
    starts = [(i % 4, i % 6) for i in range(67)]
    assert kb._lib.KBN_UNPACK_TRAIN_MAX_FRAMES == 64
    packed, plain = both(dev, raws, deps, starts, (5, 7))
    assert_same(packed, plain, raws, deps, starts, (5, 7))


# ------------------------------------------------------------------------------------- the loaders
@pytest.fixture(scope="module")
def packed_files(tmp_path_factory):
    """The train-loader sample files and the golden/io frames as packed files: name -> path."""
    root = tmp_path_factory.mktemp("packed")
    src = T_IMAGES + T_DEPTHS + [os.path.join(IO, f"triplet_{i}.png") for i in range(3)] + [os.path.join(IO, f"depth_{i}.png") for i in range(3)]
    dst = [str(root / ("train_" + os.path.basename(p)[:-4] + ".kbf")) for p in src[:8]] + [str(root / ("io_" + os.path.basename(p)[:-4] + ".kbf")) for p in src[8:]]
    kb.loader.pack_frames(src, dst, workers=4)
    return dict(zip(src, dst))


def epoch(loader):
    return [[t.clone() for t in batch] for batch in loader]


def assert_epochs_equal(a, b, what=""):
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        assert len(x) == len(y) == 5
        for j, (s, t) in enumerate(zip(x, y)):
            assert s.shape == t.shape and torch.equal(s, t), (what, i, j)


def pair(packed_files, dev, order=(0, 1, 2, 3), generator_seed=None, **arguments):
    """The same loader twice: over the PNG lists and over the packed lists, each with a generator of its own under the same seed."""
    images, depths, ks = [T_IMAGES[i] for i in order], [T_DEPTHS[i] for i in order], [T_KS[i] for i in order]
    generator = lambda: None if generator_seed is None else torch.Generator().manual_seed(generator_seed)
    make = lambda im, de: kb.loader.TrainingFrameLoader(im, de, ks, device=dev, workers=3, generator=generator(), **arguments)
    return make(images, depths), make([packed_files[p] for p in images], [packed_files[p] for p in depths])


@pytest.mark.parametrize("batch", [1, 2, 3, 4])
def test_training_loader_over_packed_files_equals_itself_over_pngs(dev, packed_files, batch):
    for crop_type, shape in ((["horizontal", "vertical"], (16, 24)), (["horizontal", "anchored", "bottom"], (13, 21))):
        for shuffle in (False, True):
            epochs = []
            for loader in pair(packed_files, dev, shape=list(shape), random_crop_type=crop_type, batch_size=batch, shuffle=shuffle,
                               generator_seed=11 if shuffle else None, prefetch=2):
                np.random.seed(21)
                epochs.append(epoch(loader) + epoch(loader))
            assert_epochs_equal(*epochs, (crop_type, shuffle))
            assert sum(b[0].shape[0] for b in epochs[1]) == 8


def test_training_loader_without_a_crop(dev, packed_files):
    epochs = [epoch(loader) for loader in pair(packed_files, dev, order=(0, 3), shape=None, batch_size=2, shuffle=False)]
    assert_epochs_equal(*epochs)
    assert tuple(epochs[1][0][0].shape) == (2, 3, 24, 40)


@pytest.mark.parametrize("rank", [0, 1])
def test_sharded_training_loader(dev, packed_files, rank):
    epochs = []
    for loader in pair(packed_files, dev, shape=[16, 24], random_crop_type=["horizontal", "vertical"], batch_size=3, shuffle=True,
                       generator_seed=5, rank=rank, world=2, crops="global", prefetch=2):
        np.random.seed(8)
        epochs.append(epoch(loader))
    assert_epochs_equal(*epochs, rank)
    assert [b[0].shape[0] for b in epochs[1]] == ([2, 1] if rank == 0 else [1, 0])


def test_training_loader_continues_an_epoch_from_its_state(dev, packed_files):
    """An epoch left after its first batch and continued by another loader through state_dict() / load_state_dict(): packed and PNG
    give the same state and the same remaining batches, which are those of the uninterrupted epoch."""
    arguments = dict(shape=[16, 24], random_crop_type=["horizontal", "vertical"], batch_size=1, shuffle=True, prefetch=2)
    whole, states, rests = [], [], []
    for k in range(2):
        loaders = pair(packed_files, dev, generator_seed=3, **arguments)
        np.random.seed(13)
        whole.append(epoch(loaders[k]))
        first = pair(packed_files, dev, generator_seed=3, **arguments)[k]
        np.random.seed(13)
        it = iter(first)
        head = [t.clone() for t in next(it)]
        states.append(first.state_dict())
        second = pair(packed_files, dev, generator_seed=99, **arguments)[k]
        second.load_state_dict(states[-1])
        rests.append([head] + epoch(second))
        for f in first._pending:
            f.exception()
    assert states[0] == states[1] and states[0]["next"] == 1
    assert_epochs_equal(rests[0], rests[1])
    assert_epochs_equal(whole[1], rests[1])
    assert_epochs_equal(whole[0], whole[1])


def test_a_mixed_batch_raises_at_its_turn(dev, packed_files):
    """Sample 2 packed, the others PNG: at batch size 2 the second batch is mixed and raises when it is due, naming two of its
    files; the same object then serves a clean epoch at batch size 1, where every batch is of one kind."""
    images = T_IMAGES[:2] + [packed_files[T_IMAGES[2]], T_IMAGES[3]]
    depths = T_DEPTHS[:2] + [packed_files[T_DEPTHS[2]], T_DEPTHS[3]]
    loader = kb.loader.TrainingFrameLoader(images, depths, T_KS, shape=(16, 24), random_crop_type=["bottom"], batch_size=2, shuffle=False, device=dev)
    it = iter(loader)
    first = [t.clone() for t in next(it)]
    with pytest.raises(KbnError, match="all PNG or all packed") as info:
        next(it)
    assert os.path.basename(images[2]) in str(info.value) and "triplet_3.png" in str(info.value)
    loader.batch_size = 1
    clean = epoch(loader)
    want = epoch(kb.loader.TrainingFrameLoader(T_IMAGES, T_DEPTHS, T_KS, shape=(16, 24), random_crop_type=["bottom"], batch_size=1, shuffle=False, device=dev))
    assert_epochs_equal(clean, want)
    assert all(torch.equal(a[:1], b) for a, b in zip(first, want[0]))
    # the inference loader: the same refusal, and the same recovery
    io_images = [os.path.join(IO, f"triplet_{i}.png") for i in range(3)]
    io_depths = [os.path.join(IO, f"depth_{i}.png") for i in range(3)]
    ks = [os.path.join(IO, f"k_{i}.npy") for i in range(3)]
    mixed = kb.loader.InferenceFrameLoader(io_images, [io_depths[0], packed_files[io_depths[1]], io_depths[2]], ks, batch_size=1, device=dev)
    it = iter(mixed)
    next(it)
    with pytest.raises(KbnError, match="all PNG or all packed"):
        next(it)


@pytest.mark.parametrize("batch", [1, 2, 3])
def test_inference_loader_over_packed_files(dev, packed_files, batch):
    io_images = [os.path.join(IO, f"triplet_{i}.png") for i in range(3)]
    io_depths = [os.path.join(IO, f"depth_{i}.png") for i in range(3)]
    ks = [os.path.join(IO, f"k_{i}.npy") for i in range(3)]
    got = [[t.clone() for t in b] for b in kb.loader.InferenceFrameLoader([packed_files[p] for p in io_images], [packed_files[p] for p in io_depths], ks,
                                                                          batch_size=batch, device=dev, workers=3)]
    want = [[t.clone() for t in b] for b in kb.loader.InferenceFrameLoader(io_images, io_depths, ks, batch_size=batch, device=dev, workers=3)]
    assert len(got) == len(want) == -(-3 // batch)
    for g, w in zip(got, want):
        assert all(a.shape == b.shape and torch.equal(a, b) for a, b in zip(g, w))


def test_inference_run_takes_packed_lists(dev, packed_files, tmp_path):
    """kb.inference.run only passes its path lists on: from packed image and sparse-depth lists it gives the per-frame metrics and
    the output files it gives from the PNG lists (the ground truth stays PNG)."""
    results, outputs = [], []
    for name in ("png", "packed"):
        directory = tmp_path / name
        directory.mkdir()
        lists = list(rc.path_lists())
        if name == "packed":
            lists[0], lists[1] = [packed_files[p] for p in lists[0]], [packed_files[p] for p in lists[1]]
        files = [str(directory / f"{i}.txt") for i in range(4)]
        for path, paths in zip(files, lists):
            kb.loader.write_paths(path, paths)
        checkpoint_path = str(directory / "run")
        results.append(kb.inference.run(files[0], files[1], files[2], ground_truth_path=files[3], checkpoint_path=checkpoint_path,
                                        depth_model_restore_path=rc.CHECKPOINT, save_outputs=True, batch_size=2, return_results=True,
                                        **rc.run_settings(kb.kitti_config().narrow())))
        outputs.append(os.path.join(checkpoint_path, "outputs"))
    assert torch.equal(results[0]["per_frame"], results[1]["per_frame"]) and results[0]["per_frame"].shape == (3, 4)
    assert torch.equal(results[0]["output_depth"], results[1]["output_depth"])
    for directory in rc.DIRECTORIES:
        names = sorted(os.listdir(os.path.join(outputs[0], directory)))
        assert names == sorted(os.listdir(os.path.join(outputs[1], directory))) and len(names) == 3
        for n in names:
            assert filecmp.cmp(os.path.join(outputs[0], directory, n), os.path.join(outputs[1], directory, n), shallow=False), (directory, n)
