"""GPU: kbn_unpack_train_frames_forward (csrc/unpack_train.hip) bit for bit against NumPy slices of the decoded fixtures, and
kb.loader.TrainingFrameLoader against what the REFERENCE's KBNetTrainingDataset returned from the same files under the same
np.random.seed (tests/golden/train_loader.npz, written by tests/golden/gen_train_loader_golden.py).

    python -m pytest tests/test_train_loader_gpu.py -m gpu -q
"""
import json
import os

import numpy as np
import pytest
import torch
from torch.utils.data import RandomSampler

import kbnet_amd as kb
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

KbnError = kb._lib.KbnError
IO = os.path.join(GOLDEN_DIR, "train_io")
GOLDEN = np.load(os.path.join(GOLDEN_DIR, "train_loader.npz"))
RUNS = {(tuple(r["crop_type"]), tuple(r["shape"]) if r["shape"] else None): r for r in json.loads(bytes(GOLDEN["runs"]).decode())}
IMAGES = [os.path.join(IO, f"triplet_{i}.png") for i in range(4)]
DEPTHS = [os.path.join(IO, f"depth_{i}.png") for i in range(4)]
KS = [os.path.join(IO, f"k_{i}.npy") for i in range(4)]


def read(path):
    with open(path, "rb") as f:
        return f.read()


SIZES = [(24, 40), (26, 44), (25, 43), (24, 40)]


class Decoded:
    """The fixtures decoded on first use: RAW[i] H x 3 W x 3 uint8, DEP[i] H x W uint16."""

    def __init__(self, paths):
        self.paths, self.arrays = paths, {}

    def __getitem__(self, i):
        if i not in self.arrays:
            self.arrays[i] = kb.loader.decode_png(read(self.paths[i]))
            assert self.arrays[i].shape[:2] == (SIZES[i][0], SIZES[i][1] * (3 if self.arrays[i].ndim == 3 else 1))
        return self.arrays[i]


RAW, DEP = Decoded(IMAGES), Decoded(DEPTHS)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need a visible MI355X (run with -m gpu on a GPU box)")
    kb._lib.load()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------------------ the kernel
def variant(sample: int, channels: int, bits: int):
    """(triplet bytes H x 3 W x C, depth samples H x W) of a fixture, with 1 and 4 channels and 8-bit depth derived from it."""
    rgb, z = RAW[sample], DEP[sample]
    image = {1: rgb[:, :, 1], 3: rgb, 4: np.concatenate([rgb, 255 - rgb[:, :, :1]], axis=2)}[channels]
    return np.ascontiguousarray(image), (z if bits == 16 else (z >> 7).astype(np.uint8))


def pack(arrays, gap: int):
    """One buffer, the arrays `gap` bytes apart (any alignment): (uint8 buffer, byte offsets)."""
    offsets, at = [], gap
    for a in arrays:
        offsets.append(at)
        at += a.nbytes + gap
    buf = np.full(at, 0xAB, dtype=np.uint8)
    for a, o in zip(arrays, offsets):
        buf[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
    return buf, offsets


def expected(image, z, y, x, h, w):
    """What the reference's dataset makes of one frame: load_image_triplet's thirds (t, t-1, t+1), cropped; depth / 256."""
    W = z.shape[1]
    rgb = np.repeat(image[:, :, None], 3, axis=2) if image.ndim == 2 else image[:, :, :3]
    thirds = [rgb[:, W:2 * W], rgb[:, :W], rgb[:, 2 * W:]]
    images = [np.transpose(t[y:y + h, x:x + w], (2, 0, 1)).astype(np.float32) for t in thirds]
    return images + [z[None, y:y + h, x:x + w].astype(np.float32) / np.float32(256.0)]


def run_kernel(dev, samples, starts, shape, channels=3, bits=16, gaps=(7, 6)):
    data = [variant(s, channels, bits) for s in sorted(set(samples))]
    where = {s: j for j, s in enumerate(sorted(set(samples)))}
    images, image_at = pack([d[0] for d in data], gaps[0])
    depths, depth_at = pack([d[1] for d in data], gaps[1])
    frames = [(image_at[where[s]], depth_at[where[s]], *SIZES[s], y, x) for s, (y, x) in zip(samples, starts)]
    outs = kb.ops.unpack_train_frames(torch.from_numpy(images).to(dev), torch.from_numpy(depths).to(dev), frames, shape,
                                      channels=channels, depth_bits=bits)
    outs = [o.cpu().numpy() for o in outs]
    assert [o.shape for o in outs] == [(len(samples), 3, *shape)] * 3 + [(len(samples), 1, *shape)]
    for n, (s, (y, x)) in enumerate(zip(samples, starts)):
        want = expected(*data[where[s]], y, x, *shape)
        for name, got, exp in zip(("image0", "image1", "image2", "sparse_depth0"), outs, want):
            assert got.dtype == np.float32 and np.array_equal(got[n].view(np.uint32), exp.view(np.uint32)), (name, n, s, y, x)


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("channels", [1, 3, 4])
@pytest.mark.parametrize("shape", [(16, 24), (13, 21), (15, 22)], ids=["16x24-vector", "13x21-scalar", "15x22-scalar"])
def test_kernel_bit_exact_against_numpy_slices(dev, shape, channels, bits):
    """All four samples (three raw sizes) in one batch, every corner of the offset range and an odd x_start; the packed buffers
    start their frames at odd byte offsets (images) and at even ones that are no multiple of four (16-bit depth)."""
    samples = [0, 1, 2, 3, 1]
    d = [(SIZES[s][0] - shape[0], SIZES[s][1] - shape[1]) for s in samples]
    starts = [(0, 0), d[1], (0, d[2][1]), (d[3][0], 0), (1, 3)]
    run_kernel(dev, samples, starts, shape, channels, bits)


def test_kernel_full_size_frames(dev):
    run_kernel(dev, [0, 3], [(0, 0), (0, 0)], (24, 40), gaps=(16, 16))
    run_kernel(dev, [2], [(0, 0)], (25, 43))


def test_kernel_launch_boundary(dev):
    """KBN_UNPACK_TRAIN_MAX_FRAMES + 3 frames: two launches from one call, the second with three records."""
    n = kb._lib.KBN_UNPACK_TRAIN_MAX_FRAMES + 3
    samples = [j % 4 for j in range(n)]
    starts = [(j % (SIZES[s][0] - 8 + 1), (3 * j + 1) % (SIZES[s][1] - 12 + 1)) for j, s in enumerate(samples)]
    assert len(set(zip(samples, starts))) == n
    run_kernel(dev, samples, starts, (8, 12))


# ------------------------------------------------------------------------------------------------------------------ the loader
def collect(loader):
    """One epoch as per-sample host arrays, in order: [(image0, image1, image2, depth, k)], and the batch sizes."""
    samples, sizes = [], []
    for batch in loader:
        assert len(batch) == 5 and all(t.is_cuda and t.dtype == torch.float32 for t in batch)
        host = [t.cpu().numpy() for t in batch]
        sizes.append(host[0].shape[0])
        samples += [tuple(t[j] for t in host) for j in range(sizes[-1])]
    return samples, sizes


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("shape", [(16, 24), (13, 21)], ids=["16x24", "13x21"])
@pytest.mark.parametrize("crop_type", [["horizontal"], ["vertical"], ["horizontal", "vertical"], ["horizontal", "vertical", "anchored"]],
                         ids=lambda c: "+".join(c))
@pytest.mark.parametrize("batch", [1, 2, 3, 4])
def test_loader_batches_are_the_reference_datasets(dev, batch, crop_type, shape):
    """shuffle=False under the run's np.random.seed: two epochs are the reference dataset read twice in index order -- the first
    pass's tensors and every intrinsics matrix from the golden, the second pass's tensors from NumPy slices at the golden's
    offsets -- whatever the batch size (short last batches among them) and with 1 or 4 batches in flight."""
    run = RUNS[(tuple(crop_type), shape)]
    g = lambda key: GOLDEN[run["name"] + "::" + key]
    for prefetch in (1, 4):
        loader = kb.loader.TrainingFrameLoader(IMAGES, DEPTHS, KS, shape=list(shape), random_crop_type=crop_type, batch_size=batch,
                                               shuffle=False, device=dev, workers=3, prefetch=prefetch)
        assert len(loader) == -(-4 // batch) and loader.do_random_crop
        np.random.seed(run["np_seed"])
        for epoch in range(2):
            samples, sizes = collect(loader)
            assert sizes == [batch] * (4 // batch) + ([4 % batch] if 4 % batch else [])
            for i, (image0, image1, image2, depth, k) in enumerate(samples):
                j = 4 * epoch + i
                assert same_bits(k, g("k")[j]), (prefetch, j)
                if epoch == 0:
                    want = [g("image0")[i].astype(np.float32), g("image1")[i].astype(np.float32), g("image2")[i].astype(np.float32), g("depth")[i]]
                else:
                    want = expected(RAW[i], DEP[i], *run["starts"][j], *shape)
                for got, exp in zip((image0, image1, image2, depth), want):
                    assert same_bits(got, exp), (prefetch, j)


def test_loader_without_a_crop_and_mixed_sizes(dev):
    """shape=None: the equal frames batch as they are (the reference's outputs); a batch of different sizes raises when it is due,
    naming both; the same object then serves an epoch with a crop shape."""
    run = RUNS[(("horizontal", "vertical"), None)]
    order = [0, 3, 1, 2]
    loader = kb.loader.TrainingFrameLoader([IMAGES[i] for i in order], [DEPTHS[i] for i in order], [KS[i] for i in order], shape=None,
                                           random_crop_type=run["crop_type"], batch_size=2, shuffle=False, device=dev, workers=2, prefetch=2)
    assert not loader.do_random_crop
    it = iter(loader)
    first = [t.cpu().numpy() for t in next(it)]
    for key, got in zip(("image0", "image1", "image2", "depth", "k"), first):
        assert same_bits(got, GOLDEN["full::" + key].astype(np.float32)), key
    with pytest.raises(KbnError, match=r"26 x 44.*25 x 43|25 x 43.*26 x 44") as info:
        next(it)
    assert "triplet_1.png" in str(info.value) and "triplet_2.png" in str(info.value)
    loader.shape = (16, 24)
    loader.random_crop_type = ["bottom"]
    samples, sizes = collect(loader)
    assert sizes == [2, 2]
    for i, got in zip(order, samples):
        y, x = SIZES[i][0] - 16, (SIZES[i][1] - 24) // 2
        for a, b in zip(got[:4], expected(RAW[i], DEP[i], y, x, 16, 24)):
            assert same_bits(a, b), i
        k = np.load(KS[i]).astype(np.float32)
        k[0, 2] -= x
        k[1, 2] -= y
        assert same_bits(got[4], k)


def test_loader_rejects_a_width_that_is_no_triplet(dev, tmp_path):
    """np.split's ValueError in the reference's load_image_triplet; here too, at the batch it belongs to."""
    from PIL import Image
    bad = str(tmp_path / "bad.png")
    Image.fromarray(np.zeros((24, 121, 3), dtype=np.uint8)).save(bad)
    loader = kb.loader.TrainingFrameLoader([IMAGES[0], bad], [DEPTHS[0], DEPTHS[0]], [KS[0], KS[0]], shape=(16, 24), batch_size=1, shuffle=False, device=dev)
    it = iter(loader)
    next(it)
    with pytest.raises(ValueError, match="equal division"):
        next(it)
    # a depth map of another size than its image; a gray triplet beside an RGB one
    loader = kb.loader.TrainingFrameLoader(IMAGES[:2], [DEPTHS[0], DEPTHS[2]], KS[:2], shape=(16, 24), batch_size=2, shuffle=False, device=dev)
    with pytest.raises(KbnError, match="depth_2.png is 25 x 43, image .*triplet_1.png is 26 x 44"):
        next(iter(loader))
    gray = str(tmp_path / "gray.png")
    Image.fromarray(RAW[0][:, :, 1]).save(gray)
    loader = kb.loader.TrainingFrameLoader([IMAGES[0], gray], [DEPTHS[0], DEPTHS[0]], [KS[0], KS[0]], shape=(16, 24), batch_size=2, shuffle=False, device=dev)
    with pytest.raises(KbnError, match="one format: .*gray.png has 1 channels"):
        next(iter(loader))
    loader.batch_size = 1           # alone in its batch the gray triplet is fine: replicated, as PIL's convert('RGB') does
    samples, _ = collect(loader)
    assert same_bits(samples[1][0], np.repeat(RAW[0][None, :, 40:80, 1], 3, axis=0)[:, 4:20, 8:32].astype(np.float32))


def test_loader_shuffle_order_is_the_random_samplers(dev):
    """Under torch.manual_seed(s) the order of two epochs, read from the yielded intrinsics (fx = 700 + 10 i), is RandomSampler's
    drawn twice under the same seed; with a generator of its own likewise."""
    for generator_seed in (None, 5):
        make = lambda: None if generator_seed is None else torch.Generator().manual_seed(generator_seed)
        torch.manual_seed(1234)
        generator = make()
        want = [list(RandomSampler(range(4), generator=generator)) for _ in range(2)]
        assert all(sorted(w) == [0, 1, 2, 3] for w in want)
        torch.manual_seed(1234)
        loader = kb.loader.TrainingFrameLoader(IMAGES, DEPTHS, KS, shape=(16, 24), random_crop_type=["horizontal", "vertical"], batch_size=3,
                                               shuffle=True, device=dev, generator=make())
        np.random.seed(3)
        got = []
        for _ in range(2):
            samples, sizes = collect(loader)
            assert sizes == [3, 1]
            got.append([int(round((float(s[4][0, 0]) - 700.0) / 10.0)) for s in samples])
        assert got == want, (generator_seed, got, want)


def test_loader_feeds_the_training_step(dev):
    """One batch through transforms.train_inputs (reference src/kbnet.py:396-422): shapes, dtype, image range 0..1."""
    loader = kb.loader.TrainingFrameLoader(IMAGES, DEPTHS, KS, shape=(16, 24), random_crop_type=["horizontal", "vertical"], batch_size=4,
                                           shuffle=False, device=dev)
    np.random.seed(2)
    image0, image1, image2, sparse_depth0, intrinsics = next(iter(loader))
    assert intrinsics.shape == (4, 3, 3)
    # the 16 x 24 crops are too small for a network's five stride-2 levels: tile them to 96 x 144 on the device
    image0, image1, image2, sparse_depth0 = (t.repeat(1, 1, 6, 6) for t in (image0, image1, image2, sparse_depth0))
    transforms = kb.transforms.Transforms(normalized_image_range=[0, 1], random_flip_type=["horizontal"], random_remove_points=[0.60, 0.70],
                                          random_noise_type="none", random_noise_spread=-1, seed=3)
    torch.manual_seed(1)
    outs = kb.transforms.train_inputs(transforms, image0, image1, image2, sparse_depth0, 1.0)
    assert [tuple(o.shape) for o in outs] == [(4, 3, 96, 144)] * 3 + [(4, 1, 96, 144)] * 3 and all(o.dtype == torch.float32 for o in outs)
    for image in outs[:3]:
        assert 0.0 <= float(image.min()) and 0.5 < float(image.max()) <= 1.0
    assert 0 < int((outs[3] > 0).sum()) < int((sparse_depth0 > 0).sum())
