"""GPU: the staging sets both loaders share (kb.loader._Staging).  One set per slot serves PNG batches and packed batches
in turn, and a batch that needs more than the set holds replaces its buffers after the copies that last used them.  Expected values
come from the PNG files through the reference-named NumPy functions (load_image_triplet, load_image, load_depth, random_crop),
never through a loader.

Frames of three raw sizes, crops drawn by ["horizontal", "vertical"]: np.random.randint(0, 0) raises, in the reference as here, so
an unanchored crop must be smaller than the smallest frame, 16 x 24, in both directions.  (12, 20) takes the 16-byte stores,
(13, 21) the float-by-float ones.  A (16, 24) crop, as large as the smallest frame, can only be drawn 'anchored'; it runs so."""
import numpy as np
import pytest
import torch
from PIL import Image

import kbnet_amd as kb

pytestmark = pytest.mark.gpu
RAW_SIZES = [(16, 24), (16, 24), (24, 40), (24, 40), (40, 56), (40, 56)]      # height, width of a third: every batch of two outgrows the last
CROPS = [((12, 20), ["horizontal", "vertical"]), ((13, 21), ["horizontal", "vertical"]), ((16, 24), ["horizontal", "vertical", "anchored"])]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need a visible MI355X (run with -m gpu on a GPU box)")
    kb._lib.load()
    return torch.device("cuda:0")


def write_samples(root, sizes, seed, gray=False):
    """One PNG triplet (or gray single image), one sparse 16-bit depth PNG and one intrinsics file per (height, width): three lists."""
    g = np.random.Generator(np.random.Philox(seed))
    images, depths, ks = [], [], []
    for i, (h, w) in enumerate(sizes):
        images.append(str(root / f"image_{i}.png"))
        depths.append(str(root / f"depth_{i}.png"))
        ks.append(str(root / f"k_{i}.npy"))
        Image.fromarray(g.integers(0, 256, size=(h, w) if gray else (h, 3 * w, 3), dtype=np.uint8)).save(images[-1])
        Image.fromarray(np.where(g.random((h, w)) < 0.3, g.integers(1, 65536, size=(h, w)), 0).astype(np.uint16)).save(depths[-1])
        np.save(ks[-1], np.array([[700.0 + 10 * i, 0.0, w / 2 + 0.25], [0.0, 710.0 + 10 * i, h / 2 - 0.5], [0.0, 0.0, 1.0]]))
    return images, depths, ks


def alternate_kinds(root, images, depths):
    """Batches of two: 0 and 2 stay PNG, batch 1 (samples 2 and 3) becomes its packed twin."""
    images, depths = list(images), list(depths)
    src = images[2:4] + depths[2:4]
    dst = [str(root / (p.rsplit("/", 1)[1][:-4] + ".kbf")) for p in src]
    kb.loader.pack_frames(src, dst, workers=2)
    images[2:4], depths[2:4] = dst[:2], dst[2:]
    return images, depths


def same_bits(tensor, array):
    got = tensor.cpu().numpy()
    want = np.ascontiguousarray(array, dtype=np.float32)
    return got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.fixture(scope="module")
def training_files(tmp_path_factory):
    root = tmp_path_factory.mktemp("staging_train")
    pngs = write_samples(root, RAW_SIZES, seed=22)
    return pngs, alternate_kinds(root, *pngs[:2])


def reference_epochs(pngs, shape, crop_type, epochs):
    """What KBNetTrainingDataset.__getitem__ (reference src/datasets.py:199-225) returns for the samples in index order, `epochs`
    times over under the np.random state it finds: [[five float32 arrays] a sample] an epoch."""
    out = []
    for _ in range(epochs):
        out.append([])
        for image, depth, k in zip(*pngs):
            image1, image0, image2 = kb.loader.load_image_triplet(image, normalize=False)
            sparse_depth0 = kb.loader.load_depth(depth, data_format="CHW")
            intrinsics = np.load(k).astype(np.float32)
            cropped, intrinsics = kb.loader.random_crop([image0, image1, image2, sparse_depth0], shape, intrinsics=intrinsics, crop_type=crop_type)
            out[-1].append([a.astype(np.float32) for a in cropped + [intrinsics]])
    return out


@pytest.mark.parametrize("shape,crop_type", CROPS)
def test_training_batches_share_and_outgrow_their_sets(dev, training_files, shape, crop_type):
    """batch_size 2, prefetch 1: two sets.  Batch 1 is packed between two PNG batches; batch 2 takes batch 0's set and needs five
    times its bytes.  The second epoch starts on the sets the first left.  All five tensors, bit for bit."""
    pngs, (images, depths) = training_files
    np.random.seed(31)
    want = reference_epochs(pngs, shape, crop_type, epochs=2)
    loader = kb.loader.TrainingFrameLoader(images, depths, pngs[2], shape=list(shape), random_crop_type=crop_type, batch_size=2, prefetch=1,
                                           shuffle=False, device=dev, workers=2)
    np.random.seed(31)
    for e in range(2):
        batches = [[t.clone() for t in batch] for batch in loader]
        assert [tuple(b[0].shape) for b in batches] == [(2, 3) + tuple(shape)] * 3
        for b, batch in enumerate(batches):
            for j in range(2):
                for t, (got, expected) in enumerate(zip(batch, want[e][2 * b + j])):
                    assert same_bits(got[j], expected), (e, b, j, t)
    assert loader._serial == 6


@pytest.fixture(scope="module")
def inference_files(tmp_path_factory):
    root = tmp_path_factory.mktemp("staging_inference")
    pngs = write_samples(root, [(16, 24)] * 6, seed=23)
    return pngs, alternate_kinds(root, *pngs[:2])


def test_inference_batches_share_their_sets(dev, inference_files):
    """Six frames of 16 x (3 x 24), batch_size 2, prefetch 1: PNG, packed, PNG through two sets; the middle third of the reference."""
    pngs, (images, depths) = inference_files
    loader = kb.loader.InferenceFrameLoader(images, depths, pngs[2], use_image_triplet=True, batch_size=2, prefetch=1, device=dev, workers=2)
    for _ in range(2):
        batches = [[t.clone() for t in batch] for batch in loader]
        assert [b[0].shape[0] for b in batches] == [2, 2, 2]
        for i, (image, depth, k) in enumerate(zip(*pngs)):
            got_image, got_depth, got_k = (t[i % 2] for t in batches[i // 2])
            assert same_bits(got_image, kb.loader.load_image_triplet(image, normalize=False)[1]), i
            assert same_bits(got_depth, kb.loader.load_depth(depth, data_format="CHW")), i
            assert same_bits(got_k, np.load(k).astype(np.float32)), i


def test_inference_gray_images_without_triplets(dev, tmp_path):
    """use_image_triplet=False over single-channel 16 x 24 PNGs: the flat staging bytes viewed as N x H x W x 1, gray replicated to
    three channels as load_image does; three frames, so the last batch is short."""
    images, depths, ks = write_samples(tmp_path, [(16, 24)] * 3, seed=24, gray=True)
    loader = kb.loader.InferenceFrameLoader(images, depths, ks, use_image_triplet=False, batch_size=2, prefetch=1, device=dev, workers=2)
    batches = [[t.clone() for t in batch] for batch in loader]
    assert [tuple(b[0].shape) for b in batches] == [(2, 3, 16, 24), (1, 3, 16, 24)]
    for i in range(3):
        got_image, got_depth, got_k = (t[i % 2] for t in batches[i // 2])
        assert same_bits(got_image, kb.loader.load_image(images[i], normalize=False, data_format="CHW")), i
        assert same_bits(got_depth, kb.loader.load_depth(depths[i], data_format="CHW")), i
        assert same_bits(got_k, np.load(ks[i]).astype(np.float32)), i
