"""GPU: ops.export_pack (kbn_export_pack_forward, csrc/export_pack.hip) bit for bit against the NumPy oracle of tests/run_cases.py
(whose power tests/test_run_cpu.py shows): every source alone and all three, the three (scale, shift) pairs, shapes that take the
16-byte path, the scalar path and more than one block, misaligned sources, outputs inside guarded buffers.

    python -m pytest tests/test_export_pack_gpu.py -m gpu -q
"""
import numpy as np
import pytest
import torch

import kbnet_amd as kb
import run_cases as rc

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 3, 5), (2, 2, 4), (2, 5, 67), (3, 24, 40), (1, 2, 1216)]
AFFINES = [(255.0, 0.0), (127.5, 127.5), (1.0, 0.0)]
SOURCES = ["all", "image", "depth_a", "depth_b"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _host(t):
    return None if t is None else t.cpu().numpy()


def _check(got, image, depth_a, depth_b, scale, shift, what):
    rgb, samples_a, samples_b = (_host(t) for t in got)
    for name, have, src in (("rgb", rgb, image), ("samples_a", samples_a, depth_a), ("samples_b", samples_b, depth_b)):
        assert (have is None) == (src is None), (what, name)
    if image is not None:
        want = rc.oracle_rgb(image, scale, shift)
        assert rgb.dtype == np.uint8 and rgb.shape == want.shape and np.array_equal(rgb, want), (what, "rgb", int((rgb != want).sum()))
    for name, have, src in (("samples_a", samples_a, depth_a), ("samples_b", samples_b, depth_b)):
        if src is not None:
            want = rc.oracle_samples(src)
            assert have.dtype == np.int16 and have.shape == want.shape and np.array_equal(have.view(np.uint16), want), (what, name)


@pytest.mark.parametrize("sources", SOURCES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_export_pack_equals_the_oracle(dev, shape, sources):
    n, h, w = shape
    image, depth_a, depth_b = rc.make_sources(n, h, w, seed=n * 1000 + h * 10 + w)
    if sources != "all":
        image, depth_a, depth_b = (t if name == sources else None for name, t in (("image", image), ("depth_a", depth_a), ("depth_b", depth_b)))
    on_device = [None if t is None else torch.from_numpy(t).to(dev) for t in (image, depth_a, depth_b)]
    for scale, shift in AFFINES if image is not None else AFFINES[:1]:
        got = kb.ops.export_pack(*on_device, scale=scale, shift=shift)
        _check(got, image, depth_a, depth_b, scale, shift, (shape, sources, scale, shift))
        again = kb.ops.export_pack(*on_device, scale=scale, shift=shift)
        for a, b in zip(got, again):
            assert (a is None and b is None) or torch.equal(a, b)      # two runs, equal bytes


def test_planted_values_reach_the_kernel(dev):
    """The (3, 24, 40) case holds every planted value in each source; a 3-d depth is taken as N x H x W."""
    n, h, w = 3, 24, 40
    image, depth_a, depth_b = rc.make_sources(n, h, w, seed=3)
    planted = rc.planted_values()
    for t in (image, depth_a, depth_b):
        assert np.array_equal(t.reshape(-1)[:planted.size].view(np.uint32), planted.view(np.uint32))
    got = kb.ops.export_pack(torch.from_numpy(image).to(dev), torch.from_numpy(depth_a[:, 0]).to(dev), torch.from_numpy(depth_b).to(dev))
    _check(got, image, depth_a, depth_b, 255.0, 0.0, "planted")
    assert np.array_equal(got[1].cpu().numpy().view(np.uint16), kb.loader.depth_samples(torch.from_numpy(depth_a).to(dev)).reshape(n, h, w))
    assert np.array_equal(got[2].cpu().numpy().view(np.uint16), kb.loader.depth_samples(depth_b).reshape(n, h, w))


@pytest.mark.parametrize("shape", [(2, 2, 4), (2, 5, 67), (1, 2, 1216)], ids=lambda s: "x".join(map(str, s)))
def test_sources_four_bytes_past_a_16_byte_boundary(dev, shape):
    """Slices of flat buffers that start one float in: dense, but no 16-byte load may be used (the scalar path)."""
    n, h, w = shape
    image, depth_a, depth_b = rc.make_sources(n, h, w, seed=17)
    shifted = []
    for t in (image, depth_a, depth_b):
        flat = torch.zeros(t.size + 9, device=dev)
        assert flat.data_ptr() % 16 == 0
        view = flat[1:1 + t.size].view(t.shape)
        view.copy_(torch.from_numpy(t))
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        shifted.append(view)
    _check(kb.ops.export_pack(*shifted), image, depth_a, depth_b, 255.0, 0.0, ("misaligned", shape))


@pytest.mark.parametrize("offset", [0, 16, 6], ids=lambda o: f"offset{o}")
@pytest.mark.parametrize("shape", [(1, 3, 5), (2, 2, 4), (2, 5, 67), (3, 24, 40)], ids=lambda s: "x".join(map(str, s)))
def test_outputs_inside_guarded_buffers(dev, shape, offset):
    """`out` views inside larger sentinel-filled buffers (at a 16-byte boundary: the vector stores; off it: the scalar ones): the
    views hold the oracle's bytes, every byte around them is unchanged."""
    n, h, w = shape
    image, depth_a, depth_b = rc.make_sources(n, h, w, seed=23)
    px = n * h * w
    guard = 64
    buffers, views = [], []
    for nbytes, view_shape, dtype in ((3 * px, (n, h, w, 3), torch.uint8), (2 * px, (n, h, w), torch.int16), (2 * px, (n, h, w), torch.int16)):
        flat = torch.full((guard + offset + nbytes + guard,), 0xA5, dtype=torch.uint8, device=dev)
        view = flat[guard + offset:guard + offset + nbytes]
        views.append(view.view(dtype).view(view_shape))
        buffers.append(flat)
    got = kb.ops.export_pack(*(torch.from_numpy(t).to(dev) for t in (image, depth_a, depth_b)), out=tuple(views))
    assert all(g.data_ptr() == v.data_ptr() for g, v in zip(got, views))
    _check(got, image, depth_a, depth_b, 255.0, 0.0, ("guarded", shape, offset))
    for flat, nbytes in zip(buffers, (3 * px, 2 * px, 2 * px)):
        host = flat.cpu().numpy()
        assert np.all(host[:guard + offset] == 0xA5) and np.all(host[guard + offset + nbytes:] == 0xA5)


def test_strided_inputs_are_made_dense(dev):
    n, h, w = 2, 6, 8
    image, depth_a, _ = rc.make_sources(n, h, 2 * w, seed=5)
    got = kb.ops.export_pack(torch.from_numpy(image).to(dev)[..., ::2], torch.from_numpy(depth_a).to(dev)[..., 1::2])
    _check(got, image[..., ::2], depth_a[..., 1::2], None, 255.0, 0.0, "strided")


def test_refusals(dev):
    KbnError = kb._lib.KbnError
    image = torch.zeros(2, 3, 4, 8, device=dev)
    with pytest.raises(KbnError, match="depth_a"):
        kb.ops.export_pack(image, torch.zeros(2, 1, 4, 9, device=dev))
    with pytest.raises(KbnError, match="depth_b"):
        kb.ops.export_pack(image, torch.zeros(2, 1, 4, 8, device=dev), torch.zeros(3, 1, 4, 8, device=dev))
    with pytest.raises(KbnError, match="image"):
        kb.ops.export_pack(torch.zeros(2, 4, 4, 8, device=dev))
    with pytest.raises(KbnError, match="samples_a"):
        kb.ops.export_pack(image, out=(None, torch.zeros(2, 4, 8, dtype=torch.int16, device=dev), None))
    with pytest.raises(KbnError, match="rgb"):
        kb.ops.export_pack(image, out=(torch.zeros(2, 4, 8, 3, dtype=torch.int16, device=dev), None, None))
    with pytest.raises(KbnError, match="image"):
        kb.ops.export_pack(image.cpu())
