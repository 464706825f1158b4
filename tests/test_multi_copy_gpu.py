"""GPU: ops.multi_tensor_scale_copy (csrc/multi_copy.hip), the pack pass of kb.dist.GradientAverager, bit for bit against
src * float32(scale) as torch computes it on the host.

One list of 100 tensors (more than two table capacities: three launches): numels 1, 3, 4, 5, 1023, 4097 and one pass of the widest
grid + 5 (a tensor that loops and has a tail), repeated, and once four passes + 5 (the vector loop's second round).  Every destination is a slice of one guard-filled buffer; every third pair
sits one element off a 16-byte boundary on the source side, every fifth on the destination side (the scalar path).

    python -m pytest tests/test_multi_copy_gpu.py -m gpu -q
"""
import numpy as np
import pytest
import torch

import kbnet_amd as kb

KbnError = kb._lib.KbnError
pytestmark = pytest.mark.gpu
CAP, PASS = kb.ops.MULTI_COPY_TABLE_CAPACITY, kb.ops.MULTI_COPY_PASS_ELEMENTS
NUMELS = [1, 3, 4, 5, 1023, 4097, PASS + 5]
COUNT = 100
LONGEST = 20
GUARD = -12345.0
SCALES = [1.0, 0.5, float(np.float32(3 / 5))]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need a visible MI355X (run with -m gpu on a GPU box)")
    kb._lib.load()   # a missing extension is an error on a GPU box, never a skip
    return torch.device("cuda:0")


def _sizes():
    # the looping tensor only four times: the list stays at 17 MB
    sizes = [NUMELS[i % len(NUMELS)] for i in range(COUNT)]
    sizes = [n if n <= PASS or i < 4 * len(NUMELS) else 4097 for i, n in enumerate(sizes)]
    sizes[LONGEST] = 4 * PASS + 5      # an aligned pair: the vector loop takes four passes at a time, this one comes round a second time
    return sizes


_SHARED = {}


def _sources(dev):
    """The list's sources on the device (computed once, never written), with a NaN, a +Inf and a -Inf in chosen elements."""
    if not _SHARED:
        gen = torch.Generator().manual_seed(7)
        sizes = _sizes()
        host = [torch.randn(n, generator=gen, dtype=torch.float32) for n in sizes]
        host[4][17], host[4][18], host[5][4096] = float("nan"), float("inf"), float("-inf")      # vector body; the tail element
        host[6][PASS + 4], host[2][3] = float("nan"), float("inf")                                # the looping tensor's tail
        srcs = []
        for i, h in enumerate(host):
            if i % 3 == 1:      # one element off: 4 bytes past a 16-byte boundary
                store = torch.empty(h.numel() + 1, dtype=torch.float32, device=dev)
                store[1:].copy_(h)
                srcs.append(store[1:])
            else:
                srcs.append(h.to(dev))
        _SHARED.update(sizes=sizes, host=host, srcs=srcs)
    return _SHARED["sizes"], _SHARED["host"], _SHARED["srcs"]


def _destinations(dev, sizes):
    """Slices of one guard-filled buffer: segments four-element aligned with four guard elements between them, every fifth moved
    on by one element."""
    offsets, at = [], 4
    for i, n in enumerate(sizes):
        offsets.append(at + (1 if i % 5 == 2 else 0))
        at += ((n + 1 + 3) & ~3) + 4
    buf = torch.full((at,), GUARD, dtype=torch.float32, device=dev)
    return buf, offsets, [buf[o:o + n] for o, n in zip(offsets, sizes)]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def test_the_list_has_every_path(dev):
    sizes, _, srcs = _sources(dev)
    _, _, dsts = _destinations(dev, sizes)
    assert len(sizes) == COUNT > 2 * CAP and sorted(set(sizes)) == sorted(NUMELS + [4 * PASS + 5])
    aligned = [s.data_ptr() % 16 == 0 and d.data_ptr() % 16 == 0 for s, d in zip(srcs, dsts)]
    assert aligned[LONGEST]
    assert any(aligned) and not all(aligned)
    assert any(s.data_ptr() % 16 == 4 for s in srcs) and any(d.data_ptr() % 16 == 4 for d in dsts)
    assert any(a and n > PASS for a, n in zip(aligned, sizes)) and any(not a and n > PASS for a, n in zip(aligned, sizes))


@pytest.mark.parametrize("scale", SCALES, ids=["1", "0.5", "3/5"])
def test_bits_guards_and_non_finite_elements(dev, scale):
    sizes, host, srcs = _sources(dev)
    buf, offsets, dsts = _destinations(dev, sizes)
    kb.ops.multi_tensor_scale_copy(srcs, dsts, scale)
    factor = torch.tensor(scale, dtype=torch.float32)
    got = buf.cpu()
    covered = torch.zeros(got.numel(), dtype=torch.bool)
    for i, (h, o, n) in enumerate(zip(host, offsets, sizes)):
        want = h * factor
        assert torch.equal(_bits(got[o:o + n]), _bits(want)), (i, n)
        if scale == 1.0:
            assert torch.equal(_bits(got[o:o + n]), _bits(h)), (i, n)
        covered[o:o + n] = True
        bad = ~torch.isfinite(h)
        assert torch.equal(~torch.isfinite(got[o:o + n]), bad), (i, n)      # a NaN or Inf stays in its own element
    assert bool((got[~covered] == GUARD).all()), "a guard element was written"
    assert int((~covered).sum()) >= 4 * (COUNT + 1)
    assert torch.isnan(got[offsets[4] + 17]) and got[offsets[4] + 18] == float("inf") and got[offsets[5] + 4096] == float("-inf")
    assert torch.isnan(got[offsets[6] + PASS + 4]) and got[offsets[2] + 3] == float("inf")


def test_profile_counts_the_launches_and_their_bytes(dev):
    sizes, _, srcs = _sources(dev)
    _, _, dsts = _destinations(dev, sizes)
    kb.ops.PROFILE = []
    try:
        kb.ops.multi_tensor_scale_copy(srcs + [torch.empty(0, device=dev)], dsts + [torch.empty(0, device=dev)], 0.5)
        records = [r for r in kb.ops.PROFILE if r[0] == "multi_tensor_scale_copy"]
        others = len(kb.ops.PROFILE) - len(records)
    finally:
        kb.ops.PROFILE = None
    torch.cuda.synchronize()
    assert others == 0 and len(records) == -(-COUNT // CAP) == 3
    assert [r[4] for r in records] == [8.0 * sum(sizes[lo:lo + CAP]) for lo in range(0, COUNT, CAP)]


def test_a_non_dense_source_is_copied_and_a_non_dense_destination_refused(dev):
    x = torch.randn(2, 6, 5, 7, generator=torch.Generator().manual_seed(3)).to(dev)
    src = x[:, 1:4]                                    # a channel slice
    assert not src.is_contiguous()
    dst = torch.full((2 * 3 * 5 * 7 + 8,), GUARD, device=dev)
    kb.ops.multi_tensor_scale_copy([src], [dst[4:-4]], 0.5)
    assert torch.equal(_bits(dst[4:-4]), _bits((x.cpu()[:, 1:4] * torch.tensor(0.5)).reshape(-1)))
    assert bool((dst[:4] == GUARD).all()) and bool((dst[-4:] == GUARD).all())
    with pytest.raises(KbnError, match="dense"):
        kb.ops.multi_tensor_scale_copy([src.contiguous()], [torch.empty_like(x)[:, 1:4]], 1.0)
    with pytest.raises(KbnError, match="elements"):
        kb.ops.multi_tensor_scale_copy([x], [dst], 1.0)
    with pytest.raises(KbnError, match="float32"):
        kb.ops.multi_tensor_scale_copy([x.double()], [torch.empty_like(x)], 1.0)
    with pytest.raises(KbnError, match="1 sources and 2 destinations"):
        kb.ops.multi_tensor_scale_copy([x], [torch.empty_like(x), torch.empty_like(x)], 1.0)


def test_cpu_tensors_are_refused(dev):
    a, b = torch.zeros(4), torch.zeros(4, device=dev)
    for srcs, dsts in (([a], [b]), ([b], [a]), ([a], [a])):
        with pytest.raises(KbnError, match="CUDA/HIP"):
            kb.ops.multi_tensor_scale_copy(srcs, dsts)


def test_writing_a_parameter_bumps_its_version(dev):
    p = torch.nn.Parameter(torch.zeros(3, 5, device=dev))
    q = torch.zeros(3, 5, device=dev, requires_grad=True)
    plain = torch.zeros(15, device=dev)
    src = torch.arange(15, dtype=torch.float32, device=dev)
    before = p._version, q._version, plain._version
    kb.ops.multi_tensor_scale_copy([src, src, src], [p, q, plain], 2.0)
    assert p._version == before[0] + 1 and q._version == before[1] + 1 and plain._version == before[2]
    for t in (p, q, plain):
        assert torch.equal(t.detach().reshape(-1), 2.0 * src)
    frozen = torch.nn.Parameter(torch.zeros(15, device=dev), requires_grad=False)
    v = frozen._version
    kb.ops.multi_tensor_scale_copy([src], [frozen])
    assert frozen._version == v + 1 and torch.equal(frozen.detach(), src)
