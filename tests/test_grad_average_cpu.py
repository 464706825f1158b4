"""No GPU: the pure parts of data-parallel training -- dist.bucket_layout (GradientAverager's buffer), loader.shard_batches and
TrainingFrameLoader's rank / world arguments, the ctypes mirror of kbn_copy_tensor, and the refusals that need no device.

    python -m pytest tests/test_grad_average_cpu.py -q
"""
import ctypes as C
import os
import re

import pytest
import torch

import kbnet_amd as kb

KbnError = kb._lib.KbnError
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bucket_layout():
    numels = [1, 3, 4, 5, 0, 1023, 0, 0, 4097, 8, 2]
    offsets, total = kb.dist.bucket_layout(numels)
    assert len(offsets) == len(numels) and total % 4 == 0
    assert all(o % 4 == 0 for o in offsets)
    assert offsets == sorted(offsets) and offsets[0] == 0
    end = 0
    for o, n in zip(offsets, numels):
        assert o >= end                       # no overlap, in order
        assert o - end <= 3                   # nothing but the padding between two segments
        end = o + n
    assert end <= total <= end + 3
    assert offsets[4] == offsets[5] and offsets[6] == offsets[7] == offsets[8]      # an empty tensor takes no room
    assert kb.dist.bucket_layout([]) == ([], 0) and kb.dist.bucket_layout([0, 0]) == ([0, 0], 0)
    assert kb.dist.bucket_layout([4, 4]) == ([0, 4], 8) and kb.dist.bucket_layout([5, 1]) == ([0, 8], 12)
    with pytest.raises(KbnError):
        kb.dist.bucket_layout([4, -1])


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_shard_batches(world):
    for n_sample, batch_size in ((13, 5), (16, 8), (7, 7), (9, 4), (3, 8), (1, 1)):
        order = [(7 * i + 3) % n_sample for i in range(n_sample)] if n_sample in (13, 9) else list(reversed(range(n_sample)))
        shards = [kb.loader.shard_batches(order, batch_size, rank, world) for rank in range(world)]
        n_batch = -(-n_sample // batch_size)
        assert all(len(s) == n_batch for s in shards)
        for b in range(n_batch):
            whole = order[b * batch_size:(b + 1) * batch_size]
            assert sum((s[b] for s in shards), []) == whole
            for rank in range(world):
                lo, hi = kb.dist.shard_bounds(len(whole), rank, world)
                assert shards[rank][b] == whole[lo:hi]
            assert (len(whole) < world) == any(len(s[b]) == 0 for s in shards)      # an empty shard exactly where n < world


def _loader_stub(n_sample, batch_size, rank=0, world=1):
    """A TrainingFrameLoader's host-side counters without its device side."""
    loader = object.__new__(kb.loader.TrainingFrameLoader)
    loader.n_sample, loader.batch_size, loader.rank, loader.world = n_sample, batch_size, rank, world
    return loader


def test_global_batch_size():
    for n_sample, batch_size in ((13, 5), (16, 8), (3, 8), (1, 1)):
        loader = _loader_stub(n_sample, batch_size, rank=1, world=2)
        sizes = [loader.global_batch_size(b) for b in range(len(loader))]
        assert sum(sizes) == n_sample and all(s == batch_size for s in sizes[:-1]) and 1 <= sizes[-1] <= batch_size
        order = list(range(n_sample))
        for b, size in enumerate(sizes):
            assert size == sum(len(kb.loader.shard_batches(order, batch_size, r, 2)[b]) for r in range(2))
        with pytest.raises(KbnError):
            loader.global_batch_size(len(loader))


@pytest.mark.parametrize("rank, world", [(1, 1), (2, 2), (0, 0), (0, -1), (-1, 2)])
def test_the_loader_refuses_a_rank_outside_its_world(rank, world):
    with pytest.raises(KbnError, match="rank"):
        kb.loader.TrainingFrameLoader(["a.png"], ["b.png"], ["k.npy"], device=torch.device("cuda:0"), rank=rank, world=world)


def test_the_record_mirrors_the_headers_struct():
    with open(os.path.join(ROOT, "include", "kbnet_hip.h")) as f:
        header = f.read()
    body = re.search(r"typedef struct kbn_copy_tensor \{(.*?)\} kbn_copy_tensor;", header, re.S).group(1)
    fields = [line.strip().rstrip(";") for line in body.strip().splitlines()]
    assert fields == ["const float* src", "float* dst", "long long numel"]
    want = 2 * C.sizeof(C.c_void_p) + C.sizeof(C.c_longlong)      # no padding: three 8-byte fields
    assert C.sizeof(kb._lib.CopyTensor) == want == kb.ops._COPY_RECORD.size == 24
    assert [name for name, _ in kb._lib.CopyTensor._fields_] == ["src", "dst", "numel"]
    assert kb._lib.SIGNATURES["kbn_multi_tensor_scale_copy"][1][2] is C.c_float
    assert f"#define KBN_MULTI_COPY_TABLE_CAPACITY {kb.ops.MULTI_COPY_TABLE_CAPACITY}\n" in header
    assert f"#define KBN_MULTI_COPY_PASS_ELEMENTS {kb.ops.MULTI_COPY_PASS_ELEMENTS} " in header
    assert "multi_copy.hip" in kb._build.SOURCES


def test_the_entry_point_checks_every_record_before_it_launches():
    """NULL table, count < 1, numel < 0, a NULL pointer with numel > 0 -- also behind records that are fine: nothing reaches a device."""
    lib = kb._lib.load()
    Rec = kb._lib.CopyTensor
    one = (Rec * 1)(Rec(0, 0, 0))
    assert lib.kbn_multi_tensor_scale_copy(None, 1, 1.0, None) == kb._lib.KBN_ERR_INVALID_ARGUMENT
    for count in (0, -1):
        assert lib.kbn_multi_tensor_scale_copy(one, count, 1.0, None) == kb._lib.KBN_ERR_INVALID_ARGUMENT
    for bad in (Rec(16, 32, -1), Rec(0, 32, 4), Rec(16, 0, 4)):
        table = (Rec * 3)(Rec(0, 0, 0), Rec(0, 0, 0), bad)
        assert lib.kbn_multi_tensor_scale_copy(table, 3, 1.0, None) == kb._lib.KBN_ERR_INVALID_ARGUMENT


def test_the_averager_refuses_cpu_parameters_and_bad_ranks():
    params = [torch.nn.Parameter(torch.zeros(3, 3)), torch.nn.Parameter(torch.zeros(5))]
    with pytest.raises(KbnError, match="CUDA/HIP"):
        kb.dist.GradientAverager(params, 0, 1)
    with pytest.raises(KbnError, match="conv.weight"):
        kb.dist.GradientAverager([("conv.weight", params[0])], 0, 1)
    with pytest.raises(KbnError, match="no parameters"):
        kb.dist.GradientAverager([], 0, 1)
    for rank, world in ((1, 1), (0, 0), (-1, 2)):
        with pytest.raises(KbnError, match="rank"):
            kb.dist.GradientAverager(params, rank, world)
    with pytest.raises(KbnError, match="not a tensor"):
        kb.dist.GradientAverager([3.0], 0, 1)
