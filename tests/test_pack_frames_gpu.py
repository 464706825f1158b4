"""GPU: the device ENCODER of the packed frame store, ops.pack_frames / kbn_pack_frames_forward.  What it writes is
compared BYTE FOR BYTE with the host encoder (loader.encode_frame) and with the NumPy statement of the format
(tests/frame_pack_oracle.py) -- not only round-tripped: tests/test_pack_outputs_cpu.py shows encoders that round-trip and are wrong.

Every call here goes through `pack`, which hands the encoder a view into a sentinel-filled buffer with a stride above the minimum
and asserts, besides the bytes: nothing past out_bytes[i] in a slot and nothing in the guards before the first and after the last
slot changed; a second run gives the same bytes; every file passes check_frame and decode_frame returns the samples."""

import numpy as np
import pytest
import torch

import frame_pack_oracle as oracle
import kbnet_amd as kb
import pack_cases as pc

pytestmark = pytest.mark.gpu
KbnError = kb._lib.KbnError
SENTINEL, GUARD, SLACK = 0xA5, 64, 48


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need a visible MI355X (run with -m gpu on a GPU box)")
    kb._lib.load()
    return torch.device("cuda:0")


def to_device(samples, dev, misalign=False):
    """N x H x W x C uint8 / uint16 -> the device tensor ops.pack_frames takes (uint16 as int16 bit patterns); with `misalign` its
    first sample lies one sample (1 byte for 8 bits, 2 for 16) past a 16-byte boundary."""
    a = np.ascontiguousarray(samples)
    flat = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).reshape(-1)
    room = torch.zeros(flat.numel() + 16, dtype=flat.dtype, device=dev)
    assert room.data_ptr() % 16 == 0
    view = room[1:1 + flat.numel()] if misalign else room[:flat.numel()]
    view.copy_(flat)
    t = view.view(a.shape[:-1] if a.ndim == 4 and a.shape[-1] == 1 else a.shape)      # one channel: N x H x W
    assert t.data_ptr() % 16 == (a.dtype.itemsize if misalign else 0)
    return t


def pack(samples, dev, misalign=False, oracle_too=True):
    """samples: N x H x W x C numpy.  Runs the encoder as the module docstring says and returns the files' bytes."""
    n, h, w, c = samples.shape
    bits = 8 * samples.dtype.itemsize
    t = to_device(samples, dev, misalign)
    stride = kb.ops.pack_frames_stride(h, w, c, bits) + SLACK
    runs = []
    for _ in range(2):
        buf = torch.full((2 * GUARD + n * stride,), SENTINEL, dtype=torch.uint8, device=dev)
        out = buf[GUARD:GUARD + n * stride].view(n, stride)
        sizes = torch.full((n,), -1, dtype=torch.int64, device=dev)
        got_out, got_sizes = kb.ops.pack_frames(t, out=out, out_bytes=sizes)
        assert got_out is out and got_sizes is sizes
        runs.append((buf.cpu().numpy(), sizes.cpu().numpy()))
    (host, size), (host2, size2) = runs
    assert np.array_equal(size, size2) and np.array_equal(host, host2), "two runs gave different bytes"
    assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + n * stride:] == SENTINEL).all(), "a guard was written"
    files = []
    for i in range(n):
        slot = host[GUARD + i * stride:GUARD + (i + 1) * stride]
        assert 0 < size[i] <= stride - SLACK
        assert (slot[size[i]:] == SENTINEL).all(), f"frame {i}: bytes past out_bytes were written"
        data = slot[:size[i]].tobytes()
        frame = samples[i] if c > 1 else samples[i, :, :, 0]
        want = kb.loader.encode_frame(frame)
        assert len(data) == len(want), f"frame {i} of {samples.shape}: {len(data)} bytes, the host encoder writes {len(want)}"
        assert data == want, f"frame {i} of {samples.shape} differs from the host encoder at byte {first_difference(data, want)}"
        if oracle_too:
            assert data == oracle.encode(frame), f"frame {i} of {samples.shape} differs from the NumPy oracle"
        kb.loader.check_frame(data)
        assert np.array_equal(kb.loader.decode_frame(data), frame)
        files.append(data)
    return files


def first_difference(a, b):
    return next(i for i, (x, y) in enumerate(zip(a, b)) if x != y)


WIDTHS = (1, 2, 15, 16, 17, 31, 33, 129, 241)


@pytest.mark.parametrize("h", [1, 7, 8, 9, 17])
@pytest.mark.parametrize("c,bits", [(1, 8), (3, 8), (4, 8), (1, 16), (3, 16), (4, 16)])
def test_shapes_and_contents(dev, c, bits, h):
    """Short last segments, short last groups, one-sample left rows, one-row groups -- each width with the five contents as the five
    frames of one call."""
    for w in WIDTHS:
        pack(pc.batch(pc.CONTENTS, h, w, c, bits, seed=w), dev)


@pytest.mark.parametrize("c,bits", [(1, 8), (3, 16)])
def test_ramp_forces_every_b(dev, c, bits):
    """The ramp content really asks for every b from 0 to bits (read back from the encoder's own header bytes)."""
    files = pack(pc.batch(("ramp",), 17, 241, c, bits), dev)
    assert set(pc.header_bytes(files[0])) == set(range(bits + 1))


@pytest.mark.parametrize("n", [1, 3, 70])
@pytest.mark.parametrize("c,bits", [(3, 8), (1, 16)])
def test_batch_sizes(dev, c, bits, n):
    """n frames in one call, each with content of its own: sizes and table offsets differ from frame to frame."""
    contents = [pc.CONTENTS[i % len(pc.CONTENTS)] for i in range(n)]
    files = pack(pc.batch(contents, 9, 33, c, bits, seed=n), dev)
    assert len({len(f) for f in files}) >= min(n, 3)


def test_payloads_start_at_every_residue(dev):
    """(group, plane) payloads are only byte-aligned: these frames' payloads start at every residue mod 4 (and mod 16 between
    them), so the ragged head and tail of the emit pass's stores are all run."""
    samples = pc.batch(("noise", "sparse", "ramp"), 41, 31, 3, 8, seed=3)
    files = pack(samples, dev)
    starts = [pc.table(f)[0] + at for f in files for at in pc.table(f)[1][:-1]]
    assert {s % 4 for s in starts} == {0, 1, 2, 3}
    assert len({s % 16 for s in starts}) >= 12


@pytest.mark.parametrize("c,bits", [(3, 8), (1, 16), (1, 8), (4, 16)])
def test_misaligned_samples(dev, c, bits):
    """The samples pointer one sample past a 16-byte boundary (asserted in to_device)."""
    pack(pc.batch(("noise", "sparse", "wrap"), 17, 33, c, bits, seed=9), dev, misalign=True)


def test_shapes_ops_accepts(dev):
    """N x H x W uint8 / int16 are one-channel frames; bits may be stated; allocated outputs equal given ones."""
    a = pc.batch(("noise", "sparse"), 9, 17, 1, 16)
    t = to_device(a, dev)
    assert t.dim() == 3
    out, sizes = kb.ops.pack_frames(t, bits=16)
    assert out.shape == (2, kb.ops.pack_frames_stride(9, 17, 1, 16)) and sizes.dtype == torch.int64
    for i in range(2):
        assert out[i, :int(sizes[i])].cpu().numpy().tobytes() == kb.loader.encode_frame(a[i, :, :, 0])
    out4, sizes4 = kb.ops.pack_frames(t.unsqueeze(-1))
    assert torch.equal(sizes4, sizes)
    with pytest.raises(KbnError, match="bits"):
        kb.ops.pack_frames(t, bits=8)


def test_output_size_frames(dev):
    """The multi-chunk path of a real output, once: 352 x 1216 x 3 of 8 bits and 352 x 1216 of 16 bits, batch 2 (a smooth picture
    with noise; a dense depth map and a sparse one).  Against the host encoder; the NumPy oracle takes seconds at this size and has
    compared every path above."""
    h, w = 352, 1216
    rng = np.random.default_rng(22)
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    smooth = (96 + 64 * np.sin(x / 37.0) * np.cos(y / 23.0))[None, :, :, None] + rng.integers(-6, 7, size=(2, h, w, 3))
    pack(np.clip(smooth, 0, 255).astype(np.uint8), dev, oracle_too=False)
    dense = (2000 + 40 * y + 3 * x + rng.integers(0, 50, size=(h, w))).astype(np.uint16)
    sparse = np.where(rng.random((h, w)) < 0.05, dense, 0).astype(np.uint16)
    pack(np.stack([dense, sparse])[:, :, :, None], dev, oracle_too=False)


def test_widest_row(dev):
    """W = KBN_PACK_FRAMES_MAX_WIDTH: the largest dynamic-LDS launch (an offset for each of 8 x 1024 segments), header bytes a
    full LDS image long, 32 chunks a (group, plane).  Eight rows against the host encoder; one row against the NumPy oracle
    as well, which takes a second and more for eight rows of this width."""
    cap = kb._lib.KBN_PACK_FRAMES_MAX_WIDTH
    pack(pc.batch(("noise", "sparse"), 8, cap, 1, 16, seed=4), dev, oracle_too=False)
    pack(pc.batch(("ramp",), 8, cap, 3, 8, seed=5), dev, oracle_too=False)
    pack(pc.batch(("noise",), 1, cap, 1, 16, seed=6), dev)


def test_refusals_before_any_launch(dev):
    """Argument checks run before anything is launched: the outputs keep their bytes."""
    lib = kb._lib.load()
    cap = kb._lib.KBN_PACK_FRAMES_MAX_WIDTH
    assert cap >= 4096
    with pytest.raises(KbnError, match="cannot be packed"):
        kb.ops.pack_frames(torch.zeros((1, 1, cap + 1), dtype=torch.uint8, device=dev))
    t = to_device(pc.batch(("noise",), 9, 33, 1, 8), dev)
    stride = kb.ops.pack_frames_stride(9, 33, 1, 8)
    with pytest.raises(KbnError, match="out is"):
        kb.ops.pack_frames(t, out=torch.zeros((1, stride - 16), dtype=torch.uint8, device=dev))
    with pytest.raises(KbnError, match="out is"):
        kb.ops.pack_frames(t, out=torch.zeros((1, stride + 8), dtype=torch.uint8, device=dev))
    with pytest.raises(KbnError, match="workspace"):
        kb.ops.pack_frames(t, workspace=torch.zeros((8,), dtype=torch.uint8, device=dev))
    with pytest.raises(KbnError, match="samples"):
        kb.ops.pack_frames(t.cpu())
    # the entry point itself, with real device pointers: status codes, and nothing written
    out = torch.full((stride + 16,), SENTINEL, dtype=torch.uint8, device=dev)
    sizes = torch.full((1,), -1, dtype=torch.int64, device=dev)
    need = lib.kbn_pack_frames_workspace_bytes(1, 33, 9, 1, 8)
    work = torch.zeros((need,), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def forward(width=33, out_ptr=out.data_ptr(), out_stride=stride, work_bytes=need, channels=1, bits=8):
        return lib.kbn_pack_frames_forward(t.data_ptr(), 1, width, 9, channels, bits, out_ptr, out_stride, sizes.data_ptr(),
                                           work.data_ptr(), work_bytes, stream)

    assert forward(width=cap + 1) == kb._lib.KBN_ERR_UNSUPPORTED
    assert forward(channels=2) == kb._lib.KBN_ERR_UNSUPPORTED and forward(bits=12) == kb._lib.KBN_ERR_UNSUPPORTED
    assert forward(out_stride=stride - 16) == kb._lib.KBN_ERR_INVALID_ARGUMENT
    assert forward(out_stride=stride + 8) == kb._lib.KBN_ERR_INVALID_ARGUMENT
    assert forward(out_ptr=out.data_ptr() + 4) == kb._lib.KBN_ERR_INVALID_ARGUMENT
    assert forward(work_bytes=need - 1) == kb._lib.KBN_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all() and int(sizes[0]) == -1
