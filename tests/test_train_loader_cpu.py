"""CPU: the host side of the training loader (loader.draw_crop / random_crop / TrainingFrameLoader's refusals) and the argument
checks of kbn_unpack_train_frames_forward, against what the REFERENCE's KBNetTrainingDataset returned from the same files
(tests/golden/train_io/*, tests/golden/train_loader.npz; written by tests/golden/gen_train_loader_golden.py)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import kbnet_amd as kb
from conftest import GOLDEN_DIR, ROOT

KbnError = kb._lib.KbnError
IO = os.path.join(GOLDEN_DIR, "train_io")
GOLDEN = np.load(os.path.join(GOLDEN_DIR, "train_loader.npz"))
RUNS = json.loads(bytes(GOLDEN["runs"]).decode())
IMAGES = [os.path.join(IO, f"triplet_{i}.png") for i in range(4)]
DEPTHS = [os.path.join(IO, f"depth_{i}.png") for i in range(4)]
KS = [os.path.join(IO, f"k_{i}.npy") for i in range(4)]
SIZES = [(24, 40), (26, 44), (25, 43), (24, 40)]
CROPPED = [r for r in RUNS if r["shape"] is not None]
ids = lambda runs: ["{}-{}x{}".format("+".join(r["crop_type"]), *(r["shape"] or (0, 0))) for r in runs]


def test_the_golden_covers_what_it_claims():
    assert len(CROPPED) == 16 and len({(tuple(r["crop_type"]), tuple(r["shape"])) for r in CROPPED}) == 16
    assert any(x % 2 for r in CROPPED for _, x in r["starts"])
    for r in CROPPED:
        assert GOLDEN[r["name"] + "::k"].shape == (12, 3, 3) and GOLDEN[r["name"] + "::image0"].shape == (4, 3, *r["shape"])
        if "horizontal" in r["crop_type"]:
            assert len({x for _, x in r["starts"]}) >= 2
        if "vertical" in r["crop_type"] and "bottom" not in r["crop_type"]:
            centred = [y == (SIZES[j % 4][0] - r["shape"][0]) // 2 for j, (y, _) in enumerate(r["starts"])]
            assert any(centred) and not all(centred)


@pytest.mark.parametrize("run", CROPPED, ids=ids(CROPPED))
def test_draw_crop_reproduces_the_reference_offsets(run):
    """All twelve draws in order under the run's seed: the offsets the golden intrinsics imply."""
    ks = [np.load(p).astype(np.float32) for p in KS]
    golden_k = GOLDEN[run["name"] + "::k"]
    np.random.seed(run["np_seed"])
    for j in range(12):
        h, w = SIZES[j % 4]
        y, x = kb.loader.draw_crop(h, w, run["shape"], run["crop_type"])
        assert isinstance(y, int) and isinstance(x, int)
        want = (float(ks[j % 4][1, 2]) - float(golden_k[j][1, 2]), float(ks[j % 4][0, 2]) - float(golden_k[j][0, 2]))
        assert (y, x) == want == tuple(run["starts"][j]), (j, y, x, want)
        assert 0 <= y <= h - run["shape"][0] and 0 <= x <= w - run["shape"][1]


@pytest.mark.parametrize("run", RUNS, ids=ids(RUNS))
def test_random_crop_over_the_loaders_equals_the_reference_bit_for_bit(run):
    """The reference's __getitem__ (src/datasets.py:199-225) written with the package's functions, all three passes."""
    indices = run.get("indices", [0, 1, 2, 3])
    g = lambda key: GOLDEN[run["name"] + "::" + key]
    np.random.seed(run["np_seed"])
    for j in range(len(g("k"))):
        i = indices[j % len(indices)]
        image1, image0, image2 = kb.loader.load_image_triplet(IMAGES[i], normalize=False)
        depth = kb.loader.load_depth(DEPTHS[i], data_format="CHW")
        k = np.load(KS[i]).astype(np.float32)
        if run["shape"] is not None:
            [image0, image1, image2, depth], k = kb.loader.random_crop([image0, image1, image2, depth], run["shape"], intrinsics=k,
                                                                      crop_type=run["crop_type"])
            assert k.dtype == np.float64      # NumPy's evaluation of float32 + list; the caller casts
        k = k.astype(np.float32)
        assert np.array_equal(k.view(np.uint32), g("k")[j].view(np.uint32)), j
        if j < len(indices):
            for got, key in ((image0, "image0"), (image1, "image1"), (image2, "image2")):
                assert got.dtype == np.float32 and np.array_equal(got, g(key)[j].astype(np.float32)), (j, key)
            assert depth.dtype == np.float32 and np.array_equal(depth.view(np.uint32), g("depth")[j].view(np.uint32)), j


def test_random_crop_without_intrinsics_and_the_negative_zero():
    a = np.arange(2 * 6 * 8, dtype=np.float32).reshape(2, 6, 8)
    [out] = kb.loader.random_crop([a], (4, 4))
    assert np.array_equal(out, a[:, 1:5, 2:6])
    k = np.array([[1.0, -0.0, 3.0], [-0.0, 2.0, 4.0], [-0.0, -0.0, 1.0]], dtype=np.float32)
    _, moved = kb.loader.random_crop([a], (4, 4), intrinsics=k)
    assert not np.signbit(moved).any() and moved[0, 2] == 1.0 and moved[1, 2] == 3.0     # 0.0 was added to the other seven entries


def test_draw_crop_refusals():
    with pytest.raises(KbnError, match="17 x 24.*16 x 40"):
        kb.loader.draw_crop(16, 40, (17, 24), ["horizontal"])
    with pytest.raises(KbnError, match="16 x 41.*16 x 40"):
        kb.loader.draw_crop(16, 40, (16, 41))
    with pytest.raises(ValueError):         # NumPy's own: randint(0, 0), the unanchored crop at the raw size, as in the reference
        kb.loader.draw_crop(16, 40, (8, 40), ["horizontal"])
    assert kb.loader.draw_crop(16, 40, (16, 40)) == (0, 0)                                 # the centre crop at the raw size is fine
    assert kb.loader.draw_crop(16, 40, (16, 40), ["horizontal", "anchored", "bottom"]) == (0, 0)
    assert kb.loader.draw_crop(17, 41, (8, 20), ["bottom"]) == (9, 10)


# ------------------------------------------------------------------------------------------------- the binding and the entry point
def test_binding_matches_the_header():
    header = open(os.path.join(ROOT, "include", "kbnet_hip.h")).read()
    assert int(re.search(r"#define KBN_UNPACK_TRAIN_MAX_FRAMES (\d+)", header).group(1)) == kb._lib.KBN_UNPACK_TRAIN_MAX_FRAMES
    struct = re.search(r"typedef struct kbn_train_frame \{(.*?)\} kbn_train_frame;", header, flags=re.S).group(1)
    struct = re.sub(r"/\*.*?\*/", "", struct, flags=re.S)
    sizes = {"long long": 8, "int": 4}
    fields = [(m.group(1), [n.strip() for n in m.group(2).split(",")]) for m in re.finditer(r"(long long|int)\s+([^;]+);", struct)]
    assert [n for _, names in fields for n in names] == [n for n, _ in kb._lib.TrainFrame._fields_]
    assert sum(sizes[t] * len(names) for t, names in fields) == C.sizeof(kb._lib.TrainFrame) == kb.ops._TRAIN_FRAME_RECORD.size == 32
    assert C.sizeof(kb._lib.TrainFrame) * kb._lib.KBN_UNPACK_TRAIN_MAX_FRAMES + 256 < 4096     # the argument block stays under 4 KB


def _call(frames, n=None, h=16, w=24, channels=3, bits=16, image_bytes=1 << 20, depth_bytes=1 << 20, null=None):
    """The entry point on host memory standing in for the device buffers: every check comes before a launch, so a refusal never
    touches them (and no test here passes arguments that would be accepted)."""
    lib = kb._lib.load()
    dummy = (C.c_ubyte * 64)()
    ptr = C.cast(dummy, C.c_void_p)
    table = (kb._lib.TrainFrame * max(1, len(frames)))()
    for slot, f in zip(table, frames):
        slot.image_offset, slot.depth_offset, slot.height, slot.raw_width, slot.y_start, slot.x_start = f
    ptrs = {name: ptr for name in ("images", "depths", "image0", "image1", "image2", "depth")}
    if null:
        ptrs[null] = None
    return lib.kbn_unpack_train_frames_forward(ptrs["images"], image_bytes, ptrs["depths"], depth_bytes, None if null == "frames" else table,
                                               len(frames) if n is None else n, h, w, channels, bits, ptrs["image0"], ptrs["image1"],
                                               ptrs["image2"], ptrs["depth"], None)


def test_entry_point_refuses_bad_arguments_before_any_launch():
    bad, unsupported = kb._lib.KBN_ERR_INVALID_ARGUMENT, kb._lib.KBN_ERR_UNSUPPORTED
    H, W, h, w = 24, 40, 16, 24
    good = (0, 0, H, 3 * W, H - h, W - w)          # the last crop that fits
    # one pixel past each of the four sides
    assert _call([(0, 0, H, 3 * W, -1, 0)]) == bad
    assert _call([(0, 0, H, 3 * W, H - h + 1, 0)]) == bad
    assert _call([(0, 0, H, 3 * W, 0, -1)]) == bad
    assert _call([(0, 0, H, 3 * W, 0, W - w + 1)]) == bad
    assert _call([good, (0, 0, H, 3 * W, 0, W - w + 1)]) == bad, "the second record is checked too"
    assert _call([(0, 0, H, 3 * W + 1, 0, 0)]) == bad, "a raw width of 3 W + 1"
    assert _call([good], n=0) == bad and _call([good], n=-1) == bad
    assert _call([good], h=0) == bad and _call([good], w=0) == bad
    for name in ("images", "depths", "frames", "image0", "image1", "image2", "depth"):
        assert _call([good], null=name) == bad, name
    assert _call([good], channels=2) == unsupported and _call([good], bits=12) == unsupported
    # a frame that does not lie inside its packed buffer, a negative offset, an odd offset of 16-bit samples
    assert _call([good], image_bytes=H * 3 * W * 3 - 1) == bad and _call([good], depth_bytes=H * W * 2 - 1) == bad
    assert _call([(-16, 0, H, 3 * W, 0, 0)]) == bad and _call([(0, -2, H, 3 * W, 0, 0)]) == bad and _call([(0, 1, H, 3 * W, 0, 0)]) == bad
    assert _call([(0, 0, 0, 3 * W, 0, 0)]) == bad and _call([(0, 0, H, 0, 0, 0)], w=1) == bad


def test_ops_names_the_offending_frame():
    images, depths = torch.zeros(2 * 24 * 120 * 3, dtype=torch.uint8), torch.zeros(2 * 24 * 40 * 2, dtype=torch.uint8)
    ok = (0, 0, 24, 40, 8, 16)
    second = (24 * 120 * 3, 24 * 40 * 2, 24, 40, 8, 16)
    with pytest.raises(KbnError, match=r"frame 1: the 16 x 24 crop at \(9, 16\) leaves the 24 x 40 frame"):
        kb.ops.unpack_train_frames(images, depths, [ok, second[:4] + (9, 16)], (16, 24))
    with pytest.raises(KbnError, match=r"frame 0: the 16 x 24 crop at \(0, -1\)"):
        kb.ops.unpack_train_frames(images, depths, [(0, 0, 24, 40, 0, -1)], (16, 24))
    with pytest.raises(KbnError, match="frame 1: .*leaves the image buffer"):
        kb.ops.unpack_train_frames(images, depths, [ok, (second[0] + 1,) + second[1:]], (16, 24))
    with pytest.raises(KbnError, match="frame 1: .*misaligned or leaves the depth buffer"):
        kb.ops.unpack_train_frames(images, depths, [ok, (second[0], second[1] + 1) + second[2:]], (16, 24))
    with pytest.raises(KbnError, match="channels"):
        kb.ops.unpack_train_frames(images, depths, [ok], (16, 24), channels=2)
    with pytest.raises(KbnError, match="8 or 16 bits"):
        kb.ops.unpack_train_frames(images, depths, [ok], (16, 24), depth_bits=12)
    with pytest.raises(KbnError, match="crop shape"):
        kb.ops.unpack_train_frames(images, depths, [ok], (0, 24))
    with pytest.raises(KbnError, match="no frames"):
        kb.ops.unpack_train_frames(images, depths, [], (16, 24))
    with pytest.raises(KbnError, match="no CPU fallback"):       # everything else is right: CPU tensors are refused, as everywhere
        kb.ops.unpack_train_frames(images, depths, [ok, second], (16, 24))


def test_loader_refusals_without_a_gpu():
    with pytest.raises(KbnError, match="no CPU fallback"):
        kb.loader.TrainingFrameLoader(IMAGES, DEPTHS, KS, shape=(16, 24), device="cpu")
    with pytest.raises(KbnError, match="no CPU fallback"):
        kb.loader.TrainingFrameLoader(IMAGES, DEPTHS, KS, shape=(16, 24))
    with pytest.raises(KbnError, match="4 image, 3 sparse depth and 4 intrinsics"):
        kb.loader.TrainingFrameLoader(IMAGES, DEPTHS[:3], KS, device="cuda:0")
    with pytest.raises(KbnError, match="4 image, 4 sparse depth and 2 intrinsics"):
        kb.loader.TrainingFrameLoader(IMAGES, DEPTHS, KS[:2], device="cuda:0")
