"""CPU: the host side of kb.inference.run -- the 8-bit RGB PNG encoder, the reference's data_utils names, the six settings-log
functions against the reference's recorded text, the refusals, and the power of the export oracle the GPU tests compare with
(tests/test_export_pack_gpu.py, tests/test_run_gpu.py).  No GPU needed.

    python -m pytest tests/test_run_cpu.py -q
"""
import ctypes as C
import io
import os

import numpy as np
import pytest
import torch

import kbnet_amd as kb
import run_cases as rc

KbnError = kb._lib.KbnError


@pytest.fixture(scope="module")
def golden():
    return np.load(rc.GOLDEN)


# ------------------------------------------------------------------------------------------------ the RGB encoder
@pytest.mark.parametrize("level", [-1, 0, 9])
@pytest.mark.parametrize("size", [(1, 1), (5, 3), (40, 24)])
def test_rgb_encoder_round_trip(size, level):
    """width x height: the file decodes to the input pixels with the native reader and with PIL."""
    from PIL import Image
    w, h = size
    px = np.random.default_rng(w * 31 + h).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    px.reshape(-1)[:3] = (0, 255, 128)
    data = kb.loader.encode_image_png(px, level=level)
    assert kb.loader.png_info(data) == (w, h, 3, 8)
    assert np.array_equal(kb.loader.decode_png(data), px)
    with Image.open(io.BytesIO(data)) as im:
        assert im.mode == "RGB" and np.array_equal(np.array(im), px)


def test_rgb_encoder_refuses_a_short_buffer_and_bad_arguments():
    lib = kb._lib.load()
    w, h = 40, 24
    px = np.zeros((h, w, 3), dtype=np.uint8)
    cap = lib.kbn_png_encode_rgb8_bound(w, h)
    assert cap > h * (1 + 3 * w)
    n = C.c_size_t()
    ptr = px.ctypes.data_as(C.c_void_p)
    short = (C.c_ubyte * (cap - 1))()
    assert lib.kbn_png_encode_rgb8(ptr, w, h, short, cap - 1, C.byref(n), 6) == kb._lib.KBN_ERR_WORKSPACE
    exact = (C.c_ubyte * cap)()
    assert lib.kbn_png_encode_rgb8(ptr, w, h, exact, cap, C.byref(n), 6) == kb._lib.KBN_OK and 0 < n.value <= cap
    for bad in ((None, w, h, exact, cap, C.byref(n), 6), (ptr, 0, h, exact, cap, C.byref(n), 6), (ptr, w, h, exact, cap, C.byref(n), 10),
                (ptr, w, h, exact, cap, C.byref(n), -2), (ptr, w, h, None, cap, C.byref(n), 6), (ptr, w, h, exact, cap, None, 6)):
        assert lib.kbn_png_encode_rgb8(*bad) == kb._lib.KBN_ERR_INVALID_ARGUMENT
    assert lib.kbn_png_encode_rgb8_bound(0, 5) == 0 and lib.kbn_png_encode_rgb8_bound(5, -1) == 0
    with pytest.raises(KbnError):
        kb.loader.encode_image_png(np.zeros((4, 4), dtype=np.uint8))
    with pytest.raises(KbnError):
        kb.loader.encode_image_png(np.zeros((4, 4, 3), dtype=np.float32))


def test_gray16_encoder_is_unchanged_by_the_shared_file_writer():
    s = np.arange(37 * 50, dtype=np.uint32).reshape(37, 50).astype(np.uint16) * 31
    assert np.array_equal(kb.loader.decode_png(kb.loader.encode_depth_png(s)), s)


# ------------------------------------------------------------------------------------------------ data_utils names
def test_read_write_paths_round_trip(tmp_path):
    paths = ["a/b.png", "c d/e.png", "/abs/f.npy"]
    f = str(tmp_path / "list.txt")
    kb.loader.write_paths(f, paths)
    assert open(f).read() == "a/b.png\nc d/e.png\n/abs/f.npy\n"
    assert kb.loader.read_paths(f) == paths
    kb.loader.write_paths(f, [])
    assert kb.loader.read_paths(f) == []
    with open(f, "w") as o:      # the reference stops at the first empty line; a last line without a newline is read
        o.write("one\ntwo\n\nthree\n")
    assert kb.loader.read_paths(f) == ["one", "two"]
    with open(f, "w") as o:
        o.write("one\ntwo")
    assert kb.loader.read_paths(f) == ["one", "two"]


def test_load_depth_with_validity_map_is_the_references(golden):
    path = os.path.join(rc.IO, "depth_0.png")
    assert kb.loader.load_depth_with_validity_map(path)[0].shape == (24, 40)      # the default format is 'HW'
    for fmt in ("HW", "CHW", "HWC"):
        z, v = kb.loader.load_depth_with_validity_map(path, data_format=fmt)
        for got, name in ((z, "depth"), (v, "map")):
            want = golden[f"validity::{fmt}::{name}"]
            assert got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (fmt, name)
        assert 0 < v.sum() < v.size and set(np.unique(v)) == {0.0, 1.0}
    with pytest.raises(ValueError):
        kb.loader.load_depth_with_validity_map(path, data_format="WHC")


# ------------------------------------------------------------------------------------------------ the settings log
@pytest.mark.parametrize("case", sorted(rc.log_cases()))
def test_settings_log_is_the_references_text(golden, tmp_path, capsys, case):
    function, kwargs = rc.log_cases()[case]
    text = rc.logged_text(getattr(kb.summary, function), kwargs, str(tmp_path / "logs"), case)
    assert text == str(golden["log::" + case])
    assert capsys.readouterr().out == text      # log() prints what it writes
    assert len(text.splitlines()) >= 3


def test_settings_log_covers_six_functions_and_both_forms():
    cases = rc.log_cases()
    assert {f for f, _ in cases.values()} == {"log_input_settings", "log_network_settings", "log_training_settings", "log_loss_func_settings",
                                             "log_evaluation_settings", "log_system_settings"}
    assert "n_batch" in cases["input_train"][1] and "n_batch" not in cases["input_run"][1]
    assert "n_checkpoint" in cases["system_train"][1] and "n_checkpoint" not in cases["system_run"][1]


# ------------------------------------------------------------------------------------------------ refusals
def _lists(tmp_path):
    names = rc.write_lists(str(tmp_path), kb.loader.write_paths)
    return [str(tmp_path / n) for n in names]


def test_run_refuses_the_cpu(tmp_path):
    image, sparse, intrinsics, truth = _lists(tmp_path)
    with pytest.raises(KbnError, match="cpu"):
        kb.inference.run(image, sparse, intrinsics, truth, checkpoint_path=str(tmp_path / "out"), depth_model_restore_path=rc.CHECKPOINT,
                         device="cpu")
    assert not os.path.exists(tmp_path / "out")


@pytest.mark.parametrize("short", ["sparse depth", "intrinsics", "ground truth"])
def test_run_refuses_path_lists_of_different_lengths(tmp_path, short):
    lists = dict(zip(("image", "sparse depth", "intrinsics", "ground truth"), _lists(tmp_path)))
    kb.loader.write_paths(lists[short], kb.loader.read_paths(lists[short])[:2])
    with pytest.raises(KbnError, match=f"3 image paths, 2 {short} paths"):
        kb.inference.run(lists["image"], lists["sparse depth"], lists["intrinsics"], lists["ground truth"],
                         checkpoint_path=str(tmp_path / "out"), depth_model_restore_path=rc.CHECKPOINT)


def test_run_has_the_references_signature():
    import inspect
    params = inspect.signature(kb.inference.run).parameters
    names = list(params)
    assert names[:4] == ["image_path", "sparse_depth_path", "intrinsics_path", "ground_truth_path"]
    assert names[-4:] == ["batch_size", "workers", "png_level", "return_results"]
    assert all(params[n].kind is inspect.Parameter.KEYWORD_ONLY for n in names[-4:])
    assert [params[n].default for n in names[-4:]] == [8, 8, 6, False]
    assert params["ground_truth_path"].default is None and params["checkpoint_path"].default == "trained_kbnet"
    assert params["max_evaluate_depth"].default == 100.0 and params["save_outputs"].default is False and params["device"].default == "cuda"
    assert names[4:-4] == list(rc.run_settings(kb.kitti_config())) + ["checkpoint_path", "depth_model_restore_path", "save_outputs",
                                                                       "keep_input_filenames", "device"]
    cfg = kb.kitti_config()
    for name, value in rc.run_settings(cfg).items():
        assert params[name].default == value, name


def test_output_writer_makes_the_four_directories_and_refuses_cpu_tensors(tmp_path):
    out = str(tmp_path / "outputs")
    with kb.loader.OutputWriter(out) as writer:
        assert sorted(os.listdir(out)) == sorted(rc.DIRECTORIES)
        image, depth = torch.zeros(1, 3, 4, 8), torch.zeros(1, 1, 4, 8)
        with pytest.raises(KbnError, match="image"):
            writer.submit(["a.png"], image, depth, depth)
    assert all(os.listdir(os.path.join(out, d)) == [] for d in rc.DIRECTORIES)
    with pytest.raises(ValueError):
        kb.loader.OutputWriter(out, normalized_image_range=(0, 2))
    with pytest.raises(KbnError):
        kb.loader.OutputWriter(out, level=11)
    assert kb.loader.image_export_affine([0, 1]) == (255.0, 0.0) and kb.loader.image_export_affine((-1, 1)) == (127.5, 127.5)
    assert kb.loader.image_export_affine([0, 255]) == (1.0, 0.0)


def test_export_pack_refusals():
    with pytest.raises(KbnError, match="nothing to pack"):
        kb.ops.export_pack()
    with pytest.raises(KbnError, match="image"):
        kb.ops.export_pack(image=torch.zeros(1, 3, 4, 8))
    with pytest.raises(KbnError, match="depth_b"):
        kb.ops.export_pack(depth_b=torch.zeros(1, 1, 4, 8))


def test_export_pack_entry_point_checks_its_arguments_before_launching():
    """No GPU here: an accepted call would fail in the launch (KBN_ERR_LAUNCH); every one of these is refused before."""
    lib = kb._lib.load()
    p = [C.c_void_p(4096 * (i + 1)) for i in range(6)]      # never dereferenced
    image, depth_a, depth_b, rgb, samples_a, samples_b = p
    invalid = kb._lib.KBN_ERR_INVALID_ARGUMENT

    def call(image, depth_a, depth_b, rgb, samples_a, samples_b, n=1, h=2, w=4):
        return lib.kbn_export_pack_forward(image, 255.0, 0.0, depth_a, depth_b, rgb, samples_a, samples_b, n, h, w, None)

    assert call(None, None, None, None, None, None) == invalid                      # nothing to do
    assert call(None, depth_a, None, rgb, samples_a, None) == invalid               # an output without its source
    assert call(None, depth_a, None, None, samples_a, samples_b) == invalid
    assert call(None, None, depth_b, None, samples_a, samples_b) == invalid
    assert call(image, None, None, None, None, None) == invalid                     # a source without its output
    assert call(image, depth_a, None, rgb, None, None) == invalid
    assert call(image, depth_a, depth_b, rgb, samples_a, None) == invalid
    for size in ((0, 2, 4), (1, 0, 4), (1, 2, 0), (-1, 2, 4)):                       # n, height or width < 1
        assert call(image, depth_a, depth_b, rgb, samples_a, samples_b, *size) == invalid


def test_wiring():
    assert "export_pack.hip" in kb._build.SOURCES
    for name in ("kbn_export_pack_forward", "kbn_png_encode_rgb8", "kbn_png_encode_rgb8_bound"):
        assert name in kb._lib.SIGNATURES
    assert kb._lib.SIGNATURES["kbn_export_pack_forward"][1][1:3] == [C.c_float, C.c_float]
    assert kb._lib.ABI_VERSION == 11      # symbols were added, nothing changed


# ------------------------------------------------------------------------------------------------ the power of the oracle
def test_oracle_tells_the_rule_from_its_near_misses():
    planted = rc.planted_values()
    image = np.tile(planted, 3)[:3 * planted.size].reshape(1, 3, 1, planted.size)
    for scale, shift in ((255.0, 0.0), (127.5, 127.5), (1.0, 0.0)):
        right = rc.oracle_rgb(image, scale, shift)
        assert right.shape == (1, 1, planted.size, 3)
        if scale != 1.0:
            assert not np.array_equal(right, rc.oracle_rgb(image, scale, shift, rounding=True)), (scale, shift)
    assert not np.array_equal(rc.oracle_rgb(image, 255.0, 0.0), rc.oracle_rgb(image, 256.0, 0.0))
    depth = planted.reshape(1, 1, 1, -1)
    right = rc.oracle_samples(depth)
    assert not np.array_equal(right, rc.oracle_samples(depth, rounding=True))
    assert not np.array_equal(right, rc.oracle_samples(depth, factor=255.0))
    # the planted edges, by hand
    by_value = dict(zip(planted[:13].tolist(), right.reshape(-1)[:13].tolist()))
    assert by_value[1.0] == 256 and by_value[300.0] == 65535 and by_value[256.0] == 65535 and by_value[255.99609375] == 65535
    assert by_value[-3.0] == 0 and by_value[float(np.float32(1.0 / 256.0))] == 1 and by_value[float(planted[12])] == 0
    assert right.reshape(-1)[4] == 0 and right.reshape(-1)[5] == 65535 and right.reshape(-1)[6] == 0      # NaN, +inf, -inf
    rgb = rc.oracle_rgb(image, 255.0, 0.0)[0, 0, :, 0]
    assert rgb[2] == 255 and rgb[3] == 254 and rgb[4] == 0 and rgb[5] == 255 and rgb[6] == 0 and rgb[7] == 0 and rgb[8] == 255
    # every 8-bit pixel k survives k / 255 -> 255 * that -> truncation in float32: the reference's files hold the input's pixels
    ramp = rgb[13:13 + 256].astype(int)
    assert np.array_equal(ramp, np.arange(256))
    assert np.array_equal(ramp, (255 * (np.arange(256, dtype=np.float32) / np.float32(255.0))).astype(np.uint8))


def test_oracle_tells_interleaved_from_planar_on_5x3():
    image, _, _ = rc.make_sources(1, 3, 5, seed=4)
    assert not np.array_equal(rc.oracle_rgb(image, 255.0, 0.0), rc.oracle_rgb(image, 255.0, 0.0, planar=True))
    px = rc.oracle_rgb(image, 255.0, 0.0)
    assert px.shape == (1, 3, 5, 3) and np.array_equal(px[0, 2, 4], rc.oracle_rgb(image[:, :, 2:, 4:], 255.0, 0.0)[0, 0, 0])


def test_oracle_is_the_references_cast_on_the_golden_image(golden):
    """(255, 0) on the normalised frame is `(255 * image).astype(np.uint8)`: the oracle applied to the loader's frame / 255 gives the
    pixels of the files the reference wrote."""
    for i in range(rc.N_FRAMES):
        frame = kb.loader.load_image_triplet(os.path.join(rc.IO, f"triplet_{i}.png"), normalize=False)[1]      # the middle third
        normalised = (torch.from_numpy(frame) / 255.0).numpy()      # transforms.transform: torch's float32 division
        assert np.array_equal(rc.oracle_rgb(normalised[None], 255.0, 0.0)[0], golden[f"file::image::{i}"])
