"""GPU: the image summaries (csrc/summary.hip through ops.summary_image_panel / ops.summary_depth_panel), kb.summary.colorize,
KBNetModel.log_summary and kb.validation.validate against the host oracle (tests/summary_oracle.py; tests/test_summary_cpu.py holds
that oracle to the reference) -- the panels bit for bit.

    python -m pytest tests/test_summary_gpu.py -m gpu -q
"""
import itertools

import numpy as np
import pytest
import torch

import kbnet_amd as kb
import summary_oracle as so

pytestmark = pytest.mark.gpu

MAX_DEPTH = 100.0
SHAPES = [(3, 13, 21), (2, 8, 64)]      # an odd width (one pixel a thread) and a multiple of four (16-byte loads)
OPTIONAL = ("image0", "image01", "image02", "output_depth0", "sparse_depth0", "validity_map0", "ground_truth0")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need a visible MI355X (run with -m gpu on a GPU box)")
    kb._lib.load()   # a missing extension is an error on a GPU box, never a skip
    return torch.device("cuda:0")


_CASES = {}


def _case(shape, edges):
    """The CPU tensors of a case, computed once and shared (nobody writes them)."""
    key = (shape, edges)
    if key not in _CASES:
        _CASES[key] = so.case(*shape, seed=17 + len(_CASES), edges=edges, max_predict_depth=MAX_DEPTH)
    return _CASES[key]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_panel(got, want, what):
    """The panel against the oracle's, bit for bit."""
    assert (got is None) == (want is None), what
    if want is None:
        return
    assert got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == want.shape, (what, tuple(got.shape), want.shape)
    differ = _bits(got.cpu().numpy()) != _bits(want)
    assert not differ.any(), (what, int(differ.sum()), np.argwhere(differ)[:5].tolist())


def _panels(c, dev, n_display, keys=OPTIONAL, prefill=True, put=None):
    """Both panels for the arguments `keys` of case c.  `prefill`: into output memory filled with NaN, so that an element the kernel
    does not write shows.  Asserts that no input changed."""
    put = put or (lambda name, t: t.to(dev))
    args = {k: (put(k, c[k]) if k in keys else None) for k in OPTIONAL}
    before = {k: t.clone() for k, t in args.items() if t is not None}
    outs = [None, None]
    if prefill:
        for i, want in enumerate((so.image_panel(c["image0"] if "image0" in keys else None, c["image01"] if "image01" in keys else None,
                                                 c["image02"] if "image02" in keys else None, n_display),
                                  _want_depth(c, keys, n_display))):
            if want is not None:
                outs[i] = torch.full(want.shape, float("nan"), device=dev)
    image = kb.ops.summary_image_panel(args["image0"], args["image01"], args["image02"], n_display=n_display, out=outs[0])
    depth = kb.ops.summary_depth_panel(args["output_depth0"], MAX_DEPTH, args["image0"], args["sparse_depth0"], args["validity_map0"],
                                       args["ground_truth0"], n_display=n_display, out=outs[1])
    torch.cuda.synchronize()
    for k, t in before.items():
        assert torch.equal(args[k].view(torch.int32) if args[k].is_contiguous() else args[k].contiguous().view(torch.int32),
                           t.contiguous().view(torch.int32)), k
    if prefill:
        assert (image is None or image.data_ptr() == outs[0].data_ptr()) and (depth is None or depth.data_ptr() == outs[1].data_ptr())
    return image, depth


def _want_image(c, keys, n_display):
    return so.image_panel(*[c[k] if k in keys else None for k in ("image0", "image01", "image02")], n_display=n_display)


def _want_depth(c, keys, n_display):
    g = lambda k: c[k] if k in keys else None
    return so.depth_panel(g("output_depth0"), MAX_DEPTH, g("image0"), g("sparse_depth0"), g("validity_map0"), g("ground_truth0"), n_display=n_display)


@pytest.mark.parametrize("edges", [False, True], ids=["random", "edges"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("n_display", [1, 2, 5])
def test_panels_are_the_oracles_bits(dev, shape, edges, n_display):
    """Both panels with every row, written into NaN-filled memory: n_display 1 (the unpadded single tile), 2 (fewer than N) and 5
    (above N); `edges`: inputs that hold the lookup's edge values (negative, 0, exactly 1, above 1, +-inf, NaN) and a validity map of
    0, 1 and 0.5."""
    c = _case(shape, edges)
    image, depth = _panels(c, dev, n_display)
    frames = min(n_display, shape[0])
    assert tuple(image.shape) == so.panel_shape(3, frames, *shape[1:]) and tuple(depth.shape) == so.panel_shape(4, frames, *shape[1:])
    _assert_panel(image, _want_image(c, OPTIONAL, n_display), "image panel")
    _assert_panel(depth, _want_depth(c, OPTIONAL, n_display), "depth panel")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_subset_of_the_optional_rows(dev, shape):
    """The rows follow the reference's `if`s for all 128 subsets of the optional arguments; None where it logs no image."""
    c = _case(shape, True)
    shown = 0
    for mask in itertools.product([False, True], repeat=len(OPTIONAL)):
        keys = tuple(k for k, on in zip(OPTIONAL, mask) if on)
        image, depth = _panels(c, dev, 2, keys)
        _assert_panel(image, _want_image(c, keys, 2), ("image panel", keys))
        _assert_panel(depth, _want_depth(c, keys, 2), ("depth panel", keys))
        shown += (image is not None) + (depth is not None)
    # image panel: image0 and a warped image (3 x 16 subsets); depth panel: the output and one of image0, sparse + validity, ground truth (13 x 4)
    assert shown == 3 * 16 + 13 * 4


@pytest.mark.parametrize("left", [1, 4], ids=["misaligned", "strided-rows"])
def test_views_take_the_path_their_alignment_allows(dev, left):
    """Inputs as views `left` elements into rows that are 8 longer, NaN around them: left = 1 breaks the 16-byte alignment (scalar
    loads inside the four-pixel items), left = 4 keeps it with rows that are not dense; the ground truth's planes are views of the
    N x 2 x H x W tensor in every case.  Same bits, and nothing outside the views is read into the panel."""
    shape = SHAPES[1]
    c = _case(shape, False)

    def put(name, t):
        n, ch, h, w = t.shape
        base = torch.full((n, ch, h, w + 8), float("nan"), device=dev)
        view = base[..., left:left + w]
        view.copy_(t)
        assert not view.is_contiguous() and (view.data_ptr() % 16 == 0) == (left == 4)
        return view
    image, depth = _panels(c, dev, 2, put=put)
    _assert_panel(image, _want_image(c, OPTIONAL, 2), "image panel")
    _assert_panel(depth, _want_depth(c, OPTIONAL, 2), "depth panel")
    # a [:, 0] view of the ground truth as the sparse depth, its [:, 1] as the validity map: frames that are two planes apart
    gt = c["ground_truth0"].to(dev)
    got = kb.ops.summary_depth_panel(c["output_depth0"].to(dev), MAX_DEPTH, sparse_depth0=gt[:, 0:1], validity_map0=gt[:, 1:2], n_display=2)
    want = so.depth_panel(c["output_depth0"], MAX_DEPTH, sparse_depth0=c["ground_truth0"][:, 0:1], validity_map0=c["ground_truth0"][:, 1:2], n_display=2)
    _assert_panel(got, want, "ground-truth planes as sparse depth")


def test_only_the_displayed_frames_are_read(dev):
    """Frames from n_display on may hold anything: they are not part of the panel."""
    c = _case(SHAPES[0], False)
    poisoned = {k: t.clone() for k, t in c.items()}
    for t in poisoned.values():
        t[2:] = float("nan")
    image, depth = _panels(poisoned, dev, 2)
    _assert_panel(image, _want_image(c, OPTIONAL, 2), "image panel")
    _assert_panel(depth, _want_depth(c, OPTIONAL, 2), "depth panel")


def test_colorize_is_the_references(dev):
    """kb.summary.colorize on the device = log_utils.colorize as recorded (random values, the edge values), and of a strided view."""
    g = so.golden()
    for name in so.MAPS:
        got = kb.summary.colorize(torch.from_numpy(g["random::x"]).to(dev), name)
        assert got.is_cuda and not (_bits(got.cpu().numpy()) != _bits(g["random::" + name])).any(), name
        edges = torch.from_numpy(g["edges::x"].reshape(1, 1, 1, -1)).to(dev)
        assert not (_bits(kb.summary.colorize(edges, name).cpu().numpy()) != _bits(g["edges::" + name])).any(), name
        wide = torch.from_numpy(g["random::x"]).to(dev).repeat(1, 2, 1, 1)
        assert torch.equal(kb.summary.colorize(wide[:, 1:2, :, ::2], name), got[..., ::2])


class Writer:
    """Records what a SummaryWriter would be asked to do."""
    def __init__(self):
        self.calls = []

    def add_image(self, tag, img_tensor, global_step=None):
        self.calls.append(("add_image", tag, img_tensor, global_step))

    def add_histogram(self, tag, values, global_step=None):
        self.calls.append(("add_histogram", tag, values, global_step))

    def add_scalar(self, tag, scalar_value, global_step=None):
        self.calls.append(("add_scalar", tag, scalar_value, global_step))


@pytest.fixture(scope="module")
def model(dev):
    cfg = kb.kitti_config().narrow()
    m = kb.modules.KBNetModel.from_config(cfg, dev)
    m.load_state_dicts(*kb.synthetic.make_state_dicts(cfg, seed=0, gain=1.3))
    assert m.max_predict_depth == MAX_DEPTH
    return m


def _assert_calls(got, want):
    assert [(c[0], c[1], c[3]) for c in got] == [(c[0], c[1], c[3]) for c in want]
    for (method, tag, payload, _), (_, _, expected, _) in zip(got, want):
        if method == "add_image":
            assert payload.is_cuda and payload.dim() == 3
            _assert_panel(payload, expected, tag)
        elif method == "add_histogram":
            assert payload.shape == expected.shape and torch.equal(payload.cpu(), expected.cpu()), tag
        else:
            assert payload is expected, tag


@pytest.mark.parametrize("given", ["train", "eval", "poses-only", "image0-only"])
def test_log_summary_makes_the_references_calls(dev, model, given):
    """The call sequence, the tags, the steps and the image tensors of log_summary with a recording writer, for the two calls the
    reference makes (src/kbnet.py:459-472 in the training loop, :625-635 in validate) and two that log no image."""
    c = _case(SHAPES[0], False)
    on = {k: t.to(dev) for k, t in c.items()}
    pose01, pose02 = torch.eye(4, device=dev).repeat(3, 1, 1), torch.eye(4, device=dev).repeat(3, 1, 1)
    pose01[:, :3, 3] = torch.arange(9.0, device=dev).reshape(3, 3)
    pose02[:, :3, 3] = -torch.arange(9.0, device=dev).reshape(3, 3)
    scalars = {"loss": torch.tensor(0.25, device=dev), "loss_color": 0.5}
    if given == "train":
        kw = dict(image0=on["image0"], image01=on["image01"], image02=on["image02"], output_depth0=on["output_depth0"],
                  sparse_depth0=on["sparse_depth0"], validity_map0=on["validity_map0"], pose01=pose01, pose02=pose02, scalars=scalars, n_display=2)
    elif given == "eval":
        kw = dict(image0=on["image0"], output_depth0=on["output_depth0"], sparse_depth0=on["sparse_depth0"], validity_map0=on["validity_map0"],
                  ground_truth0=on["ground_truth0"], scalars={"mae": np.float64(1.5)}, n_display=4)
    elif given == "poses-only":
        kw = dict(pose01=pose01, scalars=scalars)
    else:
        kw = dict(image0=on["image0"])
    writer = Writer()
    model.log_summary(writer, given, 7, **kw)
    torch.cuda.synchronize()
    want = so.expected_calls(MAX_DEPTH, given, 7, **{k: (v.cpu() if isinstance(v, torch.Tensor) and k != "scalars" else v) for k, v in kw.items()})
    _assert_calls(writer.calls, want)
    if given == "train":      # handed over as they are
        assert writer.calls[0][2] is on["output_depth0"] and writer.calls[1][2] is on["sparse_depth0"]
        assert [c[1] for c in writer.calls[-2:]] == ["train_image0_image01-error_image02-error", "train_image0_output0_sparse0-error"]
        assert [c[0] for c in writer.calls] == ["add_histogram"] * 8 + ["add_scalar"] * 2 + ["add_image"] * 2
    if given == "eval":
        assert writer.calls[-1][1] == "eval_image0_output0_sparse0-error_groundtruth0-error" and len(writer.calls) == 5
        assert writer.calls[2][2].data_ptr() == on["ground_truth0"].data_ptr() and tuple(writer.calls[2][2].shape) == (3, 1, 13, 21)
    if given in ("poses-only", "image0-only"):
        assert not any(c[0] == "add_image" for c in writer.calls)


# ------------------------------------------------------------------------------------------------ validate
def _numpy_metrics(output, gt, validity, lo, hi):
    """The reference's four metrics of one frame (src/kbnet.py:601-615, src/eval_utils.py) in fp64."""
    mask = (validity > 0) & (gt > lo) & (gt < hi)
    o, g = output[mask].astype(np.float64), gt[mask].astype(np.float64)
    mae = np.mean(np.abs(1000.0 * o - 1000.0 * g))
    rmse = np.sqrt(np.mean((1000.0 * g - 1000.0 * o) ** 2))
    imae = np.mean(np.abs(1.0 / (0.001 * o) - 1.0 / (0.001 * g)))
    irmse = np.sqrt(np.mean((1.0 / (0.001 * g) - 1.0 / (0.001 * o)) ** 2))
    return mae, rmse, imae, irmse


_VALIDATION = {}


def _validation_inputs():
    if not _VALIDATION:
        image, sparse, _, k = kb.synthetic.make_frames(5, 64, 96, "kitti", seed=3)
        rng = np.random.default_rng(8)
        gt_depth = rng.uniform(0.5, 90.0, size=(5, 64, 96)).astype(np.float32)
        gt_valid = (rng.random((5, 64, 96)) < 0.5).astype(np.float32)
        _VALIDATION.update(image=image * 255.0, sparse=sparse, k=k, gt=[np.stack([d, v], axis=-1) for d, v in zip(gt_depth, gt_valid)])
    return _VALIDATION


@pytest.mark.parametrize("batch", [1, 2])
def test_validate(dev, model, batch, tmp_path, monkeypatch, capsys):
    """Five frames at batch size 1 and 2 (a short last batch): each frame's metrics within 2e-5 relative of NumPy's formulas on the
    model's own depth maps, the mean over frames, the reference's log lines character for character, the best-results rule, one
    copy of the metrics to the host, the summary of every second frame."""
    v = _validation_inputs()
    lo, hi = 1.0, 80.0
    batches = [(v["image"][i:i + batch], v["sparse"][i:i + batch], v["k"][i:i + batch]) for i in range(0, 5, batch)]
    # the model's own depth maps, by the same steps on the same batches
    want = []
    with torch.no_grad():
        for i, (image, sparse, k) in enumerate(batches):
            img, validity, _ = kb.ops.preprocess(image.to(dev), sparse.to(dev))
            depth = model.forward(img, sparse.to(dev), validity, k.to(dev)).cpu().numpy()
            for j in range(depth.shape[0]):
                gt = v["gt"][i * batch + j]
                want.append(_numpy_metrics(depth[j, 0], gt[..., 0], gt[..., 1], lo, hi))
    want = np.array(want)
    copies = []
    real_cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (copies.append(tuple(self.shape)) if self.is_cuda else None, real_cpu(self, *a, **k))[1])
    log_path = str(tmp_path / "logs" / "results.txt")
    best0 = {"step": -1, "mae": np.inf, "rmse": np.inf, "imae": np.inf, "irmse": np.inf}
    best, per_frame = kb.validation.validate(model, batches, v["gt"], 100, best0, lo, hi, dev, log_path=log_path, return_metrics=True)
    monkeypatch.undo()
    printed = capsys.readouterr().out.splitlines()
    assert copies == [(5, 4)]                                             # the metrics reach the host once, nothing else does
    assert per_frame.shape == (5, 4) and per_frame.dtype == torch.float64 and not per_frame.is_cuda
    rel = np.abs(per_frame.numpy() - want) / np.abs(want)
    print("validate: per-frame metrics, worst relative distance from NumPy's:", rel.max())
    assert rel.max() < 2e-5
    mean = [np.mean(column) for column in per_frame.numpy().T]
    assert best0["step"] == -1 and best == {"step": 100, "mae": mean[0], "rmse": mean[1], "imae": mean[2], "irmse": mean[3]}
    header = "{:>8}  {:>8}  {:>8}  {:>8}  {:>8}".format("Step", "MAE", "RMSE", "iMAE", "iRMSE")
    values = "{:8}  {:8.3f}  {:8.3f}  {:8.3f}  {:8.3f}".format(100, *mean)
    lines = ["Validation results:", header, values, "Best results:", header, values]
    assert open(log_path).read() == "\n".join(lines) + "\n"
    assert printed[-6:] == lines
    # a later validation that is no better keeps the best; the ground truth as one tensor, the summaries of frames 0, 2 and 4
    better = {"step": 50, "mae": mean[0] / 2, "rmse": mean[1] / 2, "imae": mean[2], "irmse": mean[3] / 2}
    writer = Writer()
    gt_tensor = torch.from_numpy(np.stack([np.transpose(g, (2, 0, 1)) for g in v["gt"]]))
    kept = kb.validation.validate(model, batches, gt_tensor, 200, better, lo, hi, dev, summary_writer=writer, n_summary_display=2,
                                  n_summary_display_interval=2, log_path=log_path)
    assert kept == better
    tail = open(log_path).read().splitlines()[-6:]
    assert tail[2] == values.replace("     100", "     200", 1) and tail[5] == "{:8}  {:8.3f}  {:8.3f}  {:8.3f}  {:8.3f}".format(
        50, better["mae"], better["rmse"], better["imae"], better["irmse"])
    # as the reference's: no warped images in validate, so the image panel has one row and is not logged
    assert [c[0] for c in writer.calls] == ["add_histogram"] * 3 + ["add_scalar"] * 4 + ["add_image"]
    assert writer.calls[-1][1] == "eval_image0_output0_sparse0-error_groundtruth0-error"
    assert [c[1] for c in writer.calls[3:7]] == ["eval_mae", "eval_rmse", "eval_imae", "eval_irmse"] and all(c[3] == 200 for c in writer.calls)
    assert writer.calls[0][2].shape[0] == 3 and tuple(writer.calls[-1][2].shape) == so.panel_shape(4, 2, 64, 96)
    assert torch.equal(writer.calls[2][2][:, 0].cpu(), gt_tensor[0::2, 0])
    with pytest.raises(kb._lib.KbnError, match="ground truths"):
        kb.validation.validate(model, batches, v["gt"][:4], 300, better, lo, hi, dev, log_path=None)
