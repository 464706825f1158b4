"""CPU: the oracle of the image summaries against the reference's recorded colorize and against torch-CPU + matplotlib, the power of
that comparison, the grid's geometry, the host logic of kb.summary / kb.validation and the refusals -- no GPU needed (the kernel
itself is tests/test_summary_gpu.py).

    python -m pytest tests/test_summary_cpu.py -q
"""
import ctypes
import itertools
import os
import re
import sys

import numpy as np
import pytest
import torch

import kbnet_amd as kb
import summary_oracle as so

KbnError = kb._lib.KbnError
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OPTIONAL = ("image0", "image01", "image02", "output_depth0", "sparse_depth0", "validity_map0", "ground_truth0")


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


# ------------------------------------------------------------------------------------------------ the oracle
def test_the_compiled_tables_are_the_recorded_ones_and_matplotlibs():
    """csrc/colormaps.h (what the kernel is compiled with) = the tables the reference's colorize returned (golden) = matplotlib's."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_colormaps
    compiled = gen_colormaps.parse(open(gen_colormaps.HEADER).read())
    assert set(compiled) == set(so.MAPS)
    for name in so.MAPS:
        assert so.table(name).shape == (256, 3) and _same_bits(compiled[name], so.table(name)), name
        assert _same_bits(gen_colormaps.table(name), so.table(name)), name


def test_the_lookup_is_the_references_colorize():
    """so.lookup against log_utils.colorize as recorded: random values in [-0.1, 1.1) and the edge values, bit for bit."""
    g = so.golden()
    for name in so.MAPS:
        assert _same_bits(np.transpose(so.lookup(g["random::x"][:, 0], name), (0, 3, 1, 2)), g["random::" + name]), name
        assert _same_bits(np.transpose(so.lookup(g["edges::x"].reshape(1, 1, -1), name), (0, 3, 1, 2)), g["edges::" + name]), name


def test_lookup_edge_values():
    """negative and -inf: entry 0; -0 and 0: entry 0; exactly 1, above 1, +inf: entry 255; NaN: black; the ends of the last entry."""
    below_one = np.nextafter(np.float32(1.0), np.float32(0.0))
    for name in so.MAPS:
        t = so.table(name)
        got = so.lookup(np.array([-1.0, -np.inf, -0.0, 0.0, 1.0, 1.5, np.inf, np.nan, 255.0 / 256.0, below_one, 1.0 / 256.0,
                                  np.nextafter(np.float32(1.0 / 256.0), np.float32(0.0))], dtype=np.float32), name)
        want = [t[0], t[0], t[0], t[0], t[255], t[255], t[255], np.zeros(3, np.float32), t[255], t[255], t[1], t[0]]
        assert _same_bits(got, np.stack(want)), name


@pytest.mark.parametrize("colorize", [so.table_colorize, so.matplotlib_colorize], ids=["recorded-tables", "matplotlib"])
@pytest.mark.parametrize("edges", [False, True], ids=["random", "edges"])
def test_the_numpy_oracle_is_the_references_torch_expressions(colorize, edges):
    """image_panel / depth_panel (NumPy, what the kernel is held to) = the reference's expressions in torch on the CPU with
    matplotlib's colours and make_grid restated, bit for bit, for every subset of the optional arguments."""
    c = so.case(3, 7, 10, seed=5, edges=edges)
    for mask in itertools.product([False, True], repeat=len(OPTIONAL)):
        args = {k: (c[k] if on else None) for k, on in zip(OPTIONAL, mask)}
        image, _, depth, _ = so.torch_panels(colorize, 100.0, n_display=2, **args)
        ours_image = so.image_panel(args["image0"], args["image01"], args["image02"], n_display=2)
        ours_depth = so.depth_panel(args["output_depth0"], 100.0, args["image0"], args["sparse_depth0"], args["validity_map0"],
                                    args["ground_truth0"], n_display=2)
        for got, want in ((ours_image, image), (ours_depth, depth)):
            assert (got is None) == (want is None), mask
            if want is not None:
                assert _same_bits(got, want.numpy()), mask


def test_a_reciprocal_multiplication_is_caught():
    """The planted mistake: x / 0.10f written as x * (1 / 0.10f).  It moves the value x of a share of the pixels by an ulp (several
    per cent on random data): the oracle's cell value is held to torch's bit for bit and sees every one of them.  A colour moves
    only where x * 256 crosses an integer, which random data does not hit: the second part builds pixels on those boundaries and
    the panels differ there."""
    c = so.case(3, 24, 40, seed=9)
    a, b = c["image0"].numpy(), c["image01"].numpy()
    good, bad = so.photo_err(a, b), so.photo_err(a, b, mistake="reciprocal")
    torchs = (torch.mean(torch.abs(c["image0"] - c["image01"]), dim=1, keepdim=True) / 0.10).numpy()[:, 0]
    share = float((bad != torchs).mean())
    print(f"values changed by the reciprocal: {100 * share:.1f} %")
    assert _same_bits(good, torchs) and 0.02 < share < 0.2
    # errors e = k / 2560 and their neighbours, the same in all three channels: (e / 0.10f) * 256 lies at the integer k
    k = np.arange(1, 256, dtype=np.float64)
    e = (k / 2560.0).astype(np.float32).view(np.uint32)[:, None] + np.arange(-8, 9, dtype=np.int64)[None, :]
    e = e.astype(np.uint32).view(np.float32).reshape(1, 1, 1, -1)
    image0 = torch.zeros(1, 3, 1, e.shape[3])
    image01 = torch.from_numpy(np.repeat(e, 3, axis=1).copy())
    want = so.torch_panels(so.table_colorize, 100.0, image0=image0, image01=image01)[0].numpy()
    assert _same_bits(so.image_panel(image0, image01), want)
    mistaken = so.image_panel(image0, image01, mistake="reciprocal")
    moved = int((mistaken != want).any(axis=0).sum())
    print(f"boundary pixels whose colour the reciprocal moves: {moved} of {e.shape[3]}")
    assert moved > 0


@pytest.mark.parametrize("n, n_display, frames", [(1, 1, 1), (1, 4, 1), (2, 2, 2), (3, 3, 3), (3, 2, 2), (3, 1, 1), (3, 5, 3)])
def test_grid_geometry(n, n_display, frames):
    """B = min(n_display, N) tiles; B == 1: the tile itself; B > 1: 3 x (R H + 4) x (B (2 W + 2) + 2), tile k at row 2, column
    k (2 W + 2) + 2, zeros everywhere else."""
    h, w = 5, 6
    c = so.case(n, h, w, seed=n)
    panel = so.image_panel(c["image0"], c["image01"], c["image02"], n_display=n_display)
    assert panel.shape == so.panel_shape(3, frames, h, w) == kb.ops.summary_panel_shape(3, frames, h, w)
    if frames == 1:
        assert panel.shape == (3, 3 * h, 2 * w)
        assert _same_bits(panel[:, :h, :w], c["image0"][0].numpy()) and not panel[:, :h, w:].any()
        return
    assert panel.shape == (3, 3 * h + 4, frames * (2 * w + 2) + 2)
    covered = np.zeros(panel.shape[1:], dtype=bool)
    for k in range(frames):
        x0 = k * (2 * w + 2) + 2
        assert _same_bits(panel[:, 2:2 + h, x0:x0 + w], c["image0"][k].numpy())
        assert _same_bits(panel[:, 2 + h:2 + 2 * h, x0:x0 + w], c["image01"][k].numpy())
        assert _same_bits(panel[:, 2 + 2 * h:2 + 3 * h, x0:x0 + w], c["image02"][k].numpy())
        covered[2:2 + 3 * h, x0:x0 + 2 * w] = True
    assert not panel[:, ~covered].any() and (~covered).sum() == 4 * panel.shape[2] + 3 * h * 2 * (frames + 1)


# ------------------------------------------------------------------------------------------------ host logic
BEST0 = {"step": -1, "mae": np.inf, "rmse": np.inf, "imae": np.inf, "irmse": np.inf}


@pytest.mark.parametrize("best, new, updated", [
    (BEST0, (300.0, 1200.0, 1.3, 3.6), True),                                                     # the first validation
    ((10, 300.0, 1200.0, 1.3, 3.6), (299.0, 1199.0, 1.2, 3.7), True),                             # three improved
    ((10, 300.0, 1200.0, 1.3, 3.6), (299.0, 1199.0, 1.4, 3.7), False),                            # two improved: not more than two
    ((10, 300.0, 1200.0, 1.3, 3.6), (300.004, 1200.004, 1.304, 3.7), True),                       # ties after rounding count (<=)
    ((10, 300.0, 1200.0, 1.3, 3.6), (300.006, 1200.006, 1.306, 3.5), False),                      # 300.01 > 300.00: one improved
    ((10, 300.0, 1200.0, 1.3, 3.6), (300.0, 1200.0, 1.3, 3.6), True),                             # all equal
    ((10, 300.0, 1200.0, 1.3, 3.6), (np.nan, 1199.0, 1.2, 3.5), True),                            # a NaN never improves; three others do
    ((10, 300.0, 1200.0, 1.3, 3.6), (np.nan, np.nan, 1.2, 3.5), False),
])
def test_update_best_results(best, new, updated):
    if not isinstance(best, dict):
        best = dict(zip(("step", "mae", "rmse", "imae", "irmse"), best))
    before = dict(best)
    got = kb.validation.update_best_results(best, 20, *new)
    assert best == before and got is not best                         # a function of its inputs
    # the reference's lines (src/kbnet.py:646-661), restated
    n_improve = sum(int(np.round(v, 2) <= np.round(best[k], 2)) for k, v in zip(("mae", "rmse", "imae", "irmse"), new))
    assert (n_improve > 2) == updated
    if updated:
        assert got["step"] == 20 and [got[k] for k in ("mae", "rmse", "imae", "irmse")] == pytest.approx(list(new), nan_ok=True)
    else:
        assert got == before


def test_log_writes_the_references_file(tmp_path, capsys):
    """reference src/log_utils.py:23-46: a directory that does not exist is made and the file started; an existing one is appended to."""
    path = str(tmp_path / "new" / "deeper" / "results.txt")
    kb.summary.log("first", path)
    kb.summary.log("second", path)
    assert open(path).read() == "first\nsecond\n"
    existing = str(tmp_path / "results.txt")
    with open(existing, "w") as f:
        f.write("kept\n")
    kb.summary.log("third", existing, to_console=False)
    assert open(existing).read() == "kept\nthird\n"
    kb.summary.log("console only")
    assert capsys.readouterr().out == "first\nsecond\nconsole only\n"


def test_signatures_are_the_references():
    import inspect
    ls = inspect.signature(kb.modules.KBNetModel.log_summary)
    assert list(ls.parameters) == ["self", "summary_writer", "tag", "step", "image0", "image01", "image02", "output_depth0", "sparse_depth0",
                                   "validity_map0", "ground_truth0", "pose01", "pose02", "scalars", "n_display"]
    assert [p.default for p in list(ls.parameters.values())[4:]] == [None] * 9 + [{}, 4]
    v = inspect.signature(kb.validation.validate)
    assert list(v.parameters)[:8] == ["depth_model", "dataloader", "ground_truths", "step", "best_results", "min_evaluate_depth",
                                      "max_evaluate_depth", "device"]
    assert {k: v.parameters[k].default for k in ("summary_writer", "n_summary_display", "n_summary_display_interval", "log_path")} == \
        {"summary_writer": None, "n_summary_display": 4, "n_summary_display_interval": 250, "log_path": None}
    for module in ("tensorboard", "torchvision", "matplotlib"):
        for name in ("summary", "validation"):
            assert not re.search(rf"^\s*(import|from)\s+{module}", open(getattr(kb, name).__file__).read(), flags=re.M)


# ------------------------------------------------------------------------------------------------ refusals
def test_the_ops_refuse_cpu_tensors_and_wrong_shapes():
    c = so.case(2, 4, 8)
    with pytest.raises(KbnError, match="no CPU fallback"):
        kb.ops.summary_image_panel(c["image0"], c["image01"])
    with pytest.raises(KbnError, match="no CPU fallback"):
        kb.ops.summary_depth_panel(c["output_depth0"], 100.0, image0=c["image0"])
    with pytest.raises(KbnError, match="no CPU fallback"):
        kb.summary.colorize(c["output_depth0"], "viridis")
    with pytest.raises(ValueError, match="magma"):
        kb.summary.colorize(c["output_depth0"])
    with pytest.raises(ValueError, match="jet"):
        kb.summary.colorize(c["output_depth0"], "jet")
    with pytest.raises(KbnError, match="image01 has 1 channels"):           # the reference's torch.cat fails there too
        kb.ops.summary_image_panel(c["image0"], c["image01"][:, :1])
    with pytest.raises(KbnError, match="image0 has 1 channels"):
        kb.ops.summary_depth_panel(c["output_depth0"], 100.0, image0=c["image0"][:, :1])
    with pytest.raises(KbnError, match="ground_truth0 has 1 channels"):
        kb.ops.summary_depth_panel(c["output_depth0"], 100.0, ground_truth0=c["ground_truth0"][:, :1])
    with pytest.raises(KbnError, match="N, H and W must agree"):
        kb.ops.summary_image_panel(c["image0"], c["image01"][:, :, :3])
    with pytest.raises(KbnError, match="N, H and W must agree"):
        kb.ops.summary_depth_panel(c["output_depth0"], 100.0, sparse_depth0=c["sparse_depth0"][:1], validity_map0=c["validity_map0"])
    with pytest.raises(KbnError, match="float32"):
        kb.ops.summary_image_panel(c["image0"].double(), c["image01"])
    with pytest.raises(KbnError, match="n_display"):
        kb.ops.summary_image_panel(c["image0"], c["image01"], n_display=0)
    # nothing given: the reference logs no image
    assert kb.ops.summary_image_panel(None) is None and kb.ops.summary_depth_panel(None, 100.0) is None


def test_the_entry_point_names_what_it_refuses():
    """kbn_summary_panel_forward checks its records before anything is launched (no GPU needed)."""
    lib = kb._lib.load()
    L = kb._lib
    buf = (ctypes.c_float * 64)()
    ptr = ctypes.addressof(buf)

    def rows(left_kind=L.KBN_SUMMARY_CELL_COPY, channels=3, stride_w=1):
        r = (L.SummaryRow * 2)()
        for row in r:
            row.left.kind = left_kind
            row.left.src[0].data, row.left.src[0].channels = ptr, channels
            row.left.src[0].stride_n, row.left.src[0].stride_c, row.left.src[0].stride_h, row.left.src[0].stride_w = 16, 4, 4, stride_w
            row.right.kind = L.KBN_SUMMARY_CELL_ZERO
        return r

    call = lambda r, n_rows=2, frames=1, h=1, w=4, out=ptr: lib.kbn_summary_panel_forward(r, n_rows, frames, h, w, 100.0, out, None)
    assert call(rows(), n_rows=1) == call(rows(), n_rows=5) == L.KBN_ERR_INVALID_ARGUMENT
    assert call(rows(), frames=0) == call(rows(), h=0) == call(rows(), out=None) == L.KBN_ERR_INVALID_ARGUMENT
    assert call(rows(stride_w=-1)) == L.KBN_ERR_INVALID_ARGUMENT
    assert call(rows(left_kind=L.KBN_SUMMARY_CELL_PHOTO_ERR)) == L.KBN_ERR_INVALID_ARGUMENT       # an error map on the left
    assert call(rows(channels=1)) == L.KBN_ERR_UNSUPPORTED                                        # an image that is not 3-channel
    assert call(rows(left_kind=L.KBN_SUMMARY_CELL_DEPTH, channels=3)) == L.KBN_ERR_UNSUPPORTED
    assert call(rows(), frames=40000, h=4000, w=4000) == L.KBN_ERR_UNSUPPORTED                    # 2^31 elements or more
    assert lib.kbn_summary_colorize_forward(ptr, 4, 4, 1, 1, 1, 4, 7, ptr, None) == L.KBN_ERR_UNSUPPORTED
    assert lib.kbn_status_string(L.KBN_ERR_UNSUPPORTED) == b"configuration outside the kernel limits"


def test_binding_records_are_the_headers():
    header = open(os.path.join(ROOT, "include", "kbnet_hip.h")).read()
    for name in ("KBN_SUMMARY_CELL_ZERO", "KBN_SUMMARY_CELL_COPY", "KBN_SUMMARY_CELL_PHOTO_ERR", "KBN_SUMMARY_CELL_DEPTH", "KBN_SUMMARY_CELL_REL_ERR",
                 "KBN_SUMMARY_COLORMAP_VIRIDIS", "KBN_SUMMARY_COLORMAP_INFERNO", "KBN_SUMMARY_MAX_ROWS"):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == getattr(kb._lib, name), name
    # the structs, field by field: C types of the header against the ctypes mirror
    ctype = {"const float*": ctypes.c_void_p, "long long": ctypes.c_longlong, "int": ctypes.c_int,
             "kbn_summary_source": kb._lib.SummarySource, "kbn_summary_cell": kb._lib.SummaryCell}
    for struct, mirror in (("kbn_summary_source", kb._lib.SummarySource), ("kbn_summary_cell", kb._lib.SummaryCell), ("kbn_summary_row", kb._lib.SummaryRow)):
        body = re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", header, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            kind, names = re.match(r"(const float\*|long long|int|kbn_summary_\w+)\s+(.*)", decl).groups()
            for name in (x.strip() for x in names.split(",")):
                m = re.match(r"(\w+)\[(\d+)\]", name)
                fields.append((m.group(1), ctype[kind] * int(m.group(2))) if m else (name, ctype[kind]))
        assert [(n, t) for n, t in mirror._fields_] == fields, struct
    assert ctypes.sizeof(kb._lib.SummarySource) == 48 and ctypes.sizeof(kb._lib.SummaryCell) == 152 and ctypes.sizeof(kb._lib.SummaryRow) == 304
    assert "summary.hip" in kb._build.SOURCES
    assert kb._lib.SIGNATURES["kbn_summary_panel_forward"][1][0]._type_ is kb._lib.SummaryRow
