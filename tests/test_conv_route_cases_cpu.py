"""The route table of tests/conv_route_cases.py on the CPU: its coverage, the seams its forced tiles cross, the gates (measured
here from torch's own fp32 conv and an fp32 Winograd evaluation against fp64) and the power of those gates against six planted
mistakes in an fp64 stand-in.  tests/test_conv_routes_gpu.py runs the same table on the device."""
import torch
import torch.nn.functional as F

import conv_route_cases as rc


def test_every_required_route_is_declared():
    declared = [c.route for c in rc.ALL_CASES]
    for want in rc.REQUIRED_ROUTES:
        assert any(rc.matches(r, want) for r in declared), want
    forced = set()
    for c in rc.ALL_CASES:
        fam = c.route["family"]
        if c.force == "tiles":
            forced |= {(fam, mw, twb) for _, twb, mw in rc.forced_tiles(c)}
        elif c.force == "rt":
            forced |= {(fam, rt, ct) for rt, ct in rc.WINO_REGIONS}
        elif c.force == "twb":
            forced |= {(fam, 0, 1), (fam, 0, 2)}
    assert set(rc.REQUIRED_FORCED) <= forced, set(rc.REQUIRED_FORCED) - forced
    # the layouts and extras the table promises
    assert {s.layout for c in rc.ALL_CASES for s in c.srcs} == {"dense", "slice", "off1"}
    assert {c.out for c in rc.ALL_CASES} == {"dense", "slice", "off1"}
    assert {s.kind for c in rc.ALL_CASES for s in c.srcs} == {"tensor", "coords", "xyz", "xyz_dense"}
    for fam in ("dma", "dma_syn", "wino", "igemm_pipe", "up2x9", "up2x_dma", "up2x"):
        assert any(c.absmax for c in rc.ALL_CASES if c.route["family"] == fam), f"no out_absmax case on {fam}"
    assert any(c.transposed for c in rc.ALL_CASES)
    # the one launch whose instantiation gives the LDS epilogue up, and its neighbour that keeps it: by the geometry, not by the library
    assert rc.epi_in_effect(1, 3, 1, 4, 2, 8, 4) == 0 and rc.dma_stage_bytes(3, 1, 4, 2, 8, 4) == 32256
    assert rc.epi_in_effect(1, 3, 1, 4, 2, 8, 1) == 1
    assert rc.BY_NAME["dma_k3s1_epi_given_up"].route["epi_lds"] == 0 and rc.BY_NAME["dma_k3s1_epi_kept"].route["epi_lds"] == 1


def test_forced_tiles_cross_a_seam_in_both_directions():
    """More than one tile along the rows and along the columns under every forced shape, the last one ragged in at least one
    direction (in both for the direct kernels' tiles of more than one row)."""
    for c in rc.ALL_CASES:
        if not c.force:
            continue
        eh, ew = rc.tiled_extent(c)
        shapes = rc.tile_shapes(c)
        assert shapes, c.name
        for th, tw in shapes:
            assert eh > th and ew > tw, (c.name, (eh, ew), (th, tw))
            assert eh % th or ew % tw, (c.name, (eh, ew), (th, tw))
            if c.force == "tiles":
                assert ew % tw and (th == 1 or eh % th), (c.name, (eh, ew), (th, tw))


def _measure():
    worst = {"direct": (0.0, None), "wino": (0.0, None)}
    for c in rc.ALL_CASES:
        data = rc.make_inputs(c)
        ref = rc.activate(rc.pre_activation(c, data), c.slope)
        got32 = rc.pre_activation(c, data, torch.float32)
        f = rc.fraction(rc.activate(got32, c.slope, ref > 0 if c.slope is not None else None), ref)
        if f > worst["direct"][0]:
            worst["direct"] = (f, c.name)
        if c.route["family"] == "wino":
            x32 = rc.concat_input(c, data, torch.float32)
            y = rc.winograd_conv3x3(x32, data["weight"])
            f = rc.fraction(rc.activate(y, c.slope, ref > 0 if c.slope is not None else None), ref)
            if f > worst["wino"][0]:
                worst["wino"] = (f, c.name)
    return worst


def test_gates_come_from_the_cpu_measurement():
    worst = _measure()
    for kind, const in rc.GATES.items():
        f, name = worst[kind]
        print(f"{kind}: worst fp32 CPU fraction {f:.3e} ({name}) -> gate {rc.gate_from(f):.0e}; the table's constant {const:.0e}")
        assert const <= rc.GATE_CEILING
        # the constant is this measurement's gate where it was written down; a CPU whose conv sums in another order moves the
        # worst figure by some percent, never by a factor, so the constant must stay within a factor of two of the gate measured here
        assert 0.5 * rc.gate_from(f) <= const <= 2.0 * rc.gate_from(f), (kind, f, const)


# ------------------------------------------------------------------------------------------------ power
def _ref(c, data):
    return rc.pre_activation(c, data)


def _far(bad, ref, gate, what):
    f = rc.fraction(bad, ref)
    print(f"planted: {what}: fraction {f:.2e} = {f / gate:.0f} x the gate")
    assert f > 10 * gate, (what, f)


def test_planted_mistakes_leave_the_gates():
    """fp64 stand-ins of what a wrong kernel would compute, on the named cases (no activation: it only shrinks both sides alike)."""
    # 1. the last, ragged K chunk dropped: 15 channels in chunks of 4 -> 12
    c = rc.BY_NAME["syn_k3s1_3_5_7"]
    data = rc.make_inputs(c)
    x = rc.concat_input(c, data)
    ck = c.route["CK"]
    keep = c.cin // ck * ck
    assert keep < c.cin
    bad = F.conv2d(x[:, :keep], data["weight"].double()[:, :keep], padding=1)
    _far(bad, _ref(c, data), rc.GATES[c.gate], "last ragged K chunk dropped")
    # 2. a tile's left halo column taken as zero at an interior seam (64-column tiles: column 64 of 72)
    c = rc.BY_NAME["dma_k3s1_ck8_nb4_nowino"]
    data = rc.make_inputs(c)
    x, ref = rc.concat_input(c, data), _ref(c, data)
    bad = ref.clone()
    xz = x.clone()
    xz[..., 63] = 0
    bad[..., 64] = F.conv2d(xz, data["weight"].double(), padding=1)[..., 64]
    _far(bad, ref, rc.GATES[c.gate], "left halo column zero at a seam")
    # 3. source two read at source one's batch stride (source one is a 5-channel slice of 10 planes a frame, source two dense: 16)
    c = rc.BY_NAME["kbnet_slice_input_k1s2"]
    data = rc.make_inputs(c)
    n, h, w = c.n, c.h, c.w
    two = data["x"][1].double().contiguous()
    stride_one = (c.srcs[0].c + 5) * h * w
    assert c.srcs[0].layout == "slice" and stride_one < c.srcs[1].c * h * w
    wrong = torch.as_strided(two, two.shape, (stride_one, h * w, w, 1))
    bad = F.conv2d(torch.cat([data["x"][0].double(), wrong], 1), data["weight"].double(), stride=c.stride)
    _far(bad, _ref(c, data), rc.GATES[c.gate], "source two at source one's batch stride")
    # 4. a stride-2 conv reading the odd pixels
    c = rc.BY_NAME["dma_k3s2_w136"]
    data = rc.make_inputs(c)
    x = rc.concat_input(c, data)
    bad = F.conv2d(F.pad(x, (0, 1, 0, 1))[:, :, 1:, 1:], data["weight"].double(), stride=2, padding=1)
    _far(bad, _ref(c, data), rc.GATES[c.gate], "stride-2 conv on odd pixels")
    # 5. the nearest map off by one in the last row of the 2h - 1 resize
    c = rc.BY_NAME["gen_resize_2h_minus_1"]
    data = rc.make_inputs(c)
    xr = rc.concat_input(c, data)
    src = torch.cat([s.double() for s in data["x"]], 1)
    rows = torch.floor(torch.arange(c.h, dtype=torch.float32) * (torch.tensor(float(src.shape[2])) / c.h)).long().clamp_max(src.shape[2] - 1)
    cols = torch.floor(torch.arange(c.w, dtype=torch.float32) * (torch.tensor(float(src.shape[3])) / c.w)).long().clamp_max(src.shape[3] - 1)
    assert torch.equal(src[:, :, rows][:, :, :, cols], xr), "the stand-in's own nearest map is torch's"
    rows[-1] -= 1
    bad = F.conv2d(src[:, :, rows][:, :, :, cols], data["weight"].double(), padding=1)
    _far(bad, _ref(c, data), rc.GATES[c.gate], "nearest map off by one in the last row")
    # 6. the Winograd output's last odd row taken from the padded row below it
    c = rc.BY_NAME["wino_cout130_n3"]
    assert c.h & 1
    data = rc.make_inputs(c)
    full = rc.winograd_conv3x3(rc.concat_input(c, data), data["weight"].double(), full=True)
    ref = _ref(c, data)
    assert rc.fraction(full[:, :, :c.h, :c.w], ref) < 1e-12
    bad = full[:, :, :c.h, :c.w].clone()
    bad[:, :, c.h - 1] = full[:, :, c.h, :c.w]
    _far(bad, ref, rc.GATES[c.gate], "Winograd last odd row from the padded row")
