"""The fp32 conv family, kernel by kernel: every case of tests/conv_route_cases.py runs through ops.conv2d / ops.conv2d_kbnet /
ops.upconv2x, the route the library reports (ops.last_conv_route) must be the one the table declares, and the result is held
against fp64 on the device's own activation branches.  One line a case: route and fraction.

    python -m pytest tests/test_conv_routes_gpu.py -m gpu -q -s
"""
import pytest
import torch

import kbnet_amd as kb
import conv_route_cases as rc
import posenet_grad_oracle as pgo
from conftest import rel_err

pytestmark = pytest.mark.gpu

ops = kb.ops
TIGHT = 2e-5        # tests/test_hip_parity.py's single-op bar on max |a - b| / max |b|
GUARD = -7777.25
PAD = 64            # floats in front of and behind a flat output (256 bytes: the view keeps the allocation's alignment)

OBSERVED = []       # (case name, route) of every launch whose route was checked
FORCED = set()      # (family, MW or RT, TWB or CT) seen under a forced geometry
_DONE = {}          # case name -> None (passed) or the exception it raised


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need a visible MI355X (run with -m gpu on a GPU box)")
    kb._lib.load()
    return torch.device("cuda:0")


def _place(t, layout, dev):
    """`t` on the device as a dense tensor, as channels 3 .. 3 + c of a wider one, or one float into a flat buffer."""
    if layout == "dense":
        return t.to(dev)
    n, c, h, w = t.shape
    if layout == "slice":
        big = torch.full((n, c + 5, h, w), GUARD, device=dev)
        big[:, 3:3 + c] = t.to(dev)
        return big[:, 3:3 + c]
    flat = torch.full((t.numel() + 8,), GUARD, device=dev)
    view = flat[1:1 + t.numel()].view(t.shape)
    view.copy_(t.to(dev))
    assert view.data_ptr() % 16 == 4
    return view


class _Out:
    """The output as a view inside a buffer filled with GUARD."""

    def __init__(self, layout, shape, dev):
        n, c, h, w = shape
        numel = n * c * h * w
        if layout == "slice":
            self.whole = torch.full((n, c + 8, h, w), GUARD, device=dev)
            self.view = self.whole[:, 4:4 + c]
            self.guards = lambda: (self.whole[:, :4], self.whole[:, 4 + c:])
        else:
            shift = 1 if layout == "off1" else 0
            self.whole = torch.full((numel + 2 * PAD,), GUARD, device=dev)
            self.view = self.whole[PAD + shift:PAD + shift + numel].view(shape)
            self.guards = lambda: (self.whole[:PAD + shift], self.whole[PAD + shift + numel:])
            assert self.view.data_ptr() % 16 == 4 * shift

    def intact(self):
        return all(bool((g == GUARD).all()) for g in self.guards())


def _launcher(case, data, dev):
    """-> (launch() -> output tensor, the _Out or None, the absmax slot or None)."""
    n, (oh, ow) = case.n, case.out_hw
    weight = data["weight"].to(dev)
    xs = [None if x is None else _place(x, s.layout, dev) for s, x in zip(case.srcs, data["x"])]
    slot = torch.zeros(n, device=dev, dtype=torch.int32) if case.absmax else None
    if case.op == "kbnet":
        def launch():
            with torch.no_grad():
                return ops.conv2d_kbnet(xs, weight, case.stride, case.slope)
        return launch, None, None
    out = _Out(case.out, (n, case.cout, oh, ow), dev)
    if case.op == "upconv2x":
        packed = ops.pack_upconv2x_weight(weight.permute(1, 0, 2, 3).contiguous() if case.transposed else weight, transposed=case.transposed)

        def launch():
            if slot is not None:
                slot.zero_()
            return ops.upconv2x(xs[0], packed, case.cout, out.view, case.slope, out_absmax=slot, transposed=case.transposed)
        return launch, out, slot
    packed = ops.pack_conv_weight(weight, case.stride)
    kinv = None if data["kinv"] is None else data["kinv"].to(dev)
    coords = None if data["coords"] is None else data["coords"].to(dev)
    proj = None if data["proj"] is None else data["proj"].to(dev)
    srcs = []
    for s, x in zip(case.srcs, xs):
        if s.kind == "tensor":
            srcs.append(ops.tensor_src(x))
        elif s.kind == "coords":
            srcs.append(ops.coords_src(kinv))
        elif s.kind == "xyz":
            srcs.append(ops.xyz_src(x, proj, kinv))
        else:
            srcs.append(ops.xyz_src(x, proj, None, coordinates=coords))

    def launch():
        if slot is not None:
            slot.zero_()
        return ops.conv2d(srcs, packed, n, case.cout, case.k, case.stride, case.h, case.w, out.view, resize=case.resize_from is not None,
                          negative_slope=case.slope, out_absmax=slot)
    return launch, out, slot


def _checked_route(case, want, what=""):
    route = ops.last_conv_route()
    OBSERVED.append((case.name, route))
    assert rc.matches(route, want), f"{case.name}{what}: the library ran {route}, the table says {want}"
    return route


def _run(case, dev, kenv):
    data = rc.make_inputs(case)
    for name, value in case.knobs:
        kenv.setenv(name, value)
    try:
        launch, out, slot = _launcher(case, data, dev)
        got = launch().clone()
        route = _checked_route(case, case.route)
        assert torch.equal(launch(), got), f"{case.name}: a second call changed the bits"
        # fp64 on the branches the device took, once kink_check has shown that any that differ sit at the kink
        u = rc.pre_activation(case, data)
        mask = None
        if case.slope is not None:
            mask = (got > 0).cpu()
            pgo.kink_check([mask], [u])
        ref = rc.activate(u, case.slope, mask)
        f, gate = rc.fraction(got, ref), rc.GATES[case.gate]
        print(f"\nroute {case.name}: {' '.join(f'{k}={v}' for k, v in route.items())} | fraction {f:.2e} (gate {gate:.0e}, {case.gate})", end="")
        assert f <= gate, (case.name, f, gate)
        assert rel_err(got, ref) < TIGHT
        if slot is not None:
            assert torch.equal(ops.slot_values(slot), got.abs().amax(dim=(1, 2, 3))), f"{case.name}: the out_absmax slot"
        # where the shape-only prediction is right: aligned, dense, tensor-only sources (and, for a Winograd shape, C % 8 == 0 per source)
        if (case.op != "upconv2x" and not case.knobs and not case.off1 and all(s.kind == "tensor" and s.layout == "dense" for s in case.srcs)):
            plan = ops.conv_plan(case.n, case.cout, case.cin, case.k, case.stride, case.h, case.w, case.resize_from is not None)
            if not (plan["kernel"] == "wino" and any(s.c % 8 for s in case.srcs)):
                assert plan["kernel"] == {"wino": "wino", "dma": "dma", "dma_syn": "dma", "igemm_pipe": "igemm"}[route["family"]], (case.name, plan)
        fam = case.route["family"]
        if case.force == "tiles":
            r = case.route
            for epi in ("0", "2"):
                kenv.setenv("KBN_EPI_LDS", epi)
                for mw, twb, mw_run in rc.forced_tiles(case):
                    kenv.setenv("KBN_FORCE_MW", str(mw))
                    kenv.setenv("KBN_FORCE_TWB", str(twb))
                    assert torch.equal(launch(), got), f"{case.name}: MW={mw} TWB={twb} epi={epi}"
                    want = dict(r, MW=mw_run, TWB=twb, epi_lds=rc.epi_in_effect(epi == "2", r["KS"], r["STRIDE"], r["CK"], r["NB"], mw_run, twb))
                    _checked_route(case, want, f" MW={mw} TWB={twb} epi={epi}")
                    FORCED.add((fam, mw_run, twb))
            for name in ("KBN_EPI_LDS", "KBN_FORCE_MW", "KBN_FORCE_TWB"):
                kenv.delenv(name)
        elif case.force == "rt":
            for rt, ct in rc.WINO_REGIONS:
                kenv.setenv("KBN_WINO_RT", str(rt))
                assert torch.equal(launch(), got), f"{case.name}: Winograd region of {rt} tile rows"
                _checked_route(case, dict(case.route, RT=rt, CT=ct), f" RT={rt}")
                FORCED.add((fam, rt, ct))
            kenv.delenv("KBN_WINO_RT")
        elif case.force == "twb":
            for twb in (1, 2):
                kenv.setenv("KBN_FORCE_TWB", str(twb))
                assert torch.equal(launch(), got), f"{case.name}: TWB={twb}"
                _checked_route(case, dict(case.route, TWB=twb), f" TWB={twb}")
                FORCED.add((fam, 0, twb))
            kenv.delenv("KBN_FORCE_TWB")
        if out is not None:
            assert out.intact(), f"{case.name}: a guard value around the output was overwritten"
    finally:
        for name, _ in case.knobs:
            kenv.delenv(name)


def _once(case, dev, kenv):
    if case.name not in _DONE:
        try:
            _run(case, dev, kenv)
            _DONE[case.name] = None
        except Exception as e:     # kept for the coverage test below, raised here
            _DONE[case.name] = e
            if isinstance(e, RuntimeError) and ("HIP error" in str(e) or "illegal memory access" in str(e)):
                pytest.exit(f"{case.name}: the device reported a fault ({e}); nothing more is launched on it", returncode=3)
            raise
    elif _DONE[case.name] is not None:
        raise _DONE[case.name]


ALIGNED = [c for c in rc.ALL_CASES if not c.off1]
OFF1 = [c for c in rc.ALL_CASES if c.off1]


@pytest.mark.parametrize("case", ALIGNED, ids=[c.name for c in ALIGNED])
def test_route_case(dev, kenv, case):
    _once(case, dev, kenv)


@pytest.mark.parametrize("case", OFF1, ids=[c.name for c in OFF1])
def test_route_case_base_off_by_one_float(dev, kenv, case):
    """A source or the output starts one float past a 16-byte boundary: the alignments the dispatch code tests for by itself
    (conv_dma.hip, conv_wino.hip, conv_up2x.hip), each landing on the kernel that takes any alignment."""
    _once(case, dev, kenv)


def test_failed_call_leaves_no_route(dev):
    x = torch.randn(1, 8, 6, 8, device=dev)
    packed = ops.pack_conv_weight(torch.randn(8, 8, 3, 3, device=dev), 1)
    out = torch.empty(1, 8, 6, 8, device=dev)
    ops.conv2d([ops.tensor_src(x)], packed, 1, 8, 3, 1, 6, 8, out)
    assert ops.last_conv_route()["family"] == "dma"
    with pytest.raises(kb._lib.KbnError):     # five sources: refused before anything is launched
        ops.conv2d([ops.tensor_src(x)] * 5, packed, 1, 8, 3, 1, 6, 8, out)
    assert ops.last_conv_route()["family"] == "none"


def test_every_required_route_was_observed(dev, kenv):
    """What the CPU test checks of the DECLARED routes, of the routes the library reported on this device."""
    for case in rc.ALL_CASES:
        try:
            _once(case, dev, kenv)
        except Exception:
            pass                  # that case's own test reports it; here only what was seen counts
    seen = [r for _, r in OBSERVED]
    missing = [want for want in rc.REQUIRED_ROUTES if not any(rc.matches(r, want) for r in seen)]
    assert not missing, missing
    assert set(rc.REQUIRED_FORCED) <= FORCED, set(rc.REQUIRED_FORCED) - FORCED
    print(f"\nobserved: {len(seen)} checked launches, {len({tuple(sorted(r.items())) for r in seen})} distinct routes; every one of the "
          f"{len(rc.REQUIRED_ROUTES)} required routes and {len(rc.REQUIRED_FORCED)} forced geometries was reported by the library", end="")
