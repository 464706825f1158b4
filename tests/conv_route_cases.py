"""The fp32 conv family's route table: which kernel instantiation every case must run, written by hand from the dispatch code
(csrc/conv_igemm.hip conv2d_launch, conv_wino.hip conv_wino_launch, conv_dma.hip conv_dma_launch, conv_up2x.hip), never asked of
the library.  Plain data plus the CPU helpers both test files share (inputs, fp64 references, an fp32 Winograd evaluation, the
gates).  Imports without a GPU; tests/test_conv_route_cases_cpu.py checks the table, tests/test_conv_routes_gpu.py runs it.

The eligibility rules the expected routes are read from:
  conv2d, 3x3 stride 1, KBN_NO_WINO unset -> Winograd when cin >= 32, cin % 16 == 0, cout >= 32, no resize, W % 4 == 0, every
      source a tensor of C % 8 == 0 channels on a 16-byte base with batch stride % 4 == 0, and the output on an 8-byte base;
  otherwise LDS-DMA when no resize, W % 4 == 0 and every tensor source on a 16-byte base with batch stride % 4 == 0; its SYN
      instantiation when a source is computed (COORDS / XYZ) or a source other than the last ends off a CK boundary;
  otherwise the generic kernel, pipelined when maxpos(k, stride, MW) * CK <= 48.
  CK = 16 for 1x1, 4 for 3x3 with cin <= 16 or stride 2, else 8.  NB in 1..4 minimises the padded 16-filter blocks (ties: the
  larger): 1..16 filters -> 1, ..32 -> 2, ..48 -> 3, ..64 -> 4, 65..80 -> 1, 130 -> 3.  The plan's largest MW is 8 for NB 2, else 4.
  The LDS epilogue is asked for when cin * k * k <= 128 (KBN_EPI_LDS unset), always / never under KBN_EPI_LDS=2 / 0, and given
  up by an instantiation whose stage buffers are smaller than the epilogue's scratch (dma_stage_bytes below).
  upconv2x (exact 2x): NB as above, MW 2 for NB >= 3 else 4.  With cin % 16 == 0, W % 4 == 0, a 16-byte base and batch stride
  % 4 == 0 the 9-product kernel when cout <= 16 or cout % 32 == 0 (and neither KBN_NO_UP2X9 nor KBN_NO_UP2X3 nor a plain
  transposed conv), else the DMA kernel with 16-byte granules in its 3-product form (4-phase under KBN_NO_UP2X3 / plain).  Rows or
  a base that are not 16-byte aligned: the DMA kernel with dword granules when NB >= 3 and cin % 16 == 0 (half-size tiles while
  ceil(W/16) * ceil(H/8) * n * nTilesN * 2 <= 512).  Everything else: the general kernel (NB >= 3: MW 1 under the same count).
"""
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch
import torch.nn.functional as F


# ------------------------------------------------------------------------------------------------ the table's types
@dataclass(frozen=True)
class Src:
    c: int
    kind: str = "tensor"      # tensor | coords (K^-1 [x y 1]^T from kinv) | xyz (coords * act(proj . depth), kinv) | xyz_dense (dense coordinates)
    layout: str = "dense"     # dense | slice (channels 3 .. 3 + c of a tensor with 5 more: its own batch stride) | off1 (base + one float)
    cd: int = 0               # xyz: channels of the depth features


@dataclass(frozen=True)
class Case:
    name: str
    op: str                   # conv2d | kbnet | upconv2x
    srcs: Tuple[Src, ...]
    cout: int
    k: int
    stride: int
    n: int
    h: int                    # input size (upconv2x: the low-resolution source; resize: the size the conv sees)
    w: int
    route: dict               # the expected route: a subset of ops.last_conv_route()'s fields
    slope: Optional[float] = 0.2
    out: str = "dense"        # dense (inside a guarded flat buffer) | slice (channels of a wider guarded tensor) | off1
    knobs: Tuple[Tuple[str, str], ...] = ()
    resize_from: Optional[Tuple[int, int]] = None    # conv2d resize=True: the source's size
    absmax: bool = False      # pass an out_absmax slot
    force: Optional[str] = None    # "tiles": every KBN_FORCE_MW x KBN_FORCE_TWB (x both epilogues), "rt": every KBN_WINO_RT, "twb": KBN_FORCE_TWB 1, 2
    transposed: bool = False  # upconv2x: the plain ConvTranspose2d form (kbn_deconv2x_forward)
    gate: str = "direct"      # which gate the case answers to

    @property
    def cin(self):
        return sum(s.c for s in self.srcs)

    @property
    def off1(self):
        return self.out == "off1" or any(s.layout == "off1" for s in self.srcs)

    @property
    def out_hw(self):
        if self.op == "upconv2x":
            return 2 * self.h, 2 * self.w
        return -(-self.h // self.stride), -(-self.w // self.stride)


def T(*cs, layout="dense"):
    return tuple(Src(c, layout=layout) for c in cs)


def R(family, **kw):
    return dict(family=family, **kw)


def _dma(k, s, ck, nb, epi, syn=False):
    return R("dma_syn" if syn else "dma", KS=k, STRIDE=s, CK=ck, NB=nb, epi_lds=epi)


def _gen(k, s, ck, nb):
    return R("igemm_pipe", KS=k, STRIDE=s, CK=ck, NB=nb, epi_lds=0)


WINO = R("wino", KS=3, STRIDE=1, CK=8, NB=4)
WINO_REGIONS = ((4, 16), (8, 8), (2, 32), (6, 10), (5, 12), (3, 20), (7, 8), (10, 6))     # conv_wino.hip kRegions (RT, CT)
NO_WINO = (("KBN_NO_WINO", "1"),)

CASES = [
    # ---- conv2d, LDS-DMA without SYN: every (k, stride), CK 4 / 8 / 16, NB 1..4 and padded filter counts, both epilogues ----
    Case("dma_k3s1_ck4_nb1_pad10", "conv2d", T(8), 10, 3, 1, 2, 33, 72, _dma(3, 1, 4, 1, 1), force="tiles", absmax=True),
    Case("dma_k3s1_ck4_nb3", "conv2d", T(3), 48, 3, 1, 2, 19, 72, _dma(3, 1, 4, 3, 1), out="slice"),
    Case("dma_k3s1_ck8_nb2", "conv2d", T(24), 32, 3, 1, 2, 19, 72, _dma(3, 1, 8, 2, 0), slope=None),
    Case("dma_k3s1_ck8_nb3_pad130", "conv2d", T(24), 130, 3, 1, 1, 19, 72, _dma(3, 1, 8, 3, 0)),
    Case("dma_k3s1_ck8_nb4_nowino", "conv2d", T(64), 64, 3, 1, 2, 33, 72, _dma(3, 1, 8, 4, 0), knobs=NO_WINO, force="tiles"),
    Case("dma_k3s1_epi_given_up", "conv2d", T(12), 32, 3, 1, 2, 19, 72, dict(_dma(3, 1, 4, 2, 0), MW=8, TWB=4),
         knobs=(("KBN_FORCE_MW", "8"), ("KBN_FORCE_TWB", "4"))),     # asked for (12 * 9 <= 128), 32 256 B of stages < 33 024 B of scratch
    Case("dma_k3s1_epi_kept", "conv2d", T(12), 32, 3, 1, 2, 19, 72, dict(_dma(3, 1, 4, 2, 1), MW=8, TWB=1),
         knobs=(("KBN_FORCE_MW", "8"), ("KBN_FORCE_TWB", "1"))),
    Case("dma_k3s2_w140_scalar_stores", "conv2d", T(48), 48, 3, 2, 2, 38, 140, _dma(3, 2, 4, 3, 0), absmax=True),   # 140 -> 70: W % 4 == 0, out W not
    Case("dma_k3s2_w136", "conv2d", T(48), 48, 3, 2, 2, 38, 136, _dma(3, 2, 4, 3, 0)),
    Case("dma_k3s2_nb2_forced", "conv2d", T(19), 32, 3, 2, 2, 65, 140, _dma(3, 2, 4, 2, 0), force="tiles"),
    Case("dma_k3s2_ck4_narrow", "conv2d", T(8), 16, 3, 2, 3, 19, 72, _dma(3, 2, 4, 1, 1)),
    Case("dma_k1s1_nb4", "conv2d", T(16), 64, 1, 1, 2, 33, 72, _dma(1, 1, 16, 4, 1), force="tiles"),
    Case("dma_k1s1_nb1_one_filter", "conv2d", T(16), 1, 1, 1, 2, 19, 72, _dma(1, 1, 16, 1, 1), slope=None, out="slice"),
    Case("dma_k1s2_nb3", "conv2d", T(51), 48, 1, 2, 2, 65, 140, _dma(1, 2, 16, 3, 1), force="tiles", absmax=True),
    Case("dma_k1s2_two_sources_on_chunks", "conv2d", T(32, 48), 96, 1, 2, 2, 38, 136, _dma(1, 2, 16, 3, 1)),
    Case("dma_k3s1_slice_source", "conv2d", (Src(16), Src(8, layout="slice")), 16, 3, 1, 3, 19, 72, _dma(3, 1, 8, 1, 0)),
    # ---- conv2d, LDS-DMA SYN: chunks that straddle sources, computed sources ----
    Case("syn_k3s1_3_5_7", "conv2d", T(3, 5, 7), 70, 3, 1, 2, 33, 72, _dma(3, 1, 4, 1, 0, syn=True), force="tiles"),
    Case("syn_k1s2_24_40", "conv2d", T(24, 40), 48, 1, 2, 2, 65, 140, _dma(1, 2, 16, 3, 1, syn=True), force="tiles"),
    Case("syn_k1s1_24_40", "conv2d", T(24, 40), 20, 1, 1, 2, 19, 72, _dma(1, 1, 16, 2, 1, syn=True)),
    Case("syn_k3s2_depth_coords", "conv2d", (Src(16), Src(3, "coords")), 16, 3, 2, 2, 65, 140, _dma(3, 2, 4, 1, 0, syn=True),
         force="tiles", absmax=True),      # conv_depth of a KB block: cat[depth, K^-1 [x y 1]^T]
    Case("syn_k1s2_image_xyz_fused", "conv2d", (Src(48), Src(3, "xyz", cd=16), Src(48)), 96, 1, 2, 2, 65, 140,
         _dma(1, 2, 16, 3, 1, syn=True), force="tiles"),       # conv_fused: cat[image, coords * act(proj . depth), fused]
    Case("syn_k1s2_image_xyz_dense_coords", "conv2d", (Src(16), Src(3, "xyz_dense", cd=8)), 48, 1, 2, 3, 19, 72,
         _dma(1, 2, 16, 3, 1, syn=True)),
    Case("syn_k3s1_coords_first_level", "conv2d", (Src(8, layout="slice"), Src(3, "coords")), 16, 3, 1, 2, 19, 72,
         _dma(3, 1, 4, 1, 1, syn=True)),
    # ---- conv2d, Winograd ----
    Case("wino_one_source", "conv2d", T(64), 128, 3, 1, 2, 44, 72, WINO, force="rt", gate="wino", absmax=True),
    Case("wino_two_sources_24_40", "conv2d", T(24, 40), 64, 3, 1, 2, 19, 72, WINO, gate="wino"),    # both C % 8 == 0: no decline
    Case("wino_slice_source", "conv2d", (Src(32), Src(16, layout="slice")), 48, 3, 1, 2, 33, 40, WINO, gate="wino", out="slice"),
    Case("wino_cout130_n3", "conv2d", T(32), 130, 3, 1, 3, 7, 40, WINO, gate="wino", slope=None),
    Case("wino_h1", "conv2d", T(80), 64, 3, 1, 1, 1, 8, WINO, gate="wino"),
    Case("wino_declines_width", "conv2d", T(64), 64, 3, 1, 2, 19, 71, _gen(3, 1, 8, 4)),
    Case("wino_declines_chunk_20_44", "conv2d", T(20, 44), 64, 3, 1, 2, 19, 72, _dma(3, 1, 8, 4, 0, syn=True)),   # 20 % 8 != 0
    Case("wino_declines_knob", "conv2d", T(64), 64, 3, 1, 2, 19, 72, _dma(3, 1, 8, 4, 0), knobs=NO_WINO),
    # ---- conv2d, generic kernel ----
    Case("gen_k3s1_odd_width", "conv2d", T(19), 16, 3, 1, 2, 19, 71, _gen(3, 1, 8, 1), absmax=True),
    Case("gen_k3s2_odd_width", "conv2d", T(3, 5, 7), 70, 3, 2, 2, 33, 71, _gen(3, 2, 4, 1), out="slice"),
    Case("gen_k1s2_odd_width", "conv2d", T(99), 96, 1, 2, 1, 23, 31, _gen(1, 2, 16, 3)),
    Case("gen_k1s1_coords_odd_width", "conv2d", (Src(8), Src(3, "coords")), 20, 1, 1, 2, 19, 71, _gen(1, 1, 16, 2)),
    Case("gen_resize_free", "conv2d", T(24), 16, 3, 1, 2, 5, 7, _gen(3, 1, 8, 1), resize_from=(3, 4)),
    Case("gen_resize_2h_minus_1", "conv2d", T(24), 16, 3, 1, 2, 37, 71, _gen(3, 1, 8, 1), resize_from=(19, 36)),
    Case("gen_resize_aligned_width", "conv2d", T(24), 16, 3, 1, 2, 10, 16, _gen(3, 1, 8, 1), resize_from=(5, 7)),   # W % 4 == 0: resize alone declines the DMA
    # ---- upconv2x (the fp32 forms: what UpConv2d runs with split_up = False) ----
    Case("up9_nb2", "upconv2x", T(64), 64, 3, 1, 2, 19, 40, R("up2x9", NB=2, MW=2, form=9, granule=16, half=0), force="twb", gate="wino",
         absmax=True),
    Case("up9_nb1_narrow", "upconv2x", T(64), 12, 3, 1, 2, 20, 36, R("up2x9", NB=1, MW=4, form=9, granule=16, half=0), force="twb",
         gate="wino"),
    Case("up3_nb3", "upconv2x", T(32), 48, 3, 1, 2, 19, 40, R("up2x_dma", NB=3, MW=2, form=3, granule=16, half=0), force="twb", gate="wino"),
    Case("up3_nb4_by_knob", "upconv2x", T(64), 64, 3, 1, 2, 19, 40, R("up2x_dma", NB=4, MW=2, form=3, granule=16, half=0),
         knobs=(("KBN_NO_UP2X9", "1"),), force="twb", gate="wino"),
    Case("up4_nb4_by_knob", "upconv2x", T(64), 64, 3, 1, 2, 19, 40, R("up2x_dma", NB=4, MW=2, form=4, granule=16, half=0),
         knobs=(("KBN_NO_UP2X3", "1"),), force="twb"),
    Case("up3_nb2", "upconv2x", T(16), 20, 3, 1, 2, 19, 40, R("up2x_dma", NB=2, MW=4, form=3, granule=16, half=0), force="twb", gate="wino",
         out="slice"),
    Case("up3_nb1_by_knob", "upconv2x", T(32), 16, 3, 1, 2, 19, 40, R("up2x_dma", NB=1, MW=4, form=3, granule=16, half=0),
         knobs=(("KBN_NO_UP2X9", "1"),), force="twb", gate="wino", slope=None),
    Case("up_dword_64_64_11x38", "upconv2x", T(64), 64, 3, 1, 2, 11, 38, R("up2x_dma", NB=4, MW=1, TWB=1, form=3, granule=4, half=1),
         gate="wino", absmax=True),
    Case("up_dword_32_48_11x38", "upconv2x", T(32), 48, 3, 1, 2, 11, 38, R("up2x_dma", NB=3, MW=1, TWB=1, form=3, granule=4, half=1), gate="wino"),
    Case("up_dword_full_tile", "upconv2x", T(16), 130, 3, 1, 3, 40, 82, R("up2x_dma", NB=3, MW=2, TWB=1, form=3, granule=4, half=0),
         gate="wino"),        # 6 x 5 x 3 x 3 x 2 = 540 tiles > 512
    Case("up_dword_four_phase", "upconv2x", T(32), 48, 3, 1, 2, 11, 38, R("up2x_dma", NB=3, MW=1, TWB=1, form=4, granule=4, half=1),
         knobs=(("KBN_NO_UP2X3", "1"),)),
    Case("up_gen_nb1", "upconv2x", T(24), 16, 3, 1, 2, 19, 40, R("up2x", NB=1, MW=4, form=4, granule=0, half=0), force="twb"),
    Case("up_gen_nb2", "upconv2x", T(24), 32, 3, 1, 2, 19, 40, R("up2x", NB=2, MW=4, form=4, granule=0, half=0), force="twb"),
    Case("up_gen_nb3_half", "upconv2x", T(20), 48, 3, 1, 2, 19, 40, R("up2x", NB=3, MW=1, form=4, granule=0, half=1), force="twb",
         out="slice"),
    Case("up_gen_nb4_20_52_half", "upconv2x", T(20), 52, 3, 1, 2, 19, 40, R("up2x", NB=4, MW=1, form=4, granule=0, half=1), force="twb",
         absmax=True),
    Case("up_gen_nb3_full_tile", "upconv2x", T(20), 130, 3, 1, 3, 40, 82, R("up2x", NB=3, MW=2, form=4, granule=0, half=0)),   # 540 tiles > 512
    Case("up_gen_narrow_odd_rows", "upconv2x", T(64), 12, 3, 1, 2, 11, 38, R("up2x", NB=1, MW=4, form=4, granule=0, half=0)),   # NB < 3: no dword DMA
    Case("up_plain_transposed", "upconv2x", T(32), 24, 3, 1, 2, 19, 40, R("up2x_dma", NB=2, MW=4, form=4, granule=16, half=0),
         transposed=True, force="twb"),
    Case("up_plain_transposed_general", "upconv2x", T(24), 16, 3, 1, 2, 5, 7, R("up2x", NB=1, MW=4, form=4, granule=0, half=0), transposed=True),
    # ---- a base off by one float: only the alignments the dispatch code tests for (conv_dma.hip, conv_wino.hip, conv_up2x.hip) ----
    Case("off1_source_wino_shape", "conv2d", T(64, layout="off1"), 64, 3, 1, 2, 19, 72, _gen(3, 1, 8, 4)),     # generic, not DMA
    Case("off1_source_dma_shape", "conv2d", (Src(16), Src(8, layout="off1")), 16, 1, 2, 2, 19, 72, _gen(1, 2, 16, 1)),
    Case("off1_output_dma_shape", "conv2d", T(8), 10, 3, 1, 2, 19, 72, _dma(3, 1, 4, 1, 1), out="off1", absmax=True),   # sources decide; scalar stores
    Case("off1_output_wino_shape", "conv2d", T(64), 64, 3, 1, 2, 19, 72, _dma(3, 1, 8, 4, 0), out="off1"),      # the float2 epilogue declines
    Case("off1_up_dword_64_64_12x20", "upconv2x", T(64, layout="off1"), 64, 3, 1, 2, 12, 20,
         R("up2x_dma", NB=4, MW=1, TWB=1, form=3, granule=4, half=1), gate="wino"),
    Case("off1_up_dword_32_48_12x20", "upconv2x", T(32, layout="off1"), 48, 3, 1, 2, 12, 20,
         R("up2x_dma", NB=3, MW=1, TWB=1, form=3, granule=4, half=1), gate="wino", out="off1"),
    Case("off1_up_general_nb2", "upconv2x", T(16, layout="off1"), 20, 3, 1, 2, 12, 20, R("up2x", NB=2, MW=4, form=4, granule=0, half=0)),
]

# ---- ops.conv2d_kbnet: the training forward's convs.  One, two and three inputs, all four (k, stride); the family per
# (channels, inputs) in the order KBNET_KS.  (3, 5, 7) and (70, 3, 19): every source but the first starts off a chunk boundary
# (3 and 70 are no multiple of 4, 8 or 16) -> SYN from two inputs on.  (16, 32, 16): chunk-aligned whatever CK; 48 and 64 input
# channels in sources of C % 8 == 0 with 40 filters -> Winograd at (3, 1).
KBNET_KS = ((3, 1), (3, 2), (1, 1), (1, 2))
KBNET_FRAMES = ((2, 20, 72), (3, 19, 136))
KBNET_CHANNELS = {
    (3, 5, 7): (70, {1: ("dma",) * 4, 2: ("dma_syn",) * 4, 3: ("dma_syn",) * 4}),
    (16, 32, 16): (40, {1: ("dma",) * 4, 2: ("wino", "dma", "dma", "dma"), 3: ("wino", "dma", "dma", "dma")}),
    (70, 3, 19): (10, {1: ("dma",) * 4, 2: ("dma_syn",) * 4, 3: ("dma_syn",) * 4}),
}


def kbnet_cases():
    out = []
    for channels, (cout, families) in KBNET_CHANNELS.items():
        for frame in KBNET_FRAMES:
            for count in (1, 2, 3):
                for (k, s), fam in zip(KBNET_KS, families[count]):
                    cin = sum(channels[:count])
                    route = dict(WINO) if fam == "wino" else R(fam, KS=k, STRIDE=s, CK=16 if k == 1 else (4 if cin <= 16 or s == 2 else 8))
                    out.append(Case(f"kbnet_{'_'.join(map(str, channels[:count]))}_k{k}s{s}_{frame[0]}x{frame[1]}x{frame[2]}", "kbnet",
                                    T(*channels[:count]), cout, k, s, *frame, route, slope=(0.2, 0.0, None)[count - 1],
                                    gate="wino" if fam == "wino" else "direct"))
    # a channel-slice input (the encoder's skip buffers): Winograd reads it at its own batch stride
    out.append(Case("kbnet_slice_input_k3s1", "kbnet", (Src(32), Src(16, layout="slice")), 40, 3, 1, 2, 20, 72, dict(WINO), gate="wino"))
    out.append(Case("kbnet_slice_input_k1s2", "kbnet", (Src(5, layout="slice"), Src(16)), 40, 1, 2, 3, 19, 136,
                    R("dma_syn", KS=1, STRIDE=2, CK=16)))
    return out


ALL_CASES = CASES + kbnet_cases()
BY_NAME = {c.name: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)

# What the table must reach at least once: (field, value) pairs that one declared route holds together.
REQUIRED_ROUTES = (
    [dict(family="dma", KS=k, STRIDE=s) for k, s in KBNET_KS]
    + [dict(family="dma", CK=ck) for ck in (4, 8, 16)] + [dict(family="dma", KS=3, STRIDE=2, CK=4)]
    + [dict(family="dma", NB=nb) for nb in (1, 2, 3, 4)]
    + [dict(family="dma", epi_lds=e) for e in (0, 1)]
    + [dict(family="dma_syn", KS=k, STRIDE=s) for k, s in KBNET_KS]
    + [dict(family="wino")] + [dict(family="igemm_pipe", KS=k, STRIDE=s) for k, s in KBNET_KS]
    + [dict(family="up2x9", NB=1), dict(family="up2x9", NB=2)]
    + [dict(family="up2x_dma", form=3, granule=16), dict(family="up2x_dma", form=4, granule=16)]
    + [dict(family="up2x_dma", granule=16, NB=nb) for nb in (1, 2, 3, 4)]
    + [dict(family="up2x_dma", granule=4, half=1, NB=3), dict(family="up2x_dma", granule=4, half=1, NB=4),
       dict(family="up2x_dma", granule=4, half=0), dict(family="up2x_dma", granule=4, form=4)]
    + [dict(family="up2x", NB=nb) for nb in (1, 2, 3, 4)] + [dict(family="up2x", half=0, NB=3), dict(family="up2x", half=1, NB=3)]
)
# Forced geometry that the GPU log must show as observed (the forced loops report what the route said)
REQUIRED_FORCED = ([("dma", mw, twb) for mw in (1, 2, 4, 8) for twb in (1, 2, 4)] + [("dma_syn", mw, twb) for mw in (1, 2, 4) for twb in (1, 2, 4)]
                   + [("wino", rt, ct) for rt, ct in WINO_REGIONS]
                   + [(fam, 0, twb) for fam in ("up2x9", "up2x_dma", "up2x") for twb in (1, 2)])
# What no launch can reach, read from the dispatch code (DESIGN 8w says why): the generic kernel without its pipeline needs
# maxpos * CK > 48, i.e. 3x3 stride 2 with CK 8 and MW 8, and make_plan gives every stride-2 3x3 conv CK 4; the 16-byte-granule
# up-conv with half-size tiles is a candidate of the tuner alone (tuning off: candidate = TWB - 1, the half bit clear).
UNREACHABLE = ("igemm (generic kernel, not pipelined)", "dma / dma_syn / igemm_pipe with KS 3, STRIDE 2, CK 8",
               "up2x_dma with granule 16 and half-size tiles while tuning is off")


def matches(route, want):
    return all(route.get(k) == v for k, v in want.items())


# ------------------------------------------------------------------------------------------------ forced geometry
def plan_nb(cout):
    """make_plan's NB: 1..4 sixteen-filter blocks a workgroup, the fewest padded blocks, ties to the larger."""
    blocks = -(-cout // 16)
    return min(range(1, 5), key=lambda nb: (-(-blocks // nb) * nb, -nb))


def plan_mw(nb):
    return 8 if nb == 2 else 4


def conv_family(cin, cout, k, stride, w, sources=None):
    """The family an fp32 conv of dense, aligned tensor sources runs (the rules of the module's docstring)."""
    sources = sources or (cin,)
    if k == 3 and stride == 1 and cin >= 32 and cin % 16 == 0 and cout >= 32 and w % 4 == 0 and all(c % 8 == 0 for c in sources):
        return "wino"
    return "dma" if w % 4 == 0 else "igemm_pipe"


def up_route(cin, cout, w, plain=False):
    """(family, DMA granule) of an exact-2x up-conv of a dense, aligned source on the fp32 kernels."""
    if cin % 16 == 0 and w % 4 == 0:
        return ("up2x9", 16) if (cout <= 16 or cout % 32 == 0) and not plain else ("up2x_dma", 16)
    if plan_nb(cout) >= 3 and cin % 16 == 0:
        return ("up2x_dma", 4)
    return ("up2x", 0)


def forced_tiles(case):
    """(KBN_FORCE_MW, KBN_FORCE_TWB, the MW the route must report): a forced MW above the plan's runs the plan's."""
    cap = plan_mw(case.route["NB"])
    return [(mw, twb, min(mw, cap)) for mw in (1, 2, 4, 8) for twb in (1, 2, 4)]


def tile_shapes(case):
    """Output-pixel tile shapes (rows, columns) the case's forced loop runs."""
    if case.force == "tiles":
        return sorted({(4 * mw // twb, 16 * twb) for _, twb, mw in forced_tiles(case)})
    if case.force == "rt":
        return [(2 * rt, 2 * ct) for rt, ct in WINO_REGIONS]
    if case.force == "twb":      # low-resolution tiles of 4 * MW m-blocks (general kernel with half tiles: 4)
        mws = {case.route["MW"]}
        return sorted({(4 * mw // twb, 16 * twb) for mw in mws for twb in (1, 2)})
    return []


def tiled_extent(case):
    """The extent the forced tiles cut: output pixels; the up-convs tile their low-resolution source."""
    return (case.h, case.w) if case.op == "upconv2x" else case.out_hw


def dma_stage_bytes(k, stride, ck, nb, mw, twb):
    """conv_dma_impl.h DmaGeom + dma_variant: bytes of the two stage buffers of an instantiation."""
    th, tw = 4 * mw // twb, 16 * twb
    rows = (2 * th + 1 if stride == 2 else th + 2) if k == 3 else th
    cols = (2 * tw + 4 if stride == 2 else tw + 8) if k == 3 else stride * tw
    plane = (rows * cols + 15) // 32 * 32 + 16
    return 2 * 4 * (ck * plane + ck * k * k * nb * 16)


def epi_in_effect(asked, k, stride, ck, nb, mw, twb):
    """The LDS epilogue needs 16 * (64 MW + 4) floats of the idle stage buffers."""
    return int(bool(asked) and dma_stage_bytes(k, stride, ck, nb, mw, twb) >= 4 * 16 * (64 * mw + 4))


# ------------------------------------------------------------------------------------------------ inputs and references
def case_seed(case):
    return 1000 + sorted(BY_NAME).index(case.name)


def make_inputs(case):
    """fp32 CPU inputs: per source its tensor ("depth" features for an xyz source), the weight, and for computed sources kinv /
    the dense coordinates / the projection weight."""
    g = torch.Generator().manual_seed(case_seed(case))
    h, w = case.resize_from or (case.h, case.w)
    data = {"x": [], "kinv": None, "coords": None, "proj": None}
    for s in case.srcs:
        if s.kind == "tensor":
            data["x"].append(torch.randn(case.n, s.c, h, w, generator=g))
        elif s.kind == "coords":
            data["x"].append(None)
        else:
            data["x"].append(torch.randn(case.n, s.cd, h, w, generator=g))
            data["proj"] = torch.randn(1, s.cd, 1, 1, generator=g) / math.sqrt(s.cd)
    if any(s.kind != "tensor" for s in case.srcs):
        f = torch.rand(case.n, generator=g) * 40 + 60
        k = torch.zeros(case.n, 3, 3)
        k[:, 0, 0], k[:, 1, 1], k[:, 0, 2], k[:, 1, 2], k[:, 2, 2] = f, f * 1.1, w / 2.0, h / 2.0, 1.0
        # column-major on purpose (what torch.linalg.inv returns): ops.coords_src / ops.xyz_src once read such a kinv as its transpose
        data["kinv"] = torch.linalg.inv(k.double()).float().transpose(1, 2).contiguous().transpose(1, 2)
        assert not data["kinv"].is_contiguous()
        data["coords"] = coordinates(data["kinv"].double(), h, w).float()       # what a caller hands over as dense coordinates
    taps = case.k * case.k
    fan = case.cin * (2.25 if case.transposed else taps)
    data["weight"] = torch.randn(case.cout, case.cin, case.k, case.k, generator=g) / math.sqrt(fan)
    return data


def coordinates(kinv, h, w):
    ys, xs = torch.meshgrid(torch.arange(h, dtype=kinv.dtype), torch.arange(w, dtype=kinv.dtype), indexing="ij")
    pix = torch.stack([xs, ys, torch.ones_like(xs)], 0).reshape(3, -1)
    return (kinv @ pix).reshape(-1, 3, h, w)


def concat_input(case, data, dtype=torch.float64):
    """cat of the sources as the conv sees them, in `dtype` (fp64: the reference's input)."""
    h, w = case.resize_from or (case.h, case.w)
    parts = []
    for s, x in zip(case.srcs, data["x"]):
        if s.kind == "tensor":
            parts.append(x.to(dtype))
        else:
            c = data["coords"].to(dtype) if s.kind == "xyz_dense" else coordinates(data["kinv"].to(dtype), h, w)
            if s.kind == "coords":
                parts.append(c)
            else:
                z = F.conv2d(x.to(dtype), data["proj"].to(dtype))
                if case.slope is not None:
                    z = torch.where(z > 0, z, case.slope * z)
                parts.append(c * z)
    x = torch.cat(parts, 1)
    if case.resize_from:
        x = F.interpolate(x, size=(case.h, case.w), mode="nearest")
    return x


def pre_activation(case, data, dtype=torch.float64, x=None):
    """The conv before its activation, by torch on the CPU in `dtype`."""
    x = concat_input(case, data, dtype) if x is None else x
    wt = data["weight"].to(dtype)
    if case.op == "upconv2x":
        if case.transposed:
            return F.conv_transpose2d(x, wt.permute(1, 0, 2, 3), stride=2, padding=1, output_padding=1)
        return F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), wt, padding=1)
    return F.conv2d(x, wt, stride=case.stride, padding=case.k // 2)


def activate(u, slope, mask=None):
    return u if slope is None else torch.where(u > 0 if mask is None else mask, u, slope * u)


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


def fraction(a, b):
    """max |a - b| / (|b| + rms(b)) (posenet_grad_oracle.fraction's definition; here so that the CPU test needs nothing else)."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(((a - b).abs() / (b.abs() + rms(b))).max())


# ---- fp32 Winograd F(2x2,3x3) on the CPU (moved here from tests/analysis/winograd_error.py, which imports it back)
BT_ = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float32)
G_ = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float32)
AT_ = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float32)


def winograd_conv3x3(x, w, full=False):
    """`full`: also the rows / columns the even padding adds (what the last odd row's tile computes below the image)."""
    n, c, h, wd = x.shape
    BT, G, AT = BT_.to(x.dtype), G_.to(x.dtype), AT_.to(x.dtype)
    he, we = h + (h & 1), wd + (wd & 1)
    xp = F.pad(x, (1, 1 + we - wd, 1, 1 + he - h))
    d = xp.unfold(2, 4, 2).unfold(3, 4, 2)                       # n c th tw 4 4
    v = torch.einsum("ij,nctujk,lk->nctuil", BT, d, BT)          # B^T d B
    u = torch.einsum("ij,ocjk,lk->ocil", G, w, G)                # G g G^T
    m = torch.einsum("ocil,nctuil->notuil", u, v)
    y = torch.einsum("ij,notujk,lk->notuil", AT, m, AT)          # n o th tw 2 2
    th, tw = y.shape[2], y.shape[3]
    y = y.permute(0, 1, 2, 4, 3, 5).reshape(n, w.shape[0], 2 * th, 2 * tw)
    return y if full else y[:, :, :h, :wd]


# ------------------------------------------------------------------------------------------------ the gates
# Measured by tests/test_conv_route_cases_cpu.py (it prints the figures and asserts these constants against them): the worst
# fraction over the table of torch's own fp32 CPU conv (direct) and of the fp32 Winograd evaluation above against fp64,
# times 3, rounded up to one digit, at most 1e-5 (the bar the conv node's forward holds).
# The up-convs' 3- and 9-product forms answer to the Winograd gate: they are the same kind of algorithm (products of input
# differences with pre-summed weights, recombined by additions), the 4-phase form and the transposed conv to the direct one.
GATE_CEILING = 1e-5
DIRECT_GATE = 6e-6
WINO_GATE = 7e-6
GATES = {"direct": DIRECT_GATE, "wino": WINO_GATE}


def gate_from(worst):
    """3 x worst, rounded up to one significant digit, at most GATE_CEILING."""
    v = 3.0 * worst
    e = math.floor(math.log10(v))
    return min(GATE_CEILING, math.ceil(v / 10 ** e - 1e-9) * 10 ** e)
