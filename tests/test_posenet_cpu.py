"""CPU: the pose network's oracle against the vectors captured from the reference, the checkpoint plumbing of PoseNetModel, and
proof that the gates of tests/test_posenet_gpu.py can tell a wrong forward from a right one.

Gate (tests/posenet_oracle.py): |a - b| <= 1e-4 |b| + floor, floor = 1e-4 x RMS of the tensor for a layer, 1e-4 x 0.01 x RMS of the
6-channel map for `dof`.  A planted mistake must push `dof` PAST it (fraction > 1) on a golden case.
"""
import pytest
import torch

import kbnet_amd as kb
from conftest import load_golden

import posenet_oracle as po

GOLDENS = ("posenet_odd", "posenet_wide")
FILTERS = [8, 16, 16, 32, 32, 24, 40]


def _golden(name):
    g = load_golden(name)
    enc = {k: torch.as_tensor(v) for k, v in g["enc"].items()}
    dec = {k: torch.as_tensor(v) for k, v in g["dec"].items()}
    return g, enc, dec


@pytest.mark.parametrize("name", GOLDENS)
def test_oracle_equals_reference_bit_for_bit_in_fp32(name):
    g, enc, dec = _golden(name)
    o = po.forward(g["image0"], g["image1"], enc, dec)
    for i, layer in enumerate(o["layers"], 1):
        assert torch.equal(layer, g["ref32"][f"layer{i}"]), (name, i, float((layer - g["ref32"][f"layer{i}"]).abs().max()))
    for k in ("map", "dof", "pose"):
        assert torch.equal(o[k], g["ref32"][k]), (name, k)


@pytest.mark.parametrize("name", GOLDENS)
def test_oracle_fp64_matches_reference_fp64(name):
    g, enc, dec = _golden(name)
    o = po.forward(*po.to64(g["image0"], g["image1"], enc, dec))
    assert o["dof"].dtype == torch.float64
    for i, layer in enumerate(o["layers"], 1):
        ref = g["ref64"][f"layer{i}"]
        assert float((layer - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), (name, i)
    for k in ("map", "dof", "pose"):
        assert float((o[k] - g["ref64"][k]).abs().max()) <= 1e-12 * float(g["ref64"][k].abs().max()), (name, k)


def test_golden_maps_reach_the_sizes_they_are_there_for():
    odd, wide = load_golden("posenet_odd"), load_golden("posenet_wide")
    assert tuple(odd["image0"].shape) == (2, 3, 61, 77) and tuple(odd["ref32"]["layer7"].shape) == (2, 40, 1, 1)
    assert tuple(odd["ref32"]["layer6"].shape) == (2, 24, 1, 2)
    assert tuple(wide["image0"].shape) == (1, 3, 40, 136) and tuple(wide["ref32"]["layer7"].shape) == (1, 40, 1, 2)


def test_state_dict_keys_are_the_references():
    g, enc, dec = _golden("posenet_odd")
    m = kb.modules.PoseNetModel(device=torch.device("cpu"), n_filters=FILTERS)
    assert list(m.encoder.state_dict().keys()) == list(enc.keys())
    assert list(m.decoder.state_dict().keys()) == list(dec.keys())
    for k, v in m.encoder.state_dict().items():
        assert tuple(v.shape) == tuple(enc[k].shape) and v.dtype == enc[k].dtype, k
    m.encoder.load_state_dict(enc, strict=True)
    m.decoder.load_state_dict(dec, strict=True)
    full = kb.modules.PoseNetModel(device=torch.device("cpu"))
    assert [tuple(full.encoder.state_dict()[f"conv{i}.conv.weight"].shape) for i in range(1, 8)] == \
        [(16, 6, 7, 7), (32, 16, 5, 5), (64, 32, 3, 3), (128, 64, 3, 3), (256, 128, 3, 3), (256, 256, 3, 3), (256, 256, 3, 3)]
    assert tuple(full.decoder.state_dict()["conv.conv.weight"].shape) == (6, 256, 1, 1)
    assert kb.posenet.PoseNetModel is kb.modules.PoseNetModel
    assert len(full.parameters()) == 7 * 3 + 1


@pytest.mark.parametrize("prefix", [True, False])
def test_save_restore_round_trip(tmp_path, prefix):
    g, enc, dec = _golden("posenet_wide")
    a = kb.modules.PoseNetModel(device=torch.device("cpu"), n_filters=FILTERS)
    a.load_state_dicts(enc, dec)
    path = str(tmp_path / "pose_model-7.pth")
    a.save_model(path, step=7)
    ckpt = torch.load(path)
    assert set(ckpt) == {"train_step", "optimizer_state_dict", "encoder_state_dict", "decoder_state_dict"}
    assert all(k.startswith("module.") for k in list(ckpt["encoder_state_dict"]) + list(ckpt["decoder_state_dict"]))
    if not prefix:      # a checkpoint of bare modules
        ckpt["encoder_state_dict"] = po.strip(ckpt["encoder_state_dict"])
        ckpt["decoder_state_dict"] = po.strip(ckpt["decoder_state_dict"])
        torch.save(ckpt, path)
    b = kb.modules.PoseNetModel(device=torch.device("cpu"), n_filters=FILTERS)
    step, opt = b.restore_model(path)
    assert step == 7 and opt is None
    for got, want in ((b.encoder.state_dict(), enc), (b.decoder.state_dict(), dec)):
        assert list(got) == list(want)
        assert all(torch.equal(got[k], want[k]) for k in want)


def test_what_is_out_of_scope_raises():
    cpu = torch.device("cpu")
    for enc_type in ("resnet18", "resnet34"):
        with pytest.raises(kb._lib.KbnError, match="posenet"):
            kb.modules.PoseNetModel(encoder_type=enc_type, device=cpu)
    for act in ("elu", "sigmoid"):
        with pytest.raises(kb._lib.KbnError, match="leaky_relu"):
            kb.modules.PoseNetModel(activation_func=act, device=cpu, n_filters=FILTERS)
    for act in ("leaky_relu", "relu", "linear"):
        kb.modules.PoseNetModel(activation_func=act, device=cpu, n_filters=FILTERS)
    m = kb.modules.PoseNetModel(device=cpu, n_filters=FILTERS)
    with pytest.raises(kb._lib.KbnError, match="inference only"):
        m.train()
    assert m.data_parallel() is m
    m.eval()
    with pytest.raises(kb._lib.KbnError):          # no CPU path
        m.forward(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16))


def test_synthetic_weights_have_the_small_variances():
    enc, dec = kb.synthetic.make_posenet_weights(seed=4)
    for i in range(1, 8):
        var = enc[f"conv{i}.batch_norm.running_var"]
        assert int((var == 1e-3).sum()) == 2 and float(var[var != 1e-3].min()) >= 0.25 and float(var.max()) <= 1.75
        gamma = enc[f"conv{i}.batch_norm.weight"]
        assert 0.5 <= float(gamma.min()) and float(gamma.max()) <= 1.5
    again, _ = kb.synthetic.make_posenet_weights(seed=4)
    assert all(torch.equal(enc[k], again[k]) for k in enc)


# ---------------------------------------------------------------- power: the dof gate sees each of these mistakes
MISTAKES = {
    "images_swapped": dict(swap=True),
    "eps_dropped": dict(eps=0.0),
    "slope_0.10": dict(slope=0.10),
    "layer1_padding_2": dict(pad1=7 // 2 - 1),
    "0.01_omitted": dict(factor=1.0),
}


@pytest.mark.parametrize("mistake", list(MISTAKES))
def test_the_dof_gate_sees_a_planted_mistake(mistake):
    kwargs = dict(MISTAKES[mistake])
    swap = kwargs.pop("swap", False)
    fractions = {}
    for name in GOLDENS:
        g, enc, dec = _golden(name)
        i0, i1, e64, d64 = po.to64(g["image0"], g["image1"], enc, dec)
        right = po.forward(i0, i1, e64, d64)
        if "pad1" in kwargs and (g["image0"].shape[2] % 2 == 0 or g["image0"].shape[3] % 2 == 0):
            continue          # a narrower padding changes the map's size on an even side: such a forward fails on its shapes already
        wrong = po.forward(i1, i0, e64, d64, **kwargs) if swap else po.forward(i0, i1, e64, d64, **kwargs)
        assert float((right["dof"] - g["ref64"]["dof"]).abs().max()) <= 1e-12
        fractions[name] = po.gate_fraction(wrong["dof"], right["dof"], po.dof_floor(right["map"]))
    print(mistake, " ".join(f"{k} {v:.3g} x the gate" for k, v in fractions.items()))
    assert fractions and max(fractions.values()) > 1.0, (mistake, fractions)
