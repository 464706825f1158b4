"""CPU: the ResNet pose networks' oracle against the vectors captured from the reference, the checkpoint plumbing of
ResNetPoseNetModel and modules.load_pose_model, and proof that the gate of tests/test_resnet_pose_gpu.py can tell a wrong forward
from a right one.

Gate (tests/posenet_oracle.py): |a - b| <= 1e-4 |b| + floor, floor = 1e-4 x RMS of the tensor for a layer, 1e-4 x 0.01 x RMS of the
6-channel map for `dof`.  A planted mistake must push `dof` PAST it (fraction > 1) on a golden case.
"""
import pytest
import torch

import kbnet_amd as kb
from conftest import load_golden

import posenet_oracle as po
import resnet_pose_oracle as ro

GOLDENS = ("resnet_pose_18_odd", "resnet_pose_34_wide")
KbnError = kb._lib.KbnError
CPU = torch.device("cpu")


def _golden(name):
    g = load_golden(name)
    enc = {k: torch.as_tensor(v) for k, v in g["enc"].items()}
    dec = {k: torch.as_tensor(v) for k, v in g["dec"].items()}
    return g, enc, dec, int(g["n_layer"])


def _widths(enc, dec):
    filters = [enc["conv1.conv.weight"].shape[0]] + [enc[f"blocks{s}.0.conv1.conv.weight"].shape[0] for s in range(2, 6)]
    return filters, [dec["conv.0.conv.weight"].shape[0], dec["conv.1.conv.weight"].shape[0]]


def _model(enc, dec, n_layer):
    filters, decoder_filters = _widths(enc, dec)
    return kb.modules.ResNetPoseNetModel(n_layer, device=CPU, n_filters=filters, decoder_filters=decoder_filters)


@pytest.mark.parametrize("name", GOLDENS)
def test_oracle_equals_reference_bit_for_bit_in_fp32(name):
    g, enc, dec, n_layer = _golden(name)
    o = ro.forward(g["image0"], g["image1"], enc, dec, n_layer)
    layer_names = ro.names(n_layer)
    assert len(o["layers"]) == len(layer_names) == (12 if n_layer == 18 else 20)
    for k, layer in zip(layer_names, o["layers"]):
        assert torch.equal(layer, g["ref32"][k]), (name, k, float((layer - g["ref32"][k]).abs().max()))
    for k in ("map", "dof", "pose"):
        assert torch.equal(o[k], g["ref32"][k]), (name, k)


@pytest.mark.parametrize("name", GOLDENS)
def test_oracle_fp64_matches_reference_fp64(name):
    g, enc, dec, n_layer = _golden(name)
    o = ro.forward(*po.to64(g["image0"], g["image1"], enc, dec), n_layer)
    assert o["dof"].dtype == torch.float64
    for k, layer in zip(ro.names(n_layer), o["layers"]):
        ref = g["ref64"][k]
        assert float((layer - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), (name, k)
    for k in ("map", "dof", "pose"):
        assert float((o[k] - g["ref64"][k]).abs().max()) <= 1e-12 * float(g["ref64"][k].abs().max()), (name, k)


def test_golden_maps_reach_the_sizes_they_are_there_for():
    odd, wide = load_golden("resnet_pose_18_odd"), load_golden("resnet_pose_34_wide")
    assert tuple(odd["image0"].shape) == (2, 3, 61, 77) and tuple(wide["image0"].shape) == (1, 3, 40, 136)
    shapes = [tuple(odd["ref32"][k].shape[2:]) for k in ("conv1", "pool", "blocks2.1", "blocks3.0", "blocks4.0", "blocks5.1",
                                                        "decoder0", "decoder1")]
    assert shapes == [(31, 39), (16, 20), (16, 20), (8, 10), (4, 5), (2, 3), (1, 2), (1, 1)]
    assert tuple(wide["ref32"]["blocks5.2"].shape) == (1, 20, 2, 5) and tuple(wide["ref32"]["decoder1"].shape) == (1, 20, 1, 2)
    assert float(odd["ref32"]["conv1"].min()) < 0       # negatives under the pool: zero padding would win somewhere


@pytest.mark.parametrize("name", GOLDENS)
def test_state_dict_keys_are_the_references(name):
    g, enc, dec, n_layer = _golden(name)       # the generator asserted these key lists equal the reference's
    m = _model(enc, dec, n_layer)
    assert list(m.encoder.state_dict().keys()) == list(enc.keys())
    assert list(m.decoder.state_dict().keys()) == list(dec.keys())
    for sd, want in ((m.encoder.state_dict(), enc), (m.decoder.state_dict(), dec)):
        for k, v in sd.items():
            assert tuple(v.shape) == tuple(want[k].shape) and v.dtype == want[k].dtype, k
    m.encoder.load_state_dict(enc, strict=True)
    m.decoder.load_state_dict(dec, strict=True)
    blocks = sum(kb.posenet_resnet.RESNET_BLOCKS[n_layer])
    assert sum(k.endswith("projection.conv.weight") for k in enc) == blocks      # every block owns one, used or not
    assert len(m.parameters()) == 3 + blocks * 7 + 2 * 3 + 1
    missing = dict(enc)
    del missing["blocks2.1.projection.conv.weight"]                                # never used in a forward; a strict load needs it
    with pytest.raises(RuntimeError):
        m.load_state_dicts(missing, dec)


def test_full_width_shapes_and_synthetic_keys():
    for n_layer in (18, 34):
        m = kb.modules.ResNetPoseNetModel(n_layer, device=CPU)
        enc, dec = kb.synthetic.make_resnet_pose_weights(n_layer, seed=4)
        assert list(m.encoder.state_dict().keys()) == list(enc.keys()) and list(m.decoder.state_dict().keys()) == list(dec.keys())
        m.load_state_dicts(enc, dec)
        assert tuple(enc["conv1.conv.weight"].shape) == (16, 6, 7, 7)
        assert tuple(enc["blocks5.0.projection.conv.weight"].shape) == (256, 128, 1, 1)
        assert tuple(dec["conv.0.conv.weight"].shape) == (256, 256, 3, 3) and tuple(dec["conv.2.conv.weight"].shape) == (6, 256, 1, 1)
        for k, var in enc.items():
            if k.endswith("running_var"):
                small = int((var == 1e-3).sum())
                assert small == max(1, var.numel() // 32) and float(var[var != 1e-3].min()) >= 0.25 and float(var.max()) <= 1.75
        again, _ = kb.synthetic.make_resnet_pose_weights(n_layer, seed=4)
        assert all(torch.equal(enc[k], again[k]) for k in enc)
    assert kb.posenet_resnet.ResNetPoseNetModel is kb.modules.ResNetPoseNetModel
    assert kb.posenet_resnet.load_pose_model is kb.modules.load_pose_model


@pytest.mark.parametrize("prefix", [True, False])
@pytest.mark.parametrize("name", GOLDENS)
def test_checkpoint_restores_bit_for_bit(tmp_path, name, prefix):
    """A checkpoint in the reference's layout (src/posenet_model.py:150-172), through restore_model and through load_pose_model."""
    g, enc, dec, n_layer = _golden(name)
    pref = (lambda sd: {"module." + k: v for k, v in sd.items()}) if prefix else (lambda sd: dict(sd))
    path = str(tmp_path / "pose_model-9.pth")
    torch.save({"train_step": 9, "optimizer_state_dict": {}, "encoder_state_dict": pref(enc), "decoder_state_dict": pref(dec)}, path)
    a = _model(enc, dec, n_layer)
    step, opt = a.restore_model(path)
    assert step == 9 and opt is None
    b = kb.modules.load_pose_model(path, CPU)
    assert type(b) is kb.modules.ResNetPoseNetModel and b.n_layer == n_layer
    assert b.encoder_type == f"resnet{n_layer}" and not isinstance(b, kb.modules.PoseNetModel)      # siblings over one base
    assert isinstance(b, kb.posenet.PoseModelBase)
    for m in (a, b):
        for got, want in ((m.encoder.state_dict(), enc), (m.decoder.state_dict(), dec)):
            assert list(got) == list(want)
            assert all(torch.equal(got[k], want[k]) for k in want)
    again = str(tmp_path / "pose_model-10.pth")
    b.save_model(again, step=10)
    ckpt = torch.load(again)
    assert all(k.startswith("module.") for k in list(ckpt["encoder_state_dict"]) + list(ckpt["decoder_state_dict"]))
    assert all(torch.equal(ckpt["encoder_state_dict"]["module." + k], enc[k]) for k in enc)


def test_load_pose_model_tells_the_layouts_apart(tmp_path):
    g = load_golden("posenet_wide")
    enc = {k: torch.as_tensor(v) for k, v in g["enc"].items()}
    dec = {k: torch.as_tensor(v) for k, v in g["dec"].items()}
    path = str(tmp_path / "posenet.pth")
    torch.save({"train_step": 1, "optimizer_state_dict": {}, "encoder_state_dict": {"module." + k: v for k, v in enc.items()},
                "decoder_state_dict": dec}, path)
    m = kb.modules.load_pose_model(path, CPU)
    assert type(m) is kb.modules.PoseNetModel
    assert m.encoder_type == "posenet" and isinstance(m, kb.posenet.PoseModelBase)
    assert all(torch.equal(m.encoder.state_dict()[k], enc[k]) for k in enc) and torch.equal(m.decoder.conv.conv.weight, dec["conv.conv.weight"])
    _, renc, rdec, _ = _golden("resnet_pose_18_odd")
    three = {k: v for k, v in renc.items() if not k.startswith("blocks2.1.")}              # block counts [1, 2, 2, 2]: neither 18 nor 34
    unknown = {"features.0.weight": torch.zeros(4, 6, 3, 3)}
    for bad_enc, bad_dec, word in ((three, rdec, "blocks2.0.conv1.conv.weight"), (unknown, rdec, "features.0.weight"),
                                   (enc, rdec, "conv.2.conv.weight")):
        torch.save({"train_step": 1, "optimizer_state_dict": {}, "encoder_state_dict": bad_enc, "decoder_state_dict": bad_dec}, path)
        with pytest.raises(KbnError, match=word):
            kb.modules.load_pose_model(path, CPU)
    torch.save({"model": renc}, path)
    with pytest.raises(KbnError, match="encoder_state_dict"):
        kb.modules.load_pose_model(path, CPU)


def test_what_is_out_of_scope_raises():
    small = dict(device=CPU, n_filters=[4, 8, 8, 12, 20], decoder_filters=[12, 20])
    with pytest.raises(KbnError, match="18 or 34"):
        kb.modules.ResNetPoseNetModel(50, **small)
    for act in ("elu", "sigmoid"):
        with pytest.raises(KbnError, match="leaky_relu"):
            kb.modules.ResNetPoseNetModel(18, activation_func=act, **small)
    for act in ("leaky_relu", "relu", "linear"):
        kb.modules.ResNetPoseNetModel(18, activation_func=act, **small)
    with pytest.raises(KbnError, match="axis"):
        kb.modules.ResNetPoseNetModel(18, rotation_parameterization="euler", **small)
    with pytest.raises(KbnError):
        kb.modules.ResNetEncoder(18, input_channels=6, n_filters=[4, 8, 8, 12, 20], use_batch_norm=False)
    with pytest.raises(KbnError, match="ResNetPoseNetModel"):          # the plain class still refuses, and says where to go
        kb.modules.PoseNetModel(encoder_type="resnet18", device=CPU)
    m = kb.modules.ResNetPoseNetModel(34, **small)
    with pytest.raises(KbnError, match="inference only"):
        m.train()
    assert m.data_parallel() is m
    m.eval()
    with pytest.raises(KbnError):          # no CPU path
        m.forward(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16))
    x = torch.zeros(1, 4, 8, 8)
    with pytest.raises(KbnError):
        kb.ops.maxpool3x3s2(x)
    with pytest.raises(KbnError):
        kb.ops.conv2d_affine([x], torch.zeros(32), torch.ones(4), torch.zeros(4), 4, 1, 1)
    with pytest.raises(KbnError):
        kb.ops.pack_conv2d_affine_weight(torch.zeros(4, 4, 3, 3))


# ---------------------------------------------------------------- power: the dof gate sees each of these mistakes
MISTAKES = {
    "projection_skipped": dict(skip_projection=True),
    "conv2_activation_dropped": dict(conv2_act=False),
    "final_activation_dropped": dict(final_act=False),
    "pool_padding_zero": dict(pool_pad_zero=True),
    "slope_0.10": dict(slope=0.10),
    "eps_dropped": dict(eps=0.0),
    "stage1_stride_2": dict(stage1_stride=2),
}


@pytest.fixture(scope="module")
def right():
    """The fp64 oracle's forward of both goldens, computed once."""
    out = {}
    for name in GOLDENS:
        g, enc, dec, n_layer = _golden(name)
        args = po.to64(g["image0"], g["image1"], enc, dec)
        o = ro.forward(*args, n_layer)
        assert float((o["dof"] - g["ref64"]["dof"]).abs().max()) <= 1e-12
        out[name] = (args, n_layer, o)
    return out


@pytest.mark.parametrize("mistake", list(MISTAKES))
def test_the_dof_gate_sees_a_planted_mistake(right, mistake):
    fractions = {}
    for name, (args, n_layer, o) in right.items():
        wrong = ro.forward(*args, n_layer, **MISTAKES[mistake])
        fractions[name] = po.gate_fraction(wrong["dof"], o["dof"], po.dof_floor(o["map"]))
    print(mistake, " ".join(f"{k} {v:.3g} x the gate" for k, v in fractions.items()))
    assert min(fractions.values()) > 1.0, (mistake, fractions)
