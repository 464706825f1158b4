"""modules._PackedBlob -- the one cache of packed weights -- and the walk that refreshes every instance ahead of a graph replay.
No GPU and no library: a fake packer on CPU tensors."""
import dataclasses

import pytest
import torch

import kbnet_amd as kb

_PackedBlob = kb.modules._PackedBlob


class FakePacker:
    """pack(*weights, out=None, **opts): the sum of every weight (+ the xyz_offset option) into a blob of 4 floats, into `out`
    when one is given; counts its calls."""

    def __init__(self):
        self.calls = 0

    def __call__(self, *weights, out=None, xyz_offset=0):
        self.calls += 1
        blob = out if out is not None else torch.empty(4)
        blob.fill_(float(sum(w.sum() for w in weights)) + xyz_offset)
        return blob


@pytest.fixture
def pack():
    return FakePacker()


def test_unchanged_weight_is_not_packed_again(pack):
    cache, w = _PackedBlob(pack), torch.ones(3)
    blob = cache.get(w)
    assert pack.calls == 1 and blob.tolist() == [3.0] * 4
    assert cache.get(w) is blob and pack.calls == 1


def test_in_place_update_repacks_into_the_same_blob(pack):
    cache, w = _PackedBlob(pack), torch.ones(3)
    ptr = cache.get(w).data_ptr()
    w.mul_(2)
    blob = cache.get(w)
    assert pack.calls == 2 and blob.data_ptr() == ptr and blob.tolist() == [6.0] * 4
    assert cache.get(w) is blob and pack.calls == 2


def test_replaced_storage_repacks(pack):
    cache, w = _PackedBlob(pack), torch.ones(3)
    cache.get(w)
    version = w._version
    w.data = w.data.clone()
    assert w._version == version      # only the storage moved
    cache.get(w)
    assert pack.calls == 2


def test_changed_option_repacks(pack):
    cache, w = _PackedBlob(pack), torch.ones(3)
    assert cache.get(w, xyz_offset=16).tolist() == [19.0] * 4
    assert cache.get(w, xyz_offset=16).tolist() == [19.0] * 4 and pack.calls == 1
    assert cache.get(w, xyz_offset=32).tolist() == [35.0] * 4 and pack.calls == 2


def test_refresh_of_a_cache_never_built_calls_nothing(pack):
    cache = _PackedBlob(pack)
    cache.refresh()
    assert pack.calls == 0


def test_refresh_repacks_in_place_with_the_last_options(pack):
    cache, w = _PackedBlob(pack), torch.ones(3)
    blob = cache.get(w, xyz_offset=16)
    cache.refresh()
    assert pack.calls == 1            # nothing changed: nothing packed
    w.add_(1)
    cache.refresh()
    assert pack.calls == 2 and blob.tolist() == [22.0] * 4      # the same tensor, the new weights, xyz_offset still 16
    assert cache.get(w, xyz_offset=16) is blob and pack.calls == 2


def test_two_weights_either_change_repacks(pack):
    cache, a, b = _PackedBlob(pack), torch.ones(3), torch.ones(2)
    assert cache.get(a, b).tolist() == [5.0] * 4
    a.mul_(3)
    assert cache.get(a, b).tolist() == [11.0] * 4 and pack.calls == 2
    b.mul_(3)
    assert cache.get(a, b).tolist() == [15.0] * 4 and pack.calls == 3
    assert cache.get(a, b).tolist() == [15.0] * 4 and pack.calls == 3


def _reachable_blobs(model):
    """Every _PackedBlob among the attributes of the model's sub-modules -- found without modules.packed_blobs: torch's own
    named_modules() walk and a look into each module's attributes, containers included."""
    found = {}

    def look(value):
        if isinstance(value, _PackedBlob):
            found[id(value)] = value
        elif isinstance(value, (list, tuple)):
            for v in value:
                look(v)
        elif isinstance(value, dict):
            for v in value.values():
                look(v)

    for top in model.modules():
        for _, sub in top.named_modules():
            for name, value in sub.__dict__.items():
                if name not in ("_modules", "_parameters", "_buffers"):
                    look(value)
    return found


def _refreshed_blobs(model, monkeypatch):
    seen = {}
    monkeypatch.setattr(_PackedBlob, "refresh", lambda self: seen.__setitem__(id(self), self))
    model.refresh_packed()
    return seen


@pytest.mark.parametrize("deconv_type", ["up", "transpose"])
def test_refresh_packed_reaches_every_blob_of_kbnet(monkeypatch, deconv_type):
    cfg = dataclasses.replace(kb.kitti_config().narrow(), deconv_type=deconv_type)
    m = kb.modules.KBNetModel.from_config(cfg, torch.device("cpu"))
    want = _reachable_blobs(m)
    assert set(_refreshed_blobs(m, monkeypatch)) == set(want) and want
    enc, dec = m.encoder, m.decoder
    owned = [enc._packed_front, enc._packed_front_next, enc._packed_depth_front, enc._packed_s2d_front, dec._packed_tail]
    n_layers = 0
    for top in m.modules():
        for sub in top.modules():
            if isinstance(sub, (kb.modules.Conv2d, kb.modules.UpConv2d, kb.modules.TransposeConv2d)):
                n_layers += 1
                layer = [v for v in vars(sub).values() if isinstance(v, _PackedBlob)]
                assert layer, type(sub).__name__
                owned += layer
    assert n_layers > 20 and len({id(b) for b in owned}) == len(owned)
    assert {id(b) for b in owned} == set(want)
    ups = [type(getattr(dec, f"deconv{i}").deconv) for i in range(5)]
    assert ups == [kb.modules.TransposeConv2d if deconv_type == "transpose" else kb.modules.UpConv2d] * 5


def test_refresh_packed_reaches_every_blob_of_posenet(monkeypatch):
    m = kb.posenet.PoseNetModel(device=torch.device("cpu"))
    want = _reachable_blobs(m)
    assert set(_refreshed_blobs(m, monkeypatch)) == set(want)
    assert set(want) == {id(layer._packed) for layer in m.encoder.layers()} and len(want) == 7
