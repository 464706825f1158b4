"""CPU: what the frame-axis properties of tests/test_grad_batch_axis_gpu.py reject.  Their helpers run here on a CPU stand-in of the
stride-2 data gradient that is right by construction (torch's conv2d_input, one frame at a time), and then on the same stand-in with
one mistake of the flattened index m = (frame * H + y) * W + x planted in it: every property must pass the first and name the second."""
import math

import pytest
import torch

import posenet_grad_oracle as pgo
import test_grad_batch_axis_gpu as axis

CASE = ((5,), 19, 9, 13, 3, 3, 2)       # 117 pixels per frame: the tile boundary at 128 falls inside the first row of frame 1
CPU = torch.device("cpu")


def _stand_in(mistake=None):
    cins, oc, h, w, n, k, stride = CASE
    c = axis._conv_problem(*CASE)
    weight = c["weight"]

    def call(d, out=None):
        g = d["grad_out"]
        if mistake == "dense batch stride" and not g.is_contiguous():        # the batch stride of a dense tensor on a channel slice
            g = g.as_strided(g.shape, (g.shape[1] * g.shape[2] * g.shape[3],) + tuple(g.stride()[1:]), g.storage_offset())
        frames = [torch.nn.grad.conv2d_input((1, sum(cins), h, w), weight, g[i:i + 1].double().contiguous(), stride=stride, padding=k // 2)
                  for i in range(g.shape[0])]
        res = torch.cat(frames).float()
        if mistake == "tile keeps its first frame" and g.shape[0] > 1:      # the tile that starts in frame 0 ends in frame 1's first row
            res[1, :, 0, :128 - h * w] = res[0, :, 0, :128 - h * w]
        if mistake == "zero times a load":                                   # the frame's other pixels load the value and multiply by 0
            res = res + 0.0 * g.sum(dim=(1, 2, 3), keepdim=True)
        if mistake == "zero times the next frame's load" and g.shape[0] > 1:
            res[:-1] = res[:-1] + 0.0 * g[1:].sum(dim=(1, 2, 3), keepdim=True)
        if out is not None:
            out[0].copy_(res)
            return [out[0]]
        return [res]
    label = f"stand-in ({mistake})"
    return axis.Op(label, {"grad_out": c["grad_out"].float()}, call, lambda got: axis._fractions(label, got, [c["grad_xs"][0]], pgo.TOL),
                   ("grad_out",), [(n, sum(cins), h, w)])


def _containment(op):
    cins, oc, h, w, n, k, stride = CASE
    mid, f = n // 2, oc // 2
    oy, ox = axis._interior(h, w, k, stride)
    field, _, _ = axis._receptive_field(h, w, k, stride, oy, ox)
    clean = op.call(op.on(CPU))
    for bad in (axis.NAN, math.inf):
        args = {"grad_out": op.args["grad_out"].clone()}
        args["grad_out"][mid, f, oy, ox] = bad
        axis._contained(op.label, op.call(op.on(CPU, args)), clean, mid, [field.expand(sum(cins), h, w)], bad)


PROPERTIES = {"a frame alone": lambda op: axis._frame_alone(CPU, op), "frame order": lambda op: axis._frame_order(CPU, op),
              "batch strides": lambda op: axis._batch_strides(CPU, op), "containment": _containment}


@pytest.mark.parametrize("name", list(PROPERTIES))
def test_the_right_stand_in_has_every_property(name):
    PROPERTIES[name](_stand_in())


@pytest.mark.parametrize("mistake, seen_by", [
    ("tile keeps its first frame", ("a frame alone", "frame order")),
    ("zero times a load", ("containment",)),
    ("zero times the next frame's load", ("containment",)),
    ("dense batch stride", ("batch strides",)),
])
def test_a_planted_mistake_fails_its_property(mistake, seen_by):
    for name in seen_by:
        with pytest.raises(AssertionError):
            PROPERTIES[name](_stand_in(mistake))
    # the mistakes of the clean data are invisible to the value gate on random inputs only where they multiply by zero
    if mistake.startswith("zero times"):
        PROPERTIES["a frame alone"](_stand_in(mistake))
