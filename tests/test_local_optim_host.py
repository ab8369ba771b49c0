"""Host half of the population optimizer (no GPU): layer_offsets, every refusal of
PopulationOptimizer.check, bytes_per_step per rule, the library's host-only queries, and the C entry
point's argument checks, which run before any device work."""
import numpy as np
import pytest

from federated_amd import _lib
from federated_amd.local_optim import PopulationOptimizer, layer_offsets

# the drivers' MNIST CNN in get_weights() order: conv 3x3x1x32, conv 3x3x32x64, dense 9216x128, 128x10
MNIST = [(3, 3, 1, 32), (32,), (3, 3, 32, 64), (64,), (9216, 128), (128,), (128, 10), (10,)]


def test_layer_offsets():
    got = layer_offsets(MNIST)
    assert got.dtype == np.int32
    assert got.tolist() == [0, 288, 320, 18752, 18816, 1198464, 1198592, 1199872, 1199882]
    assert layer_offsets([(), (3,), 5]).tolist() == [0, 1, 4, 9]  # a scalar variable holds one element
    for bad in ([], [(3, 0)], [(1 << 20, 1 << 12)]):
        with pytest.raises(ValueError):
            layer_offsets(bad)


def test_check_accepts_shapes_and_tables():
    info = PopulationOptimizer.check(8, MNIST, "adam", 1e-3, clipnorm=1.0)
    assert (info["D"], info["P"], info["n"], info["state"], info["clipnorm"]) == (8, 1199882, 8, 2, 1.0)
    assert info["rule"] == _lib.OPTIM_ADAM and info["trainable"].tolist() == [1] * 8
    assert info["layer_ptr"].tolist() == layer_offsets(MNIST).tolist()
    info = PopulationOptimizer.check(2, layer_offsets(MNIST), "momentum", 0.01, momentum=0.9, P=1199882,
                                     trainable=[1, 1, 0, 0, 1, 1, 1, 1])
    assert (info["rule"], info["state"], info["clipnorm"]) == (_lib.OPTIM_MOMENTUM, 1, 0.0)
    assert info["trainable"].tolist() == [1, 1, 0, 0, 1, 1, 1, 1]
    info = PopulationOptimizer.check(1, [0, 3, 7], "sgd", 0.1)
    assert (info["rule"], info["state"], info["P"], info["n"]) == (_lib.OPTIM_SGD, 0, 7, 2)


@pytest.mark.parametrize("kw", [
    dict(rule="nesterov"),                                    # an unknown rule
    dict(rule="adam", beta_1=1.0),                            # beta = 1
    dict(rule="adam", beta_2=1.0),
    dict(rule="adam", beta_1=-0.1),
    dict(layers=np.array([0, 4, 4, 9])),                      # a non-increasing table
    dict(layers=np.array([0, 5, 3, 9])),
    dict(layers=np.array([1, 5, 9])),                         # does not start at 0
    dict(layers=np.array([0, 4, 8]), P=9),                    # does not end at P
    dict(trainable=[1, 1]),                                   # wrong length
    dict(D=0),
    dict(lr=float("inf")),
    dict(lr=float("nan")),
    dict(rule="adam", epsilon=-1.0),
    dict(rule="adam", clipnorm=0.0),
    dict(rule="sgd", clipnorm=1.0),                           # the reference clips under Adam only
])
def test_check_refusals(kw):
    a = dict(D=3, layers=np.array([0, 4, 6, 9]), rule="adam", lr=1e-3)
    a.update(kw)
    with pytest.raises(ValueError):
        PopulationOptimizer.check(a.pop("D"), a.pop("layers"), a.pop("rule"), a.pop("lr"), **a)


class _HostOnly(PopulationOptimizer):
    """bytes_per_step needs the sizes only: no engine, no device."""

    def __init__(self, D, layers, rule, clipnorm=None, trainable=None):
        info = self.check(D, layers, rule, 0.1, clipnorm=clipnorm, trainable=trainable)
        self.D, self.rule_name, self.clipnorm = info["D"], rule, info["clipnorm"]
        self._trainable_elems = int(np.diff(info["layer_ptr"])[info["trainable"] != 0].sum())


def test_bytes_per_step():
    D, P = 8, 1199882
    assert _HostOnly(D, MNIST, "sgd").bytes_per_step() == 12 * D * P           # w read + written, g read
    assert _HostOnly(D, MNIST, "momentum").bytes_per_step() == 20 * D * P      # + the accumulator, both ways
    assert _HostOnly(D, MNIST, "adam").bytes_per_step() == 28 * D * P          # + v, both ways
    assert _HostOnly(D, MNIST, "adam", clipnorm=1.0).bytes_per_step() == 32 * D * P  # g twice under the clip
    frozen = _HostOnly(D, MNIST, "adam", clipnorm=1.0, trainable=[1, 1, 1, 1, 0, 1, 1, 1])
    assert frozen.bytes_per_step() == 32 * D * (P - 9216 * 128)


def test_library_queries_are_host_only():
    lib = _lib.load()
    for name in ("cfa_optim_step_f32", "cfa_optim_tile", "cfa_optim_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    T = lib.cfa_optim_tile()
    assert T >= 4 and T % 4 == 0
    # one fp64 partial per (tile, layer) pair that can meet: tiles + layers slots per device
    assert lib.cfa_optim_workspace_bytes(3, 4 * T + 11, 7) == 3 * (5 + 7) * 8
    assert lib.cfa_optim_workspace_bytes(1, T, 1) == 2 * 8
    assert lib.cfa_optim_workspace_bytes(0, T, 1) == 0


def _step(**kw):
    a = dict(models=1 << 20, pitch=100, grads=1 << 21, gpitch=100, m=1 << 22, v=1 << 23, spitch=100,
             layer_ptr=1 << 24, trainable=1 << 25, n=3, skip=None, t=1 << 26, pow=1 << 27, rule=_lib.OPTIM_ADAM,
             lr=1e-3, momentum=0.0, b1=0.9, b2=0.999, eps=1e-7, clip=1.0, ws=1 << 28, ws_bytes=1 << 20, D=2, P=100)
    a.update(kw)
    _lib.call("cfa_optim_step_f32", a["models"], a["pitch"], a["grads"], a["gpitch"], a["m"], a["v"], a["spitch"],
              a["layer_ptr"], a["trainable"], a["n"], a["skip"], a["t"], a["pow"], a["rule"], a["lr"], a["momentum"],
              a["b1"], a["b2"], a["eps"], a["clip"], a["ws"], a["ws_bytes"], a["D"], a["P"], None)


@pytest.mark.parametrize("kw,match,code", [
    (dict(models=None), "null models", _lib.CFA_E_INVALID),
    (dict(grads=None), "null models", _lib.CFA_E_INVALID),
    (dict(layer_ptr=None), "null models", _lib.CFA_E_INVALID),
    (dict(trainable=None), "null models", _lib.CFA_E_INVALID),
    (dict(t=None), "null models", _lib.CFA_E_INVALID),
    (dict(m=None), "null state m", _lib.CFA_E_INVALID),
    (dict(m=None, rule=_lib.OPTIM_MOMENTUM), "null state m", _lib.CFA_E_INVALID),
    (dict(v=None), "null state v", _lib.CFA_E_INVALID),
    (dict(pow=None), "null state v or running powers", _lib.CFA_E_INVALID),
    (dict(D=0), "must be >= 1", _lib.CFA_E_INVALID),
    (dict(P=0), "must be >= 1", _lib.CFA_E_INVALID),
    (dict(n=0), "must be >= 1", _lib.CFA_E_INVALID),
    (dict(rule=3), "unknown optimizer rule 3", _lib.CFA_E_INVALID),
    (dict(rule=-1), "unknown optimizer rule", _lib.CFA_E_INVALID),
    (dict(pitch=99), "below P", _lib.CFA_E_INVALID),
    (dict(gpitch=99), "below P", _lib.CFA_E_INVALID),
    (dict(spitch=99), "below P", _lib.CFA_E_INVALID),
    (dict(models=(1 << 20) + 2), "misaligned", _lib.CFA_E_UNSUPPORTED),
    (dict(v=(1 << 23) + 1), "misaligned", _lib.CFA_E_UNSUPPORTED),
    (dict(t=(1 << 26) + 4), "misaligned", _lib.CFA_E_UNSUPPORTED),
    (dict(b1=1.0), "must lie in", _lib.CFA_E_INVALID),
    (dict(b2=1.0), "must lie in", _lib.CFA_E_INVALID),
    (dict(b1=-0.5), "must lie in", _lib.CFA_E_INVALID),
    (dict(b2=float("nan")), "must lie in", _lib.CFA_E_INVALID),
    (dict(lr=float("inf")), "learning rate is not finite", _lib.CFA_E_INVALID),
    (dict(lr=float("nan"), rule=_lib.OPTIM_SGD), "learning rate is not finite", _lib.CFA_E_INVALID),
    (dict(momentum=float("inf"), rule=_lib.OPTIM_MOMENTUM), "momentum is not finite", _lib.CFA_E_INVALID),
    (dict(eps=-1.0), "epsilon", _lib.CFA_E_INVALID),
    (dict(ws=None), "workspace", _lib.CFA_E_INVALID),
    (dict(ws_bytes=8), "workspace", _lib.CFA_E_INVALID),
    (dict(P=(1 << 31) - 1, pitch=1 << 31, gpitch=1 << 31, spitch=1 << 31), "int32 layer table", _lib.CFA_E_UNSUPPORTED),
    (dict(D=65536), "devices in one step", _lib.CFA_E_UNSUPPORTED),
])
def test_entry_point_validates_before_any_device_work(kw, match, code):
    """The library's code and message; nothing is launched (the pointers are fake)."""
    with pytest.raises(_lib.CFAError, match=match) as e:
        _step(**kw)
    assert e.value.code == code
