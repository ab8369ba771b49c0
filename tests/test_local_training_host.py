"""Host half of the local-training feature (no GPU): LocalSgd.check accepts the two CFA-GE model
shapes and refuses every documented misuse, the library exports the two entry points, and the
entry points validate their arguments before any device work."""
import pytest

from federated_amd import _lib
from federated_amd.local_training import LocalSgd, model_size

CNN = {"filter": 16, "number": 8, "stride": 5}
NN = {"intermediate_nodes": 32}


def test_check_accepts_the_c3_and_c1_shapes():
    # config 3: 16 devices, CNN, 24 samples of 512 inputs, 8 classes; the drivers' slicing
    info = LocalSgd.check(1, CNN, (16, 24, 512), (16, 24, 8))
    assert info == {"D": 16, "Ns": 24, "L": 512, "classes": 8, "P": 1488, "steps": 4}
    # config 1: the 2NN
    info = LocalSgd.check(2, NN, (16, 24, 512), (16, 24, 8), x_test_shape=(16, 11, 512), y_test_shape=(16, 11, 8))
    assert info["P"] == 16680 and info["steps"] == 4 and info["Nt"] == 11 and info["test_steps"] == 2
    # the last minibatch may end exactly at Ns
    assert LocalSgd.check(1, CNN, (2, 34, 512), (2, 34, 8), steps=7)["steps"] == 7
    assert LocalSgd.check(1, CNN, (2, 9, 512), (2, 9, 8), batch_stride=3, batch_rows=3)["steps"] == 3
    assert model_size(1, CNN, 512, 8) == 1488 and model_size(2, NN, 512, 8) == 16680


@pytest.mark.parametrize("kw", [
    dict(x_shape=(16, 24, 512), y_shape=(15, 24, 8)),                     # devices differ
    dict(x_shape=(16, 24, 512), y_shape=(16, 23, 8)),                     # samples differ
    dict(x_shape=(24, 512), y_shape=(24, 8)),                             # not a population
    dict(x_shape=(16, 24, 512), y_shape=(16, 24, 8), steps=6),            # the 6th ends at row 29
    dict(x_shape=(16, 33, 512), y_shape=(16, 33, 8), steps=7),            # the 7th ends at row 34
    dict(x_shape=(16, 3, 512), y_shape=(16, 3, 8)),                       # not one minibatch
    dict(x_shape=(16, 24, 512), y_shape=(16, 24, 8), steps=0),
    dict(x_shape=(16, 24, 512), y_shape=(16, 24, 8), batch_rows=0),
    dict(x_shape=(16, 24, 512), y_shape=(16, 24, 8), batch_stride=0),
    dict(x_shape=(16, 24, 512), y_shape=(16, 24, 8), x_test_shape=(16, 10, 512)),                      # half a test set
    dict(x_shape=(16, 24, 512), y_shape=(16, 24, 8), x_test_shape=(16, 10, 500), y_test_shape=(16, 10, 8)),
    dict(x_shape=(16, 24, 512), y_shape=(16, 24, 8), x_test_shape=(16, 10, 512), y_test_shape=(16, 10, 8),
         test_steps=3),                                                   # the test set holds two
])
def test_check_refusals(kw):
    kw = dict(kw)
    x_shape, y_shape = kw.pop("x_shape"), kw.pop("y_shape")
    with pytest.raises(ValueError):
        LocalSgd.check(1, CNN, x_shape, y_shape, **kw)


def test_check_refuses_an_unknown_model():
    with pytest.raises(ValueError, match="ml_model"):
        LocalSgd.check(3, CNN, (16, 24, 512), (16, 24, 8))
    with pytest.raises(ValueError, match="ml_model"):
        model_size(0, NN, 512, 8)


def test_library_exports_both_entry_points():
    lib = _lib.load()
    for name in ("cfa_local_sgd_cnn_f32", "cfa_local_sgd_2nn_f32"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)


def _cnn(**kw):
    a = dict(x=1 << 20, y=1 << 20, Ns=24, L=512, C=8, F=16, NC=8, S=5, models=1 << 20, pitch=1488, D=2, bstride=5,
             brows=4, steps=4, lr=0.1, update=1, cost=None, log=None, cap=0, epoch=None)
    a.update(kw)
    _lib.call("cfa_local_sgd_cnn_f32", a["x"], a["y"], a["Ns"], a["L"], a["C"], a["F"], a["NC"], a["S"], a["models"],
              a["pitch"], a["D"], a["bstride"], a["brows"], a["steps"], a["lr"], a["update"], a["cost"], a["log"],
              a["cap"], a["epoch"], None)


def _nn(**kw):
    a = dict(x=1 << 20, y=1 << 20, Ns=24, L=512, H=32, C=8, models=1 << 20, pitch=16680, D=2, bstride=5, brows=4,
             steps=4, lr=0.1, update=1, cost=None, log=None, cap=0, epoch=None)
    a.update(kw)
    _lib.call("cfa_local_sgd_2nn_f32", a["x"], a["y"], a["Ns"], a["L"], a["H"], a["C"], a["models"], a["pitch"],
              a["D"], a["bstride"], a["brows"], a["steps"], a["lr"], a["update"], a["cost"], a["log"], a["cap"],
              a["epoch"], None)


@pytest.mark.parametrize("call", [_cnn, _nn])
@pytest.mark.parametrize("kw,match", [
    (dict(steps=0), "must be >= 1"),
    (dict(brows=0), "must be >= 1"),
    (dict(steps=6), "ends at row 29"),
    (dict(pitch=100), "pitch"),
    (dict(x=None), "null buffer"),
    (dict(models=None), "null buffer"),
    (dict(log=1 << 20), "given together"),
    (dict(log=1 << 20, epoch=1 << 20, cap=0), "log_cap"),
    (dict(L=0), "bad dimensions"),
])
def test_entry_points_validate_before_any_device_work(call, kw, match):
    """CFA_E_INVALID with the library's message; nothing is launched (the pointers are fake)."""
    with pytest.raises(_lib.CFAError, match=match) as e:
        call(**kw)
    assert e.value.code == _lib.CFA_E_INVALID


@pytest.mark.parametrize("call", [_cnn, _nn])
def test_an_empty_population_is_a_no_op(call):
    call(D=0)
