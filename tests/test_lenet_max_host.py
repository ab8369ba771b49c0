"""Host checks of the max-pool CNNs of the TF2 drivers (tests/lenet_max_cases.py has the
restatement, the cases and the seed rule): sizes and stage chain, the restatement's backward pass
against central finite differences of its own forward pass, the seed rule derived again for every
case, the launch plan of cfa_lenet_max.hip that puts each case on its path, `check(pool=...)`, and
the new entry points' validation with fake pointers (nothing is launched). No GPU."""
import numpy as np
import pytest

import lenet_cases as lc
import lenet_grad_cases as gc
import lenet_max_cases as mc


def test_sizes_and_stage_chain_of_the_driver_models():
    from federated_amd import _lib
    from federated_amd.tf2_validation import MNIST_CNN14, MNIST_CNN32, lenet_layer_shapes, lenet_size
    assert (MNIST_CNN32, MNIST_CNN14) == (mc.MNIST_CNN32, mc.MNIST_CNN14)
    for geom, P in ((MNIST_CNN32, 34826), (MNIST_CNN14, 24278)):
        assert lenet_size(geom) == lc.size(geom) == P == int(_lib.load().cfa_lenet_params(*geom))
        assert (geom[0],) + lc.stages(geom) == (28, 26, 13, 11, 5)
        assert lenet_layer_shapes(geom)[4] == (1600, 10)
    assert lc.UNSUPPORTED == MNIST_CNN32  # what the average-pool entries refuse


@pytest.mark.parametrize("loss", mc.LOSSES)
@pytest.mark.parametrize("name", ["pool2_drops", "pool1_drops"])
def test_restatement_backward_against_central_differences(name, loss):
    """fp64, every parameter of model 0: (f(w + h) - f(w - h)) / 2h with h = 1e-6."""
    geom, batch, Nt, _, _ = mc.CASES[name]
    x, labels, models = mc.data(name)
    idx = np.arange(batch)
    row = models[0].astype(np.float64)
    g, value = mc.grads(x[idx], labels[idx], row, geom, loss)
    assert abs(value - mc.loss_of(x[idx], labels[idx], row, geom, loss)) <= 1e-15
    h = 1e-6
    fd = np.zeros_like(g)
    for i in range(len(row)):
        up, dn = row.copy(), row.copy()
        up[i] += h
        dn[i] -= h
        fd[i] = (mc.loss_of(x[idx], labels[idx], up, geom, loss) - mc.loss_of(x[idx], labels[idx], dn, geom, loss)) / (2 * h)
    # the loss is piecewise smooth and the case keeps every kink GUARD away: the central difference's
    # error is O(h^2) of the third derivative plus 1e-16 / h of rounding, both below 1e-8 here
    for a, b in zip(gc.tensors(g, geom), gc.tensors(fd, geom)):
        assert np.abs(a).max() > 0
        assert np.max(np.abs(a - b)) <= 1e-7 * max(1.0, np.abs(b).max()), (name, loss, np.max(np.abs(a - b)))


def test_first_maximum_takes_a_tie_and_a_dead_window_passes_nothing():
    z = np.zeros((1, 5, 5, 1))
    z[0, 0:2, 0:2, 0] = [[1.0, 2.0], [2.0, 0.5]]   # a tie of (0,1) and (1,0): the first wins
    z[0, 0:2, 2:4, 0] = [[-1.0, -2.0], [0.0, -3.0]]  # no positive z: relu ties at 0, nothing passes
    z[0, 2:4, 0:2, 0] = [[-1.0, -1.0], [-1.0, 3.0]]
    z[0, 4, :, 0] = 9.0  # the dropped row and column
    z[0, :, 4, 0] = 9.0
    assert mc.max_pool(np.maximum(z, 0))[0, :, :, 0].tolist() == [[2.0, 0.0], [3.0, 0.0]]
    d = np.array([[10.0, 20.0], [30.0, 40.0]]).reshape(1, 2, 2, 1)
    out = mc._unpool(d, z)[0, :, :, 0]
    want = np.zeros((5, 5))
    want[0, 1], want[3, 1] = 10.0, 30.0
    assert (out == want).all()


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_a_case_keeps_its_decisions_and_has_the_smallest_seed_that_meets_the_rule(name):
    geom, batch, Nt, D, seed = mc.CASES[name]
    assert mc.smallest_seed(name) == seed < mc.SEED_BOUND
    x, _, models = mc.data(name)
    for row in models:
        lo, gap, hi, shift = mc.decisions(x, row, geom)
        print(name, "smallest |z|", lo, "smallest gap", gap, "largest |z|", hi, "fp32 shift", shift, shift / hi)
        assert lo >= mc.GUARD * hi and gap >= mc.GUARD * hi
        assert shift <= 0.1 * mc.GUARD * hi  # fp32 moves a pre-activation by under a tenth of the guard


@pytest.mark.parametrize("name", sorted(mc.CASES) + sorted(mc.EVAL_CASES))
def test_a_case_reaches_its_path(name):
    for text, ok in mc.path(name).items():
        assert ok, (name, text)


def test_workspace_bytes_without_gpu():
    from federated_amd import _lib
    lib = _lib.load()
    for geom in (mc.MNIST_CNN32, mc.MNIST_CNN14, (12, 3, 2, 3, 4)):
        for batch in (1, 8, 9, 100):
            assert int(lib.cfa_lenet_max_grad_workspace_bytes(16, batch, *geom)) == mc.grad_workspace_bytes(geom, batch, 16)
    assert mc.grad_workspace_bytes(mc.MNIST_CNN32, 100, 16) == 28981888  # DESIGN: 27.6 MiB at the drivers' sizes
    assert mc.grad_workspace_bytes(mc.MNIST_CNN14, 100, 16) == 20205952
    assert int(lib.cfa_lenet_max_grad_workspace_bytes(0, 4, *mc.MNIST_CNN32)) == 0
    assert int(lib.cfa_lenet_max_grad_workspace_bytes(1, 4, 6, 3, 2, 3, 4)) == 0
    assert int(lib.cfa_lenet_max_eval_workspace_bytes(3, 5)) == 60 and int(lib.cfa_lenet_max_eval_workspace_bytes(3, 0)) == 0


def test_check_takes_the_pool():
    from federated_amd.tf2_training import LenetTraining
    from federated_amd.tf2_validation import MNIST_CNN14, MNIST_CNN32, LenetValidation
    for geom, P in ((MNIST_CNN32, 34826), (MNIST_CNN14, 24278)):
        info = LenetValidation.check(geom, (16, 200, 28, 28), (16, 200), 100, target=0.5, pool="max")
        assert (info["P"], info["batches"], info["per_device"]) == (P, 2, 16)
        info = LenetTraining.check(geom, (16, 200, 28, 28), (16, 200), 100, loss="huber", pool="max")
        assert (info["P"], info["Nt"], info["batch"]) == (P, 200, 100)
    for bad in ("min", "MAX", None, 1):
        with pytest.raises(ValueError, match="pool"):
            LenetValidation.check(MNIST_CNN32, (200, 28, 28), (200,), 100, pool=bad)
        with pytest.raises(ValueError, match="pool"):
            LenetTraining.check(MNIST_CNN32, (200, 28, 28), (200,), 100, pool=bad)
    # the default is the average pool
    assert LenetValidation.check(lc.LENET1, (200, 28, 28), (200,), 100)["P"] == 2202


GEOM = (12, 3, 2, 3, 4)
FAKE = 1 << 28  # never dereferenced: every call below is refused on the host


def _eval(**kw):
    from federated_amd import _lib
    a = dict(x=FAKE, xstride=0, labels=FAKE, lstride=0, Nt=7, geom=GEOM, models=FAKE, pitch=93, D=3, batch=3, batches=2,
             skip=None, target=0.5, ended=None, cost=FAKE, log=None, cap=0, epoch=None, ws=FAKE, ws_bytes=24, loss=0)
    a.update(kw)
    _lib.call("cfa_lenet_max_eval_loss_f32", a["x"], a["xstride"], a["labels"], a["lstride"], a["Nt"], *a["geom"],
              a["models"], a["pitch"], a["D"], a["batch"], a["batches"], a["skip"], a["target"], a["ended"], a["cost"],
              a["log"], a["cap"], a["epoch"], a["ws"], a["ws_bytes"], a["loss"], None)


def _grad(**kw):
    from federated_amd import _lib
    a = dict(x=FAKE, xstride=0, labels=FAKE, lstride=0, Nt=7, geom=GEOM, models=FAKE, pitch=93, D=3, src=None,
             first=None, batch=3, skip=None, grads=FAKE, gpitch=93, loss=None, ws=FAKE,
             ws_bytes=mc.grad_workspace_bytes(GEOM, 3, 3), kind=0)
    a.update(kw)
    _lib.call("cfa_lenet_max_grad_loss_f32", a["x"], a["xstride"], a["labels"], a["lstride"], a["Nt"], *a["geom"],
              a["models"], a["pitch"], a["D"], a["src"], a["first"], a["batch"], a["skip"], a["grads"], a["gpitch"],
              a["loss"], a["ws"], a["ws_bytes"], a["kind"], None)


INVALID, UNSUPPORTED = "CFA_E_INVALID", "CFA_E_UNSUPPORTED"


@pytest.mark.parametrize("kw, match, code", [
    (dict(loss=2, x=None), "unknown loss kind", INVALID),  # checked first, before any buffer
    (dict(x=None), "null buffer", INVALID), (dict(cost=None), "null buffer", INVALID),
    (dict(ws=None), "null buffer", INVALID), (dict(batches=0), "must be >= 1", INVALID),
    (dict(geom=(6, 3, 2, 3, 4)), "bad geometry", INVALID), (dict(batches=3), "do not fit", INVALID),
    (dict(pitch=92), "pitch", INVALID), (dict(xstride=7 * 144 - 1), "device strides", INVALID),
    (dict(log=FAKE), "together", INVALID), (dict(ws_bytes=23), "workspace of 23 bytes, 24 needed", INVALID),
    (dict(ended=FAKE, target=float("inf")), "finite", INVALID),
    (dict(geom=(12, 3, 2, 3, 65), pitch=1 << 20), "more than 64 classes", UNSUPPORTED),
    (dict(D=65536, ws_bytes=1 << 20), "more than 65535 devices", UNSUPPORTED),
    (dict(geom=(300, 3, 2, 3, 4), Nt=7, pitch=1 << 20), "do not fit one workgroup's LDS", UNSUPPORTED),
])
def test_eval_entry_validates_before_any_device_work(kw, match, code):
    from federated_amd import _lib
    with pytest.raises(_lib.CFAError, match=match) as e:
        _eval(**kw)
    assert e.value.code == getattr(_lib, code)


@pytest.mark.parametrize("kw, match, code", [
    (dict(kind=-1, grads=None), "unknown loss kind", INVALID),
    (dict(grads=None), "null buffer", INVALID), (dict(models=None), "null buffer", INVALID),
    (dict(batch=0), "must be >= 1", INVALID), (dict(geom=(12, 0, 2, 3, 4)), "bad geometry", INVALID),
    (dict(batch=8), "does not fit", INVALID), (dict(pitch=92), "pitch", INVALID), (dict(gpitch=92), "gpitch", INVALID),
    (dict(lstride=6), "device strides", INVALID),
    (dict(ws_bytes=mc.grad_workspace_bytes(GEOM, 3, 3) - 1), "workspace of 1211 bytes, 1212 needed", INVALID),
    (dict(geom=(12, 3, 2, 3, 65), pitch=1 << 20, gpitch=1 << 20), "more than 64 classes", UNSUPPORTED),
    (dict(D=65536), "more than 65535 devices", UNSUPPORTED),
    (dict(geom=(300, 3, 2, 3, 4), pitch=1 << 20, gpitch=1 << 20), "do not fit one workgroup's LDS", UNSUPPORTED),
])
def test_grad_entry_validates_before_any_device_work(kw, match, code):
    from federated_amd import _lib
    with pytest.raises(_lib.CFAError, match=match) as e:
        _grad(**kw)
    assert e.value.code == getattr(_lib, code)
