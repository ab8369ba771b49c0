"""The CIFAR drivers' hidden-layer LeNet without a GPU: the family's geometry, the case table of
tests/lenet_hidden_cases.py (paths and seeds), its numpy restatement against an independent torch
CPU fp64 autograd and against central differences, and the host checks of LenetValidation /
LenetTraining and of the cfa_lenet_hidden_* entries, which refuse before any device work."""
import numpy as np
import pytest
import torch

import lenet_hidden_cases as hc

INVALID, UNSUPPORTED = "CFA_E_INVALID", "CFA_E_UNSUPPORTED"


def test_cifar_lenet_is_the_drivers_model():
    from federated_amd import tf2_training, tf2_validation
    from federated_amd.tf2_validation import CIFAR_LENET, _stages, lenet_layer_shapes, lenet_size
    assert CIFAR_LENET == hc.CIFAR_LENET == (32, 3, 5, 4, 8, 128, 10) and tf2_training.CIFAR_LENET == CIFAR_LENET
    assert "CIFAR_LENET" in tf2_validation.__all__ and "CIFAR_LENET" in tf2_training.__all__
    assert lenet_size(CIFAR_LENET) == 28130 == 304 + 808 + 25728 + 1290 == hc.size(CIFAR_LENET)
    shapes = lenet_layer_shapes(CIFAR_LENET)
    assert shapes == [(5, 5, 3, 4), (4,), (5, 5, 4, 8), (8,), (200, 128), (128,), (128, 10), (10,)] \
        == hc.layer_shapes(CIFAR_LENET)
    assert hc.stages(CIFAR_LENET) == (28, 14, 10, 5) and _stages(CIFAR_LENET) == (32, 5, 4, 8, 10, 5)
    for geom in [c[0] for c in hc.CASES.values()]:
        assert lenet_layer_shapes(geom) == hc.layer_shapes(geom) and lenet_size(geom) == hc.size(geom)
    # five numbers keep their six shapes
    assert len(lenet_layer_shapes((28, 5, 4, 8, 10))) == 6 and lenet_size((28, 5, 4, 8, 10)) == 2202


@pytest.mark.parametrize("name", sorted(hc.CASES) + sorted(hc.EVAL_CASES))
def test_every_case_is_on_its_path(name):
    for text, ok in hc.path(name).items():
        assert ok, (name, text)


@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_every_seed_is_the_smallest_by_the_rule(name):
    assert hc.smallest_seed(name) == hc.CASES[name][4]
    geom, _, Nt, D, seed = hc.CASES[name]
    x, _, models = hc.make(geom, D, Nt, seed)
    for row in models:
        lo, hi, shift = hc.decisions(x, row, geom)
        print(name, "smallest", lo, "largest", hi, "fp32 shift", shift)
        assert lo >= hc.GUARD * hi and shift <= 0.1 * lo


def _torch_loss(x, labels, tensors, loss):
    """The same layers in torch CPU fp64: NHWC -> NCHW, kernels (kh, kw, in, out) -> (out, in, kh, kw),
    and the Flatten in NHWC order."""
    F = torch.nn.functional
    K1, b1, K2, b2, Wh, bh, Wd, bd = tensors
    h = torch.from_numpy(np.asarray(x, dtype=np.float64)).permute(0, 3, 1, 2)
    h = F.avg_pool2d(torch.relu(F.conv2d(h, K1.permute(3, 2, 0, 1), b1)), 2)
    h = F.avg_pool2d(torch.relu(F.conv2d(h, K2.permute(3, 2, 0, 1), b2)), 2)
    flat = h.permute(0, 2, 3, 1).reshape(h.shape[0], -1)
    z = torch.matmul(torch.relu(torch.matmul(flat, Wh) + bh), Wd) + bd
    lp = F.log_softmax(z, dim=1)
    idx = torch.from_numpy(np.asarray(labels, dtype=np.int64))
    picked = lp.gather(1, idx[:, None])[:, 0]
    if loss == "huber":
        return F.huber_loss(picked.exp(), idx.double(), delta=1.0)
    return -picked.mean()


@pytest.mark.parametrize("loss", hc.LOSSES)
@pytest.mark.parametrize("name", hc.SMALL)
def test_the_restatement_agrees_with_torch_autograd(name, loss):
    geom, batch, Nt, D, _ = hc.CASES[name]
    x, labels, models = hc.data(name)
    for d in range(D):
        for first in (0, Nt - 1):
            idx = (np.arange(batch) + first) % Nt
            ts = [torch.tensor(t.astype(np.float64), requires_grad=True) for t in hc.split(models[d], geom)]
            value = _torch_loss(x[idx], labels[idx], ts, loss)
            value.backward()
            value = value.detach()
            ref = np.concatenate([t.grad.numpy().reshape(-1) for t in ts])
            got, got_value = hc.grads(x[idx], labels[idx], models[d], geom, loss)
            assert abs(got_value - float(value)) <= 1e-10 * max(1.0, abs(float(value)))
            assert abs(got_value - hc.loss_of(x[idx], labels[idx], models[d], geom, loss)) <= 1e-12
            for a, b in zip(hc.tensors(got, geom), hc.tensors(ref, geom)):
                assert np.max(np.abs(a - b)) <= 1e-10 * np.max(np.abs(b)), (name, loss, d)


@pytest.mark.parametrize("loss", hc.LOSSES)
@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_the_gradient_matches_central_differences(name, loss):
    geom, batch, Nt, D, _ = hc.CASES[name]
    x, labels, models = hc.data(name)
    row = models[0].astype(np.float64)
    g, _ = hc.grads(x[:batch], labels[:batch], row, geom, loss)
    rng = np.random.default_rng(7)
    o, eps = 0, 1e-6
    for shape in hc.layer_shapes(geom):
        n = int(np.prod(shape))
        for e in o + rng.choice(n, size=min(3, n), replace=False):
            hi, lo = row.copy(), row.copy()
            hi[e] += eps
            lo[e] -= eps
            fd = (hc.loss_of(x[:batch], labels[:batch], hi, geom, loss)
                  - hc.loss_of(x[:batch], labels[:batch], lo, geom, loss)) / (2 * eps)
            assert abs(fd - g[e]) <= 1e-6 * max(1.0, np.abs(g[o:o + n]).max()), (name, loss, shape, e, fd, g[e])
        o += n


@pytest.mark.parametrize("loss", hc.LOSSES)
def test_the_restated_epochs_take_the_path_they_exist_for(loss):
    """hc.drivers_epochs at hc.epochs_target: no flag in the first epoch (so its round is the eps-mix of
    three rows), exactly one raised by the second epoch's validation, that device takes no further step,
    a neighbour copies its row in that epoch's round, at least one device trains through all three
    epochs, and no cost the run compares with the target lies within the margin of it."""
    E, D = hc.EPOCHS, hc.CASES[hc.EPOCHS["case"]][3]
    target = hc.epochs_target(loss)
    models, cost, ended, history = hc.drivers_epochs(loss, target)
    flags = [h[1].tolist() for h in history]
    assert flags[0] == [0] * D and sum(flags[1]) == 1
    first = flags[1].index(1)
    assert history[-1][2][first] == E["steps"] and max(history[-1][2]) == E["steps"] * E["epochs"]
    assert np.isnan(history[2][0][first]) and cost[first] == history[1][0][first]
    assert any((models[d] == models[first]).all() for d in range(D) if d != first) or sum(flags[2]) < D
    for seen, _, _ in history:
        live = seen[~np.isnan(seen)]
        print(loss, "target", target, "costs", live, "relative distance", np.abs(live - target) / target)
        assert (np.abs(live - target) >= E["margin"] * target).all()
    row = np.arange(12.0).reshape(3, 4)
    lists = [[2, 1], [0, 2], [1, 0]]
    mixed = hc.tf2_round(row, np.zeros(3, dtype=np.int32), lists)
    w = row[0] + (row[2] - row[0]) / 3
    assert np.array_equal(mixed[0], w + (row[1] - w) / 3)
    copied = hc.tf2_round(row, np.array([0, 0, 1], dtype=np.int32), lists)
    assert np.array_equal(copied, row[[2, 2, 2]])


def test_workspace_bytes_and_params_without_a_device():
    from federated_amd import _lib
    lib = _lib.load()
    C = hc.CIFAR_LENET
    assert int(lib.cfa_lenet_hidden_params(*C)) == 28130
    for bad in ((32, 0, 5, 4, 8, 128, 10), (32, 3, 5, 4, 8, 0, 10), (12, 3, 5, 4, 8, 128, 10), (32, 3, 5, 4, 8, 128, 0)):
        assert int(lib.cfa_lenet_hidden_params(*bad)) == 0
        assert int(lib.cfa_lenet_hidden_grad_workspace_bytes(3, 4, *bad)) == 0
    for name, (geom, batch, _, D, _) in hc.CASES.items():
        assert int(lib.cfa_lenet_hidden_params(*geom)) == hc.size(geom)
        assert int(lib.cfa_lenet_hidden_grad_workspace_bytes(D, batch, *geom)) == hc.grad_workspace_bytes(geom, batch, D)
    assert int(lib.cfa_lenet_hidden_grad_workspace_bytes(16, 100, *C)) == 4 * 16 * 13 * 28138
    assert int(lib.cfa_lenet_hidden_grad_workspace_bytes(0, 4, *C)) == 0
    assert int(lib.cfa_lenet_hidden_eval_workspace_bytes(3, 5)) == 60
    assert int(lib.cfa_lenet_hidden_eval_workspace_bytes(3, 0)) == 0


def test_check_takes_seven_numbers():
    from federated_amd.tf2_training import LenetTraining
    from federated_amd.tf2_validation import CIFAR_LENET, LenetValidation
    info = LenetValidation.check(CIFAR_LENET, (10000, 32, 32, 3), (10000,), 100, target=0.5)
    assert (info["geom"], info["P"], info["batches"], info["per_device"]) == (CIFAR_LENET, 28130, 100, 0)
    info = LenetTraining.check(CIFAR_LENET, (16, 200, 32, 32, 3), (16, 200), 100, loss="huber")
    assert (info["P"], info["Nt"], info["batch"], info["per_device"]) == (28130, 200, 100, 16)
    one = (12, 1, 3, 2, 3, 6, 4)
    assert LenetTraining.check(one, (7, 12, 12, 1), (7,), 3)["P"] == hc.size(one)
    for check in (LenetValidation.check, LenetTraining.check):
        for x_shape, l_shape in (((200, 32, 32), (200,)),            # the channel axis is missing
                                 ((7, 12, 12), (7,)),
                                 ((200, 3, 32, 32), (200,)),         # NCHW
                                 ((2, 2, 200, 32, 32, 3), (2, 2, 200)),  # wrong rank
                                 ((200, 32, 32, 3), (199,))):
            geom = one if x_shape[1] == 12 else CIFAR_LENET
            with pytest.raises(ValueError, match="x must be"):
                check(geom, x_shape, l_shape, 2)
        with pytest.raises(ValueError, match="hidden"):
            check((32, 3, 5, 4, 8, 0, 10), (200, 32, 32, 3), (200,), 100)
        with pytest.raises(ValueError, match="p2 < 1"):
            check((12, 3, 5, 4, 8, 16, 10), (200, 12, 12, 3), (200,), 100)
        with pytest.raises(ValueError, match="pool"):
            check(CIFAR_LENET, (200, 32, 32, 3), (200,), 100, pool="max")
        with pytest.raises(ValueError, match="64 classes"):
            check((32, 3, 5, 4, 8, 128, 65), (200, 32, 32, 3), (200,), 100)
        with pytest.raises(ValueError, match="labels must lie"):
            check(CIFAR_LENET, (4, 32, 32, 3), (4,), 2, labels=np.array([0, 1, 10, 2]))
        with pytest.raises(ValueError, match="geom must be"):
            check(CIFAR_LENET[:6], (200, 32, 32, 3), (200,), 100)
    with pytest.raises(ValueError, match="does not fit"):
        LenetTraining.check(CIFAR_LENET, (4, 32, 32, 3), (4,), 5)
    with pytest.raises(ValueError, match="do not fit"):
        LenetValidation.check(CIFAR_LENET, (4, 32, 32, 3), (4,), 2, batches=3)
    with pytest.raises(ValueError, match="src must lie"):
        LenetTraining.check(CIFAR_LENET, (4, 32, 32, 3), (4,), 2, src=np.array([0, 3, 1]), D=3)
    # five numbers keep their shapes and their refusals
    assert LenetValidation.check((28, 5, 4, 8, 10), (200, 28, 28), (200,), 100)["P"] == 2202
    with pytest.raises(ValueError, match="x must be"):
        LenetValidation.check((28, 5, 4, 8, 10), (200, 28, 28, 1), (200,), 100)


GEOM = (12, 3, 3, 2, 3, 5, 4)  # P = 157, an image of 432 floats
P = hc.size(GEOM)
FAKE = 1 << 28  # never dereferenced: every call below is refused on the host
WS = hc.grad_workspace_bytes(GEOM, 3, 3)


def _eval(**kw):
    from federated_amd import _lib
    a = dict(x=FAKE, xstride=0, labels=FAKE, lstride=0, Nt=7, geom=GEOM, models=FAKE, pitch=P, D=3, batch=3, batches=2,
             skip=None, target=0.5, ended=None, cost=FAKE, log=None, cap=0, epoch=None, ws=FAKE, ws_bytes=24, loss=0)
    a.update(kw)
    _lib.call("cfa_lenet_hidden_eval_loss_f32", a["x"], a["xstride"], a["labels"], a["lstride"], a["Nt"], *a["geom"],
              a["models"], a["pitch"], a["D"], a["batch"], a["batches"], a["skip"], a["target"], a["ended"], a["cost"],
              a["log"], a["cap"], a["epoch"], a["ws"], a["ws_bytes"], a["loss"], None)


def _grad(**kw):
    from federated_amd import _lib
    a = dict(x=FAKE, xstride=0, labels=FAKE, lstride=0, Nt=7, geom=GEOM, models=FAKE, pitch=P, D=3, src=None,
             first=None, batch=3, skip=None, grads=FAKE, gpitch=P, loss=None, ws=FAKE, ws_bytes=WS, kind=0)
    a.update(kw)
    _lib.call("cfa_lenet_hidden_grad_loss_f32", a["x"], a["xstride"], a["labels"], a["lstride"], a["Nt"], *a["geom"],
              a["models"], a["pitch"], a["D"], a["src"], a["first"], a["batch"], a["skip"], a["grads"], a["gpitch"],
              a["loss"], a["ws"], a["ws_bytes"], a["kind"], None)


def _with(i, v):
    return GEOM[:i] + (v,) + GEOM[i + 1:]


def test_the_too_large_geometry_comes_from_the_lds_formula():
    assert hc.grad_lds_bytes(hc.TOO_LARGE, 1) > hc.LDS_LIMIT and hc.eval_lds_bytes(hc.TOO_LARGE, 1, 2) > hc.LDS_LIMIT
    assert 4 * 120 * 120 * 3 > hc.LDS_LIMIT and hc.grad_chunk(hc.TOO_LARGE) == 0 and hc.eval_chunk(hc.TOO_LARGE, 2) == 0


@pytest.mark.parametrize("kw, match, code", [
    (dict(loss=2, x=None), "unknown loss kind", INVALID),  # checked first, before any buffer
    (dict(x=None), "null buffer", INVALID), (dict(cost=None), "null buffer", INVALID),
    (dict(ws=None), "null buffer", INVALID), (dict(batches=0), "must be >= 1", INVALID),
    (dict(batches=0, geom=_with(5, 0)), "must be >= 1", INVALID),  # the counts before the geometry
    (dict(geom=_with(0, 6)), "bad geometry", INVALID), (dict(geom=_with(1, 0)), "bad geometry", INVALID),
    (dict(geom=_with(5, 0)), "hidden 0", INVALID), (dict(geom=_with(5, 0), batches=3), "bad geometry", INVALID),
    (dict(batches=3), "do not fit", INVALID), (dict(pitch=P - 1), "pitch", INVALID),
    (dict(xstride=7 * 432 - 1), "device strides", INVALID), (dict(lstride=6), "device strides", INVALID),
    (dict(log=FAKE), "together", INVALID), (dict(ws_bytes=23), "workspace of 23 bytes, 24 needed", INVALID),
    (dict(ended=FAKE, target=float("inf")), "finite", INVALID),
    (dict(geom=_with(6, 65), pitch=1 << 20), "more than 64 classes", UNSUPPORTED),
    (dict(D=65536, ws_bytes=1 << 20), "more than 65535 devices", UNSUPPORTED),
    (dict(geom=hc.TOO_LARGE, pitch=1 << 20), "do not fit one workgroup's LDS", UNSUPPORTED),
])
def test_eval_entry_validates_before_any_device_work(kw, match, code):
    from federated_amd import _lib
    with pytest.raises(_lib.CFAError, match=match) as e:
        _eval(**kw)
    assert e.value.code == getattr(_lib, code)


@pytest.mark.parametrize("kw, match, code", [
    (dict(kind=-1, grads=None), "unknown loss kind", INVALID),
    (dict(grads=None), "null buffer", INVALID), (dict(models=None), "null buffer", INVALID),
    (dict(batch=0), "must be >= 1", INVALID), (dict(geom=_with(2, 0)), "bad geometry", INVALID),
    (dict(geom=_with(5, 0)), "hidden 0", INVALID), (dict(geom=_with(5, -1), batch=8), "bad geometry", INVALID),
    (dict(batch=8), "does not fit", INVALID), (dict(pitch=P - 1), "pitch", INVALID),
    (dict(gpitch=P - 1), "gpitch", INVALID), (dict(xstride=7 * 432 - 1), "device strides", INVALID),
    (dict(ws_bytes=WS - 1), "workspace of %d bytes, %d needed" % (WS - 1, WS), INVALID),
    (dict(geom=_with(6, 65), pitch=1 << 20, gpitch=1 << 20), "more than 64 classes", UNSUPPORTED),
    (dict(D=65536), "more than 65535 devices", UNSUPPORTED),
    (dict(geom=hc.TOO_LARGE, pitch=1 << 20, gpitch=1 << 20, ws_bytes=0), "do not fit one workgroup's LDS", UNSUPPORTED),
])
def test_grad_entry_validates_before_any_device_work(kw, match, code):
    from federated_amd import _lib
    with pytest.raises(_lib.CFAError, match=match) as e:
        _grad(**kw)
    assert e.value.code == getattr(_lib, code)
