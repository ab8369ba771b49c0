"""The host half of the Huber objective of the TF2 LeNet-1 classes (`loss="huber"` of
tf2_validation.LenetValidation and tf2_training.LenetTraining) and the fp64 restatement the GPU
tests compare against (tests/lenet_huber_cases.py), without a GPU.

The restatement is pinned by a second implementation: torch's CPU autograd in fp64 through an
independent torch forward (conv2d, avg_pool2d, softmax, gather) and torch's own huber_loss with
the integer labels cast to double as the target, as the drivers hand them to keras.losses.Huber."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lenet_cases as lc
import lenet_grad_cases as gc
import lenet_huber_cases as hc
from conftest import ROOT, normwise_close
from federated_amd import _lib
from federated_amd.tf2_training import LENET1, LenetTraining
from federated_amd.tf2_validation import LenetValidation


def _torch_grads(x, labels, row, geom):
    ts = [torch.from_numpy(t.astype(np.float64)).requires_grad_() for t in lc.split(row, geom)]
    K1, b1, K2, b2, Wd, bd = ts
    h = torch.from_numpy(x.astype(np.float64))[:, None]
    h = F.avg_pool2d(F.relu(F.conv2d(h, K1.permute(3, 2, 0, 1), b1)), 2)
    h = F.avg_pool2d(F.relu(F.conv2d(h, K2.permute(3, 2, 0, 1), b2)), 2)
    h = h.permute(0, 2, 3, 1).reshape(x.shape[0], -1)
    lab = torch.from_numpy(labels.astype(np.int64))
    p = torch.softmax(h @ Wd + bd, dim=1).gather(1, lab[:, None])[:, 0]
    loss = F.huber_loss(p, lab.double(), delta=1.0)
    return [g.numpy().reshape(-1) for g in torch.autograd.grad(loss, ts)], float(loss.detach())


@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_restatement_against_torch_cpu_fp64_autograd(name):
    geom = hc.CASES[name][0]
    x, labels, models = hc.data(name)
    for shift, first in sorted(set(hc.batches_used(name))):
        idx = hc.batch_index(name, first, shift)
        for d in range(hc.D):
            want, wloss = _torch_grads(x[idx], labels[idx], models[d], geom)
            got, loss = hc.reference(name, d, first, shift)
            for i, (a, b) in enumerate(zip(gc.tensors(got, geom), want)):
                assert np.abs(b).max() > 0 and normwise_close(a, b, 1e-10), (name, d, first, shift, i)
            assert abs(loss - wloss) <= 1e-10 * abs(wloss)
            assert abs(hc.loss_of(x[idx], labels[idx], models[d], geom) - wloss) <= 1e-10 * abs(wloss)


def test_huber_is_keras_huber_at_delta_one():
    """The branch rule on its own: <= selects the quadratic branch, and at |e| = 1 both branches
    have the same value and slope, so a probability that saturates to 0 or 1 changes nothing."""
    e = np.array([-8.5, -1.5, -1.0, -0.25, 0.0, 0.25, 1.0, 1.5])
    h, g = hc.huber(e, np.zeros(len(e), dtype=np.int32))  # label 0: e = p
    assert h.tolist() == [8.0, 1.0, 0.5, 0.03125, 0.0, 0.03125, 0.5, 1.0]
    assert g.tolist() == [-1.0, -1.0, -1.0, -0.25, 0.0, 0.25, 1.0, 1.0]
    for l, p in ((0, 1.0), (1, 0.0), (2, 1.0)):  # the saturated cases: e = +-1
        e = p - l
        assert abs(e) == 1.0 and 0.5 * e * e == abs(e) - 0.5 and e == np.sign(e)


@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_every_batch_the_tests_use_holds_every_branch(name):
    """A label 0, a label 1 and, with more than two classes, a label >= 2 in every batch of
    hc.batches_used: the shared and per-device gradient batches, the batch positions (one wraps)
    and both validation batches of every set. And the case's label C - 1 (lenet1: 9)."""
    geom, batch, Nt, _ = hc.CASES[name]
    C = geom[4]
    _, labels, _ = hc.data(name)
    assert labels.dtype == np.int32 and labels.min() == 0 and labels.max() == C - 1
    used = hc.batches_used(name)
    assert {(s, 0) for s in hc.shifts(name)} <= set(used) and {(0, f) for f in hc.firsts(name)} <= set(used)
    assert {(s, b * batch) for s in hc.shifts(name) for b in range(hc.VAL_BATCHES)} <= set(used)
    assert any(f % Nt + batch > Nt for f in hc.firsts(name)) and hc.VAL_BATCHES * batch <= Nt
    xs, ls = hc.per_device(name)
    for d, s in enumerate(hc.shifts(name)):  # the per-device sets are the rolls `reference` indexes
        assert (ls[d] == labels[(np.arange(Nt) + s) % Nt]).all() and (xs[d, 0] == hc.data(name)[0][s % Nt]).all()
    for shift, first in used:
        got = labels[hc.batch_index(name, first, shift)]
        assert (got == 0).any() and (got == 1).any(), (name, shift, first, got)
        assert C == 2 or (got >= 2).any(), (name, shift, first, got)
    assert name != "lenet1" or 9 in labels


@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_the_seed_is_the_smallest_that_meets_the_rule(name):
    geom, batch, Nt, seed = hc.CASES[name]
    assert (geom, batch, Nt) == gc.CASES[name][:3]  # the shapes are the existing tables'
    assert [s for s in range(seed + 1) if hc.meets_the_seed_rule(name, s)] == [seed]
    x, _, models = hc.data(name)
    for d in range(hc.D):
        lo, hi = gc.margin(x, models[d], geom)
        assert lo >= gc.GUARD * hi and gc.preactivation_shift(x, models[d], geom) <= 0.1 * lo


def test_check_takes_the_loss_and_returns_the_same_plan():
    for cls, args in ((LenetTraining, (LENET1, (200, 28, 28), (200,), 100)),
                      (LenetValidation, (LENET1, (200, 28, 28), (200,), 100, 2, 0.5, 3))):
        plain = cls.check(*args)
        assert cls.check(*args, loss="xent") == plain and cls.check(*args, loss="huber") == plain
        for bad in ("l2", "Huber", "", None, 1):
            with pytest.raises(ValueError, match="loss"):
                cls.check(*args, loss=bad)


def test_the_classes_refuse_an_unknown_loss_before_any_device_call():
    """The loss is checked first: neither the tensors nor the engine are looked at (the Engine's
    own methods: test_gpu_lenet_huber.py)."""
    x, labels = torch.zeros(7, 12, 12), torch.zeros(7, dtype=torch.int32)
    with pytest.raises(ValueError, match="loss"):
        LenetValidation(None, (12, 3, 2, 3, 4), x, labels, 3, loss="l2")
    with pytest.raises(ValueError, match="loss"):
        LenetTraining(None, (12, 3, 2, 3, 4), x, labels, 3, loss="l2")
    assert _lib.LENET_LOSSES == {"xent": _lib.LENET_LOSS_XENT, "huber": _lib.LENET_LOSS_HUBER}


def test_an_unknown_kind_through_the_c_entry_points_is_invalid_without_gpu():
    """The library checks the kind before any buffer, on the host: CFA_E_INVALID with a message."""
    lib = _lib.load()
    for name in ("cfa_lenet_eval_loss_f32", "cfa_lenet_grad_loss_f32"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    with open(os.path.join(ROOT, "include", "cfa_engine.h")) as fh:
        text = fh.read()
    assert "CFA_LENET_LOSS_XENT = 0" in text and "CFA_LENET_LOSS_HUBER = 1" in text
    assert (_lib.LENET_LOSS_XENT, _lib.LENET_LOSS_HUBER) == (0, 1)
    for kind in (2, -1):
        with pytest.raises(_lib.CFAError, match="unknown loss kind") as e:
            _lib.call("cfa_lenet_eval_loss_f32", None, 0, None, 0, 7, 12, 3, 2, 3, 4, None, 93, 3, 3, 2, None, 0.0,
                      None, None, None, 0, None, None, 0, kind, None)
        assert e.value.code == _lib.CFA_E_INVALID
        with pytest.raises(_lib.CFAError, match="unknown loss kind") as e:
            _lib.call("cfa_lenet_grad_loss_f32", None, 0, None, 0, 7, 12, 3, 2, 3, 4, None, 93, 3, None, None, 3,
                      None, None, 93, None, None, 0, kind, None)
        assert e.value.code == _lib.CFA_E_INVALID
    # a known kind goes on to the buffers, under the name of the entry the caller used
    with pytest.raises(_lib.CFAError, match="cfa_lenet_grad_loss_f32: null buffer"):
        _lib.call("cfa_lenet_grad_loss_f32", None, 0, None, 0, 7, 12, 3, 2, 3, 4, None, 93, 3, None, None, 3, None,
                  None, 93, None, None, 0, _lib.LENET_LOSS_HUBER, None)
    with pytest.raises(_lib.CFAError, match="cfa_lenet_eval_f32: null buffer"):
        _lib.call("cfa_lenet_eval_f32", None, 0, None, 0, 7, 12, 3, 2, 3, 4, None, 93, 3, 3, 2, None, 0.0, None, None,
                  None, 0, None, None, 0, None)
