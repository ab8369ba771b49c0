"""The host half of the TF2 local batches (federated_amd/tf2_training.py) and the fp64 backward
restatement the GPU tests compare against (tests/lenet_grad_cases.py), without a GPU.

The restatement is pinned by a second implementation: torch's CPU autograd in fp64 through an
independent torch forward (conv2d, avg_pool2d, log_softmax), the Keras kernel (kh, kw, in, out)
permuted to torch's (out, in, kh, kw) and the NCHW result flattened in NHWC order."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lenet_cases as lc
import lenet_grad_cases as gc
from conftest import normwise_close
from federated_amd import _lib
from federated_amd.tf2_training import LENET1, LenetTraining, lenet_size


def _torch_grads(x, labels, row, geom):
    ts = [torch.from_numpy(t.astype(np.float64)).requires_grad_() for t in lc.split(row, geom)]
    K1, b1, K2, b2, Wd, bd = ts
    h = torch.from_numpy(x.astype(np.float64))[:, None]
    h = F.avg_pool2d(F.relu(F.conv2d(h, K1.permute(3, 2, 0, 1), b1)), 2)
    h = F.avg_pool2d(F.relu(F.conv2d(h, K2.permute(3, 2, 0, 1), b2)), 2)
    h = h.permute(0, 2, 3, 1).reshape(x.shape[0], -1)
    loss = F.nll_loss(torch.log_softmax(h @ Wd + bd, dim=1), torch.from_numpy(labels.astype(np.int64)))
    return [g.numpy().reshape(-1) for g in torch.autograd.grad(loss, ts)], float(loss.detach())


@pytest.mark.parametrize("name", sorted(gc.CASES))
def test_restatement_against_torch_cpu_fp64_autograd(name):
    geom, batch, Nt, _ = gc.CASES[name]
    x, labels, models = gc.data(name)
    for d in range(gc.D):
        for first in (0, Nt - 1):  # the second batch wraps
            idx = (np.arange(batch) + first) % Nt
            want, wloss = _torch_grads(x[idx], labels[idx], models[d], geom)
            got, loss = gc.reference(name, d, first)
            for i, (a, b) in enumerate(zip(gc.tensors(got, geom), want)):
                assert np.abs(b).max() > 0 and normwise_close(a, b, 1e-10), (name, d, first, i)
            assert abs(loss - wloss) <= 1e-10 * abs(wloss)


@pytest.mark.parametrize("name", sorted(gc.CASES))
def test_no_relu_gate_is_within_rounding_of_its_threshold(name):
    """Over every model and every sample of the case's set (any batch a test draws lies inside):
    the smallest |pre-activation| is at least 1e-5 of the largest, and an fp32 evaluation moves
    a pre-activation by at most a tenth of that margin."""
    geom = gc.CASES[name][0]
    x, _, models = gc.data(name)
    for d in range(gc.D):
        lo, hi = gc.margin(x, models[d], geom)
        shift = gc.preactivation_shift(x, models[d], geom)
        print(name, d, "smallest", lo, "largest", hi, "ratio", lo / hi, "fp32 shift", shift)
        assert lo >= gc.GUARD * hi
        assert shift <= 0.1 * lo


@pytest.mark.parametrize("name", gc.PATHS)
def test_a_path_case_reaches_its_path_with_the_smallest_seed_that_meets_the_rule(name):
    """The arithmetic of gc.path (items against 256 lanes, logit lanes against 256, P + 1 against a
    finish block, LDS bytes against 64 KiB) from the mirror of the launch plan, and the seed derived
    again from the restatement alone: no smaller one meets the margin rule with every tensor's
    gradient non-zero on every batch of the set."""
    conditions = gc.path(name)
    print(name, gc.plan(name))
    assert conditions and all(conditions.values()), [k for k, v in conditions.items() if not v]
    geom, batch, Nt, seed = gc.CASES[name]
    assert [s for s in range(seed + 1) if gc.meets_the_seed_rule(geom, batch, Nt, s)] == [seed]
    assert int(_lib.load().cfa_lenet_params(*geom)) == lc.size(geom) == lenet_size(geom)


def test_the_lane_plans_of_the_cases():
    """lenet_lanes over the table: the earlier cases reach 1 to 32 lanes a weight-gradient sum, never
    more items than threads; the PATHS cases add 64 lanes (fewer rows than lanes) and one lane with
    more items than threads, a second pass of lenet_logits, a third group and LDS above 64 KiB."""
    assert [gc.lanes(n) for n in (1, 4, 5, 8, 9, 20, 36, 128, 129, 256, 257)] == [64, 64, 32, 32, 16, 8, 4, 2, 1, 1, 1]
    before = {L for n in gc.CASES if n not in gc.PATHS for L in gc.plan(n)["L"]}
    assert before == {32, 16, 8, 4, 1} and gc.plan("lenet1")["L"] == (8, 1) and gc.plan("generic_k")["L"] == (16, 4)
    assert max(i for n in gc.CASES if n not in gc.PATHS for i in gc.plan(n)["items"]) <= gc.BLOCK
    assert max(gc.plan(n)["logit_lanes"] for n in gc.CASES if n not in gc.PATHS) <= gc.BLOCK
    assert max(gc.plan(n)["groups"] for n in gc.CASES if n not in gc.PATHS) == 2
    assert all(gc.plan(n)["lds"] <= lc.LDS_DEFAULT for n in gc.CASES if n != "raised_lds")
    # cfa_lenet_graph.h's 39.9 KiB: 2 * 2 202 + 2 * (784 + 1 152 + 256 + 20 + 512) + 4 + 2 + 352 floats
    assert gc.plan("lenet1")["lds"] == 4 * 10210 == 40840


def test_check_returns_the_plan():
    info = LenetTraining.check(LENET1, (60000, 28, 28), (60000,), 100)
    assert (info["P"], info["Nt"], info["batch"], info["per_device"]) == (2202, 60000, 100, 0)
    assert info["P"] == lenet_size(LENET1) and info["geom"] == LENET1
    info = LenetTraining.check(LENET1, (3, 250, 28, 28), (3, 250), 250, labels=np.zeros((3, 250), dtype=np.int32),
                               src=np.array([1, 2, 0]))
    assert (info["Nt"], info["batch"], info["per_device"]) == (250, 250, 3)  # batch == Nt is a batch
    LenetTraining.check(LENET1, (200, 28, 28), (200,), 100, src=[4, 0, 1, 2, 3], D=5)


@pytest.mark.parametrize("kw", [
    dict(x_shape=(200, 28, 27)),                      # not side x side
    dict(x_shape=(200, 28)),
    dict(labels_shape=(199,)),                        # labels disagree with x
    dict(x_shape=(3, 200, 28, 28)),                   # per-device x with shared labels
    dict(batch=201),                                  # batch > Nt
    dict(batch=0),
    dict(geom=(8, 5, 4, 8, 10)),                      # p2 < 1
    dict(geom=(28, 5, 4, 8, 65)),                     # classes > 64
    dict(geom=(28, 5, 4, 8)),
    dict(geom=(28, 5, 0, 8, 10)),
    dict(labels=np.full(200, 10, dtype=np.int32)),    # label out of range
    dict(labels=np.full(200, -1, dtype=np.int32)),
    dict(labels=np.zeros(200, dtype=np.float32)),
    dict(src=[0, 1, 3], D=3),                         # src out of range
    dict(src=[-1, 1, 2], D=3),
    dict(src=[0, 1], D=3),                            # one entry per device
    dict(src=[0.0, 1.0, 2.0], D=3),
    dict(src=[0, 1, 2]),                              # a shared set says nothing about D
    dict(D=0),
    dict(x_shape=(3, 200, 28, 28), labels_shape=(3, 200), D=4),  # D disagrees with the per-device set
])
def test_check_refuses(kw):
    args = dict(geom=LENET1, x_shape=(200, 28, 28), labels_shape=(200,), batch=100)
    args.update(kw)
    with pytest.raises(ValueError):
        LenetTraining.check(**args)


def test_library_exports_and_workspace_without_gpu():
    lib = _lib.load()
    for name in ("cfa_lenet_grad_f32", "cfa_lenet_grad_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    ws = lib.cfa_lenet_grad_workspace_bytes
    assert ws(0, 100, *LENET1) == 0 and ws(30, 0, *LENET1) == 0 and ws(-1, -1, *LENET1) == 0
    assert ws(30, 100, 8, 5, 4, 8, 10) == 0  # no such model
    one = ws(1, 1, *LENET1)
    assert one >= 2202 * 4 and one % 4 == 0
    # proportional to D, and a function of the batch alone beyond that: no smaller for a larger batch
    assert ws(30, 1, *LENET1) == 30 * one
    sizes = [ws(1, b, *LENET1) for b in (1, 2, 6, 100)]
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0]
