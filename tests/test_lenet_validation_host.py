"""The host half of the TF2 validation pass (federated_amd/tf2_validation.py) and the fp64
restatement the GPU tests compare against (tests/lenet_cases.py), without a GPU.

The restatement is pinned by a second implementation: torch's CPU conv2d / avg_pool2d in fp64,
with the Keras kernel (kh, kw, in, out) permuted to torch's (out, in, kh, kw) and the NCHW result
flattened in NHWC order. Parity against TensorFlow itself is not pinned (TensorFlow is not a
dependency of this repository)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lenet_cases as lc
from conftest import normwise_close
from federated_amd import _lib
from federated_amd.local_optim import layer_offsets
from federated_amd.tf2_validation import LENET1, LenetValidation, lenet_layer_shapes, lenet_size


def test_sizes():
    assert LENET1 == lc.LENET1 and lenet_size(LENET1) == 2202
    for geom, *_ in list(lc.CASES.values()) + [(lc.UNSUPPORTED,)]:
        shapes = lenet_layer_shapes(geom)
        assert len(shapes) == 6 and shapes == lc.layer_shapes(geom)
        assert lenet_size(geom) == sum(int(np.prod(s)) for s in shapes) == lc.size(geom)
        assert int(layer_offsets(shapes)[-1]) == lenet_size(geom)
        assert int(_lib.load().cfa_lenet_params(*geom)) == lenet_size(geom)
    assert lenet_size(lc.CASES["pool2_drops"][0]) == 93 and lenet_size(lc.UNSUPPORTED) == 34826
    assert lc.stages(lc.CASES["pool2_drops"][0])[2] == 3   # conv2 output 3: the pool drops one
    assert lc.stages(lc.CASES["pool1_drops"][0])[0] == 11  # conv1 output 11
    assert lc.stages(lc.CASES["map_1x1"][0])[3] == 1


def test_library_size_and_workspace_without_gpu():
    lib = _lib.load()
    assert lib.cfa_lenet_params(8, 5, 4, 8, 10) == 0      # p1 = 2 < kernel: no second map
    assert lib.cfa_lenet_params(28, 5, 0, 8, 10) == 0
    assert lib.cfa_lenet_params(28, 0, 4, 8, 10) == 0
    assert lib.cfa_lenet_eval_workspace_bytes(30, 100) == 30 * 100 * 4
    assert lib.cfa_lenet_eval_workspace_bytes(0, 100) == 0 and lib.cfa_lenet_eval_workspace_bytes(3, 0) == 0


def test_check_returns_the_plan():
    info = LenetValidation.check(LENET1, (10000, 28, 28), (10000,), 100)
    assert (info["P"], info["Nt"], info["batch"], info["batches"], info["per_device"]) == (2202, 10000, 100, 100, 0)
    info = LenetValidation.check(LENET1, (3, 250, 28, 28), (3, 250), 100, target=0.5)
    assert (info["batches"], info["per_device"], info["target"]) == (2, 3, 0.5)  # int(Nt / batch)
    assert LenetValidation.check((13, 4, 3, 5, 3), (7, 13, 13), (7,), 3, 2)["batches"] == 2


@pytest.mark.parametrize("kw", [
    dict(x_shape=(200, 28, 27)),                      # not side x side
    dict(x_shape=(200, 28)),
    dict(labels_shape=(199,)),                        # labels disagree with x
    dict(x_shape=(3, 200, 28, 28)),                   # per-device x with shared labels
    dict(batch=100, batches=3),                       # batch * batches > Nt
    dict(batch=201),                                  # batches = int(Nt / batch) = 0
    dict(batch=0),
    dict(geom=(8, 5, 4, 8, 10)),                      # p2 < 1
    dict(geom=(28, 5, 4, 8, 65)),                     # classes > 64
    dict(geom=(28, 5, 4, 8)),
    dict(geom=(28, 5, 0, 8, 10)),
    dict(target=float("nan")),
    dict(log_cap=-1),
    dict(labels=np.full(200, 10, dtype=np.int32)),    # label out of range
    dict(labels=np.full(200, -1, dtype=np.int32)),
    dict(labels=np.zeros(200, dtype=np.float32)),
])
def test_check_refuses(kw):
    args = dict(geom=LENET1, x_shape=(200, 28, 28), labels_shape=(200,), batch=100)
    args.update(kw)
    with pytest.raises(ValueError):
        LenetValidation.check(**args)


def _torch_log_probs(x, row, geom):
    K1, b1, K2, b2, Wd, bd = (torch.from_numpy(t.astype(np.float64)) for t in lc.split(row, geom))
    h = torch.from_numpy(x.astype(np.float64))[:, None]
    h = F.avg_pool2d(F.relu(F.conv2d(h, K1.permute(3, 2, 0, 1), b1)), 2)
    h = F.avg_pool2d(F.relu(F.conv2d(h, K2.permute(3, 2, 0, 1), b2)), 2)
    h = h.permute(0, 2, 3, 1).reshape(x.shape[0], -1)
    return torch.log_softmax(h @ Wd + bd, dim=1).numpy()


@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_restatement_against_torch_cpu_fp64(name):
    geom, batch, batches, Nt = lc.CASES[name]
    x, labels, models, ref = lc.reference(name, 3)
    n = batch * batches
    got = np.zeros(len(models))
    for d, row in enumerate(models):
        lp = _torch_log_probs(x[:n], row, geom)
        assert normwise_close(lc.log_probs(x[:n], row, geom), lp, 1e-10)
        got[d] = (-lp[np.arange(n), labels[:n]]).reshape(batches, batch).mean(axis=1).mean()
        print(name, d, "min probability", np.exp(lp).min(), "cost", got[d])
        assert np.exp(lp).min() > 1e-3  # fp32 underflows below 1e-38: far away
    assert normwise_close(ref, got, 1e-10)


def test_a_path_case_reaches_its_path():
    """The arithmetic of lc.path from the mirror of the launch plan: workgroups against batches for
    any device of up to 300 compute units, chunk tails, logit lanes against 256, LDS bytes against
    64 KiB; and that no earlier case is there."""
    for name in lc.PATHS:
        for cus in (1, 104, 256, 300):
            conditions = lc.path(name, lc.MANY_D, cus)
            assert conditions and all(conditions.values()), (name, cus, [k for k, v in conditions.items() if not v])
    assert lc.eval_grid_x(5, lc.MANY_D, 256) == 2  # batches 0, 2, 4 and 1, 3
    assert lc.eval_grid_x(100, 30, 256) == 34      # docs/history.md: 34 groups of 3 batches
    for name, (geom, batch, batches, _) in lc.CASES.items():
        if name not in lc.PATHS:
            assert lc.eval_grid_x(batches, 5, 104) == batches   # one batch per workgroup at the tests' D <= 5
            assert lc.eval_lds_bytes(geom, batch) <= lc.LDS_DEFAULT
            s1, _, s2, _ = lc.stages(geom)
            assert batch % lc.CHUNK in (0, 3) and (geom[1] != 5 or s1 % 2 == s2 % 2 == 0)
    assert lc.eval_lds_bytes(lc.LENET1, 100) == 4 * (2202 + 4 * (784 + 576 + 128 + 10) + 100)  # 33 KB
    assert lc.eval_lds_bytes(lc.UNSUPPORTED, 2) > 160 * 1024


def test_flag_rule_of_the_restatement():
    cost = np.array([0.4, 0.6, 0.2, 0.7])
    assert lc.flags(cost, 0.5).tolist() == [1, 0, 1, 0]
    assert lc.flags(cost, 0.5, before=[0, 1, 0, 0]).tolist() == [1, 1, 1, 0]   # a set flag stays set
    assert lc.flags(cost, 0.5, skip=[1, 0, 0, 0]).tolist() == [0, 0, 1, 0]     # a skipped device keeps its flag
