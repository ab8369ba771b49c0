"""oracle.cfa_ge_population_round against an independent replay of the reference's file protocol
(cfa_ge_2stage.py:388-621), both in float64 on the CPU.

The population oracle is the only whole-round reference of CfaGePopulation, and it was written
with the class. The replay below shares none of its bookkeeping: it keeps the reference's
per-epoch files as dictionaries, ``datamat[(i, e)]`` (four tensors) and ``datagrad[(i, e)]``
(four tensors with the reference's device-indexed last axis, zero-initialised, slot
``lists[i][n]`` written in list order), and composes only the oracle pieces that the golden
fixtures pin to the reference's own outputs: tf1_mix, tf1_cnn_grads / tf1_2nn_grads,
tf1_datagrad_slice and tf1_mewma. Device i reads slot i of ``datagrad[(j, e-1)]``, publishes its
pre-mix model, and evaluates its gradients at ``datamat[(j, e-1)]``. Which slot is read, what is
published, where the gradients are evaluated and the order of the neighbour updates are thus
decided twice, independently; the two must agree to 1e-12 normwise (float64 against float64).
"""
import numpy as np
import pytest

from conftest import normwise_close
from oracle import cfa_oracle as orc

CNN = {"filter": 5, "number": 3, "stride": 2, "input_data": 64, "classes": 2}   # P = 116, split 18
NN2 = {"intermediate_nodes": 2, "input_data": 8, "classes": 2}                  # P = 24, split 18

EPS, RHO, LR1, LR2 = 0.7, 0.9, 0.1, 0.03

GRAPHS = {
    "kregular": (5, 2, None),
    "ragged": (4, 2, [[1, 2, 1], [0], [3, 0], [1]]),  # asymmetric, duplicates, unequal lengths
    "isolated": (4, 2, [[1, 3], [0], [], [1, 0]]),    # device 2 lists nobody and nobody lists it
}


def _split4(v, shapes):
    offs = np.concatenate([[0], np.cumsum([int(np.prod(s)) for s in shapes])])
    return [np.asarray(v)[offs[k]:offs[k + 1]].reshape(shapes[k]) for k in range(4)]


def _flat4(t4):
    return np.concatenate([np.asarray(t).reshape(-1) for t in t4])


def _grads4(ml, geom, x, y, m4):
    if ml == 1:
        return orc.tf1_cnn_grads(x, y, *m4, stride=geom["stride"])[0]
    return orc.tf1_2nn_grads(x, y, *m4)[0]


def _replay_epoch(e, datamat, datagrad, local, states, lists, x, y, ml, geom, shapes, neighbors):
    """Epoch e of every device through the dictionaries; returns the new local models. ``states``
    [i][k] are the caller's saved-state arrays [..., Nmax], updated in place as the reference
    updates W_l1_saved / n_l1_saved / W_l2_saved / n_l2_saved."""
    D = len(lists)
    new = []
    for i in range(D):
        nb = [int(j) for j in lists[i]]
        factors = [orc.tf1_weight_factor(D, i, j, neighbors - 1) for j in nb]
        # stage 1 (:446-466) on the neighbours' files of epoch e - 1
        w4 = orc.tf1_mix(local[i], [datamat[(j, e - 1)] for j in nb], EPS, factors)
        # :468-478 the PRE-mix model is this epoch's file
        datamat[(i, e)] = [np.array(t) for t in local[i]]
        # :491-547 own gradients at the neighbours' epoch e - 1 models, slot j of [..., devices]
        gv = [np.zeros(tuple(s) + (D,)) for s in shapes]
        for j in nb:
            g = _grads4(ml, geom, x[i], y[i], datamat[(j, e - 1)])
            for k in range(4):
                gv[k][..., j] = np.asarray(g[k]).reshape(shapes[k])
        datagrad[(i, e)] = gv
        # :564-621 slot i of every neighbour's epoch e - 1 gradients, in list order
        got = [orc.tf1_datagrad_slice(datagrad[(j, e - 1)], i) for j in nb]
        w4 = orc.tf1_mewma(w4, states[i], got, RHO, LR1, LR2, use_filtered=(ml == 1), init=False)
        new.append([np.asarray(w4[k]).reshape(shapes[k]) for k in range(4)])
    return new


@pytest.mark.parametrize("graph", sorted(GRAPHS))
@pytest.mark.parametrize("ml", [1, 2])
def test_population_round_equals_file_protocol_replay(ml, graph):
    geom = CNN if ml == 1 else NN2
    D, neighbors, lists = GRAPHS[graph]
    if lists is None:
        lists = [orc.tf1_kregular(i, neighbors, D).tolist() for i in range(D)]
    assert len(lists) == D
    shapes = orc.tf1_flat_shapes(ml, geom)
    sizes = [int(np.prod(s)) for s in shapes]
    P = sum(sizes)
    assert P % 4 == 0 and (sizes[0] + sizes[1]) % 4 != 0
    Nmax = max(len(l) for l in lists)
    rng = np.random.default_rng(100 * ml + len(graph))
    B, L, C = 6, geom["input_data"], geom["classes"]
    x = rng.standard_normal((D, B, L)).astype(np.float32)
    y = np.eye(C, dtype=np.float32)[rng.integers(0, C, (D, B))]
    f32 = lambda a: a.astype(np.float32).astype(np.float64)  # the driver's fp32 TF variables
    W = f32(rng.standard_normal((D, P)) * 0.1)
    pub = f32(rng.standard_normal((D, P)) * 0.1)
    S = rng.standard_normal((D, Nmax, P)) * 0.01
    G = rng.standard_normal((D, Nmax, P)) * 0.01

    # the replay's files of epoch 0 and its per-device states
    datamat = {(i, 0): _split4(pub[i], shapes) for i in range(D)}
    datagrad = {}
    for i in range(D):
        gv = [np.zeros(tuple(s) + (D,)) for s in shapes]
        for n, j in enumerate(lists[i]):  # list order: a repeated neighbour's later slot overwrites
            for k, t in enumerate(_split4(G[i, n], shapes)):
                gv[k][..., j] = t
        datagrad[(i, 0)] = gv
    states = [[np.stack([_split4(S[i, n], shapes)[k] for n in range(Nmax)], axis=-1) for k in range(4)]
              for i in range(D)]
    local = [_split4(W[i], shapes) for i in range(D)]

    oW, opub, oS, oG = W, pub, S, G
    for e in range(1, 4):
        local = _replay_epoch(e, datamat, datagrad, local, states, lists, x, y, ml, geom, shapes, neighbors)
        oW, oS, oG, opub = orc.cfa_ge_population_round(oW, opub, oG, oS, lists, x, y, ml, geom, EPS, neighbors,
                                                       RHO, LR1, LR2)
        for i in range(D):
            assert normwise_close(_flat4(local[i]), oW[i], 1e-12), ("W", e, i)
            assert normwise_close(_flat4(datamat[(i, e)]), opub[i], 1e-12), ("pub", e, i)
            for n, j in enumerate(lists[i]):
                s = _flat4([states[i][k][..., n] for k in range(4)])
                assert normwise_close(s, oS[i, n], 1e-12), ("S", e, i, n)
                g = _flat4([datagrad[(i, e)][k][..., j] for k in range(4)])
                assert normwise_close(g, oG[i, n], 1e-12), ("G", e, i, n)
            for n in range(len(lists[i]), Nmax):  # slots beyond the list: untouched state, no gradient
                assert np.array_equal(oS[i, n], S[i, n]) and not oG[i, n].any(), ("pad", e, i, n)
            unlisted = [j for j in range(D) if j not in lists[i]]
            assert not any(datagrad[(i, e)][k][..., unlisted].any() for k in range(4)), ("slots", e, i)
        # the driver: the results go into fp32 TF variables, then one (stand-in) local SGD step
        drift = rng.standard_normal((D, P)) * 0.01
        oW = f32(f32(oW) + drift)
        local = [_split4(f32(f32(_flat4(local[i])) + drift[i]), shapes) for i in range(D)]
