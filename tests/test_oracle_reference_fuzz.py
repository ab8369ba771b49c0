"""Randomised differential check of the CPU oracle against the reference's own consensus modules.

The golden fixtures (tests/golden/*.npz) pin the oracle on fixed cases. This test holds seeded
random cases those fixtures do not: device counts, neighbour counts, eps values, layer shapes,
neighbour lists and training_end flags, and requires the oracle to reproduce every output of the
reference's own modules bit for bit. What the reference returned for each case is recorded in
tests/golden/reference_fuzz/<test>.npz (outputs only: the inputs are drawn again from the case's
seed), so the test needs nothing outside the repository. The recordings are made where the
reference tree is present (CFA_REFERENCE, default as in tests/golden/make_golden.py), with its TF
stubs and temporary working directory; nothing of the reference is copied into the repo:

    CFA_FUZZ_RECORD=1 python -m pytest tests/test_oracle_reference_fuzz.py

- TF1 cfa.py (a1, TF1/consensus/cfa.py:35-154): k-regular neighbours, epoch-0 publish then an
  epoch-1 mix, fp64 results under numpy 2 (and the reference's UnboundLocalError for a device
  left without a neighbour, which the drop-ins reproduce: test_tf1_no_neighbour.py);
- TF2 consensus_v3 weights (a5, consensus_v3.py:73-159) with the eps override and the
  training_end transfer, and consensus_v4 gradients (a6, consensus_v4.py:219-260) with the
  caller's eps.

It checks the checker; the GPU tests then compare the kernels with the oracle.
"""
import importlib.util
import os
import sys

import numpy as np
import pytest

from oracle import cfa_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("cfa_make_golden", os.path.join(ROOT, "tests", "golden", "make_golden.py"))
MG = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MG)

FUZZ_DIR = os.path.join(ROOT, "tests", "golden", "reference_fuzz")
RECORD = os.environ.get("CFA_FUZZ_RECORD") == "1"
_recorded = {}  # test function -> {"<case>/<i>": array, "<case>/n": count}, written when the module ends
_stored = {}


def _observe(request, run):
    """What the reference returned for this case, as a list of arrays: read from the recording, or
    (CFA_FUZZ_RECORD=1, reference tree present) from ``run()``, which is then recorded."""
    func = request.node.originalname
    case = request.node.name[len(func):].strip("[]") or "-"
    if RECORD:
        obs = [np.asarray(a) for a in run()]
        rec = _recorded.setdefault(func, {})
        rec[f"{case}/n"] = np.asarray(len(obs))
        for i, a in enumerate(obs):
            rec[f"{case}/{i}"] = a
        return obs
    if func not in _stored:
        with np.load(os.path.join(FUZZ_DIR, func + ".npz"), allow_pickle=False) as z:
            _stored[func] = {k: z[k] for k in z.files}
    z = _stored[func]
    return [z[f"{case}/{i}"] for i in range(int(z[f"{case}/n"]))]


RAISED, RETURNED = np.asarray(1), np.asarray(0)  # how a reference call that may raise ended

_REF_FILES = {"cfa": (MG.TF1, "consensus", "cfa.py"),
              "v3": (MG.TF2, "MNIST_dataset", "consensus", "consensus_v3.py"),
              "v4": (MG.TF2, "MNIST_dataset", "consensus", "consensus_v4.py")}


class _Modules(dict):
    """The reference's modules, loaded on first use (only a recording run uses them)."""

    def __missing__(self, name):
        self[name] = MG.load_ref(os.path.join(*_REF_FILES[name]), "fuzz_ref_" + name)
        return self[name]


_STUBBED = ("tensorflow", "tensorflow.keras", "tensorflow.keras.layers", "tensorflow.keras.models", "keras",
            "keras.utils")


@pytest.fixture(scope="module")
def ref():
    saved = {k: sys.modules.get(k) for k in _STUBBED}
    if RECORD:
        MG.install_stubs()
    try:
        yield _Modules()
        if RECORD:
            os.makedirs(FUZZ_DIR, exist_ok=True)
            for func, rec in _recorded.items():
                path = os.path.join(FUZZ_DIR, func + ".npz")
                if os.path.isfile(path):  # a run of some cases only keeps the other cases' recordings
                    with np.load(path, allow_pickle=False) as z:
                        rec = {**{k: z[k] for k in z.files if k.split("/")[0] not in {c.split("/")[0] for c in rec}},
                               **rec}
                np.savez_compressed(path, **rec)
    finally:
        for k, v in saved.items():  # the stubs must not leak into the rest of the session
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def _shapes(rng):
    a, b, c = (int(x) for x in rng.integers(1, 48, size=3))
    return [(a, b), (b,), (b, c), (c,)]


@pytest.mark.parametrize("seed", range(8))
def test_tf1_cfa_random_configs(ref, request, seed):
    rng = np.random.default_rng(9100 + seed)
    K = int(rng.integers(3, 10))
    N = int(rng.integers(1, min(5, K)))
    eps = float(rng.uniform(0.05, 1.0))
    shapes = _shapes(rng)
    scale = float(rng.choice([1e-3, 1.0, 30.0]))
    e0 = [MG.gen_model(rng, shapes, scale) for _ in range(K)]
    e1 = [MG.gen_model(rng, shapes, scale) for _ in range(K)]

    def run():  # per device: its neighbour list, how the epoch-1 call ended, its four results
        obs = []
        with MG.Workdir():
            procs = [ref["cfa"].CFA_process(True, K, j, N) for j in range(K)]
            for j in range(K):
                W1, b1, W2, b2 = e0[j]
                procs[j].getFederatedWeight(W1, W2, b1, b2, 0, np.zeros(3), eps)
            for ii in range(K):
                W1, b1, W2, b2 = e1[ii]
                obs.append(np.asarray(procs[ii].neighbor_vec))
                try:
                    res = procs[ii].getFederatedWeight(W1, W2, b1, b2, 1, np.zeros(3), eps)
                except UnboundLocalError:
                    obs.append(RAISED)
                    continue
                obs += [RETURNED] + [np.asarray(res[t]) for t in range(4)]
        return obs
    obs = iter(_observe(request, run))
    for ii in range(K):
        nbr = O.tf1_kregular(ii, N, K)
        assert nbr.tolist() == next(obs).tolist(), (K, N, ii)
        # N = 1 leaves interior devices without a neighbour: the reference fails with
        # UnboundLocalError (test_tf1_no_neighbour.py: so do the drop-ins)
        assert int(next(obs)) == (RAISED if nbr.size == 0 else RETURNED), (K, N, ii)
        if nbr.size == 0:
            continue
        wf = [O.tf1_weight_factor(K, ii, int(j), N - 1) for j in nbr]
        got = O.tf1_mix(e1[ii], [e0[int(j)] for j in nbr], eps, wf)
        for t in range(4):
            want = next(obs)
            assert got[t].dtype == want.dtype, (K, N, ii, t)
            assert np.array_equal(np.asarray(got[t]).reshape(want.shape), want), (K, N, ii, t)
    assert next(obs, None) is None


@pytest.mark.parametrize("seed", range(8))
def test_tf2_v3_weights_and_v4_grads_random_configs(ref, request, seed):
    rng = np.random.default_rng(9200 + seed)
    D = int(rng.integers(4, 11))
    n = int(rng.integers(1, min(6, D)))
    shapes = [(int(x),) if i % 2 else (int(x), int(y)) for i, (x, y) in enumerate(rng.integers(1, 40, size=(4, 2)))]
    models = [MG.gen_model(rng, shapes) for _ in range(D)]
    grads = [MG.gen_model(rng, shapes, 0.1) for _ in range(D)]
    local = MG.gen_model(rng, shapes)
    local_g = MG.gen_model(rng, shapes, 0.1)
    nbr = [int(j) for j in rng.choice(np.arange(1, D), size=n, replace=False)]
    ended = {int(rng.choice(nbr))} if rng.random() < 0.4 else set()
    eps = float(rng.uniform(0.05, 0.95))

    def run():  # the mixed weights, then the mixed gradients, one array per layer
        with MG.Workdir():
            for k in range(D):
                MG.publish_tf2(k, models[k], 10, k in ended, grads[k])
            p3 = ref["v3"].CFA_process(D, 0, 2)
            loc = MG.obj_array([a.copy() for a in local])
            p3.update_local_model(loc)
            res_w = p3.federated_weights_computing(nbr, n, 10, eps, 0, 30)
            p4 = ref["v4"].CFA_process(D, 0, 2)
            p4.update_local_model(MG.obj_array([a.copy() for a in local]))
            gl = MG.obj_array([a.copy() for a in local_g])
            p4.update_local_gradient(gl)
            # consensus_v4.py:225-246: one neighbour is passed as a scalar id (the ring rule's form)
            res_g = p4.federated_grads_computing(nbr if n > 1 else nbr[0], n, 10, eps, 1)
        return [np.asarray(res_w[t]) for t in range(len(shapes))] + [np.asarray(res_g[t]) for t in range(len(shapes))]
    obs = _observe(request, run)
    assert len(obs) == 2 * len(shapes)
    res_w, res_g = obs[:len(shapes)], obs[len(shapes):]
    # both stop loading at the first neighbour that reports training_end (v3 :139-141, v4 :233-235)
    upto = next((i + 1 for i, j in enumerate(nbr) if j in ended), len(nbr))
    want_w = O.tf2_weights(local, [models[j] for j in nbr[:upto]], training_end=bool(ended))
    for t in range(len(shapes)):
        assert np.array_equal(np.asarray(res_w[t]), want_w[t]), (D, n, sorted(ended), t)
    want_g = O.tf2_grads_v4(local_g, [grads[j] for j in nbr[:upto]], eps)
    for t in range(len(shapes)):
        assert np.array_equal(np.asarray(res_g[t]), want_g[t]), (D, n, t)


@pytest.mark.parametrize("fast", [True, False])
def test_tf1_cfa_ge_without_neighbour_raises_in_the_reference(ref, request, fast):
    """The case test_tf1_no_neighbour.py pins for the drop-in: the reference's CFA-GE negotiation
    (cfa_ge_2stage.py:388-470 fast, :129-211 4-stage) fails with UnboundLocalError when the
    device has no neighbour (N = 1, interior device), before it publishes its epoch-1 model."""
    rng = np.random.default_rng(9300 + int(fast))
    K, ii, epoch = 5, 2, 1
    W1, b1, W2, b2 = MG.gen_model(rng, MG.SHAPES_CNN_GE)

    def run():  # the device's neighbour list, how the call ended, whether it published its model
        ge = MG.load_ref(os.path.join(MG.TF1, "consensus", "cfa_ge_2stage.py"), "fuzz_ref_cfa_ge")
        with MG.Workdir():
            p = ge.CFA_ge_process(True, K, ii, 1, 0.99)
            p.setCNNparameters(16, 8, 5, 5, 21, 8, 512)
            conn = np.asarray(p.get_connectivity(ii, 1, K))
            st = [np.zeros(tuple(s) + (1,)) for s in MG.SHAPES_CNN_GE]
            fn = p.getFederatedWeight_gradients_fast if fast else p.getFederatedWeight_gradients
            try:
                fn(W1, W2, b1, b2, epoch, np.zeros(3), 0, None, None, st[0], st[2], st[1], st[3], 1.0, 0.1, 0.05)
                ended = RETURNED
            except UnboundLocalError:
                ended = RAISED
            return [conn, ended, np.asarray(int(os.path.isfile(f"datamat{ii}_{epoch}.mat")))]
    conn, ended, published = _observe(request, run)
    assert conn.size == 0 and O.tf1_kregular(ii, 1, K).size == 0
    assert int(ended) == RAISED and int(published) == 0


@pytest.mark.parametrize("seed", range(10))
def test_tf1_ongraphs_mode1_random_configs(ref, request, seed):
    """cfa_ongraphs.py:152-314, consensus mode 1 with the caller's neighbour list (graph != 0):
    random device, neighbour list, eps and compression mode on models in the regime the
    compression thresholds act on; the oracle's fp64 chain, epilogue and counter_param match."""
    rng = np.random.default_rng(9400 + seed)
    K = 5  # the vGraph.mat fixture's device count
    ii = int(rng.integers(0, K))
    others = [j for j in range(K) if j != ii]
    nb = [int(j) for j in rng.choice(others, size=int(rng.integers(1, K)), replace=False)]
    eps = float(rng.uniform(0.1, 1.0))
    comp = int(rng.integers(0, 5))
    m0 = MG.ongraphs_models(rng, K, MG.SHAPES_ONGRAPHS_SMALL)
    m1 = MG.ongraphs_models(rng, K, MG.SHAPES_ONGRAPHS_SMALL)
    def run():  # the four results and counter_param
        og = MG.load_ref(os.path.join(MG.TF1, "consensus", "cfa_ongraphs.py"), "fuzz_ref_ongraphs")
        with MG.Workdir():
            procs = [og.CFA_process(True, K, j, 2, 6, comp, 1) for j in range(K)]
            for j in range(K):
                W1, b1, W2, b2 = m0[j]
                procs[j].getFederatedWeight(W1, W2, b1, b2, 0, np.zeros(3), eps, [], False)
            W1, b1, W2, b2 = [a.copy() for a in m1[ii]]
            res = procs[ii].getFederatedWeight(W1, W2, b1, b2, 1, np.zeros(3), eps, nb, False)
        return [np.asarray(res[t]) for t in range(4)] + [np.asarray(int(res[4]))]
    res = _observe(request, run)
    assert len(res) == 5
    local = [a.copy() for a in m1[ii]]
    wf = [O.tf1_weight_factor(K, ii, j, len(nb)) for j in nb]
    out = O.tf1_mix(local, [m0[j] for j in nb], eps, wf)
    counter = O.tf1_compress(out[2], local[2], comp)
    for t in range(4):
        want = np.asarray(res[t])
        assert np.array_equal(np.asarray(out[t]).reshape(want.shape), want), (ii, nb, comp, t)
    assert counter == int(res[4]), (ii, nb, comp)


@pytest.mark.parametrize("seed", range(8))
def test_parameter_server_v2_random_configs(ref, request, seed):
    """parameter_server_v2.py:83-164 FedAvg: the active devices of column ``epoch`` of indexes_tx,
    p <- p + u (x_k - p) / C in order, or the transfer from the first device reporting
    training_end (:150-157); random device counts, active sets, update factors and ended flags."""
    rng = np.random.default_rng(9500 + seed)
    D = int(rng.integers(3, 10))
    active = int(rng.integers(1, D + 1))
    epochs = 4
    indexes_tx = np.stack([rng.permutation(D)[:active] for _ in range(epochs)], axis=1)
    epoch = int(rng.integers(0, epochs))
    u = float(rng.uniform(0.5, 1.0))
    shapes = [(int(x),) if i % 2 else (int(x), int(y)) for i, (x, y) in enumerate(rng.integers(1, 30, size=(4, 2)))]
    models = [MG.gen_model(rng, shapes) for _ in range(D)]
    glob_ = MG.gen_model(rng, shapes)
    chosen = [int(k) for k in indexes_tx[:, epoch]]
    ended = {int(rng.choice(chosen))} if rng.random() < 0.3 else set()
    def run():  # the aggregated global model, one array per layer
        ps2 = MG.load_ref(os.path.join(MG.TF2, "MNIST_dataset", "consensus", "parameter_server_v2.py"), "fuzz_ref_ps2")
        with MG.Workdir():
            for k in range(D):
                MG.publish_tf2(k, models[k], 10, k in ended)
            p = ps2.Parameter_Server(D, MG.obj_array([a.copy() for a in glob_]), active, indexes_tx, update_factor=u)
            res = p.federated_target_weights_aggregation(epoch, 0)
        return [np.asarray(res[t]) for t in range(len(shapes))]
    res = _observe(request, run)
    assert len(res) == len(shapes)
    if ended:
        first = next(k for k in chosen if k in ended)
        want = O.ps_fedavg(glob_, [models[first]], u, divide=False)
    else:
        want = O.ps_fedavg(glob_, [models[k] for k in chosen], u)
    for t in range(len(shapes)):
        assert np.array_equal(np.asarray(res[t]), want[t]), (D, active, epoch, sorted(ended), t)


@pytest.mark.parametrize("seed", range(6))
def test_cfa_ge_random_configs(ref, request, seed):
    """cfa_ge_2stage.py: the fast negotiation (:388-635) and the 4-stage one (:129-385, epoch 1
    initialises the states, later epochs filter them): stage-1 mix with the previous epoch's
    models, then the MEWMA / SGD update from the neighbours' gradient slots, random K, N, rho,
    eps and learning rates, CNN geometry of federated_sample_CNN_CFA-GE.py:36-42."""
    rng = np.random.default_rng(9600 + seed)
    variant = ("fast", "4stage_e1", "4stage_e3")[seed % 3]
    K = int(rng.integers(4, 10))
    N = int(rng.integers(2, min(5, K)))
    ii = int(rng.integers(0, K))
    rho, eps = float(rng.uniform(0.5, 0.999)), float(rng.uniform(0.2, 1.0))
    lr1, lr2 = float(rng.uniform(0.01, 0.2)), float(rng.uniform(0.01, 0.2))
    epoch = {"fast": int(rng.integers(1, 6)), "4stage_e1": 1, "4stage_e3": 3}[variant]
    shapes = MG.SHAPES_CNN_GE
    prev = [MG.gen_model(rng, shapes) for _ in range(K)]
    cur = [MG.gen_model(rng, shapes) for _ in range(K)]
    grads = [[rng.standard_normal(tuple(s) + (K,)) for s in shapes] for _ in range(K)]
    local = MG.gen_model(rng, shapes)
    states = [rng.standard_normal(tuple(s) + (N,)) for s in shapes]
    grad_epoch = epoch - 1 if variant == "fast" else epoch

    def run():  # the device's neighbour list, the four results, the four updated states
        ge = MG.load_ref(os.path.join(MG.TF1, "consensus", "cfa_ge_2stage.py"), f"fuzz_ref_cfa_ge_{seed}")
        with MG.Workdir():
            p = ge.CFA_ge_process(True, K, ii, N, rho)
            p.setCNNparameters(16, 8, 5, 5, 21, 8, 512)
            nbr = np.asarray(p.get_connectivity(ii, N, K))
            for j in range(K):
                W1, b1, W2, b2 = prev[j]
                MG.sio.savemat(f"datamat{j}_{epoch - 1}.mat", {"weights1": W1, "biases1": b1, "weights2": W2, "biases2": b2})
                if variant != "fast" and j != ii:
                    W1, b1, W2, b2 = cur[j]
                    MG.sio.savemat(f"datamat{j}_{epoch}.mat", {"weights1": W1, "biases1": b1, "weights2": W2, "biases2": b2})
                g = grads[j]
                MG.sio.savemat(f"datagrad{j}_{grad_epoch}.mat", {"grad_weights1": g[0], "grad_biases1": g[1],
                                                                "grad_weights2": g[2], "grad_biases2": g[3],
                                                                "epoch": grad_epoch})
            st = [s.copy() for s in states]
            W1, b1, W2, b2 = local
            fn = p.getFederatedWeight_gradients_fast if variant == "fast" else p.getFederatedWeight_gradients
            res = fn(W1, W2, b1, b2, epoch, np.zeros(3), 0, None, None, st[0], st[2], st[1], st[3], eps, lr1, lr2)
        return [nbr] + [np.asarray(r) for r in res[:8]]
    obs = _observe(request, run)
    assert len(obs) == 9
    nbr, res = obs[0], obs[1:]
    assert nbr.tolist() == O.tf1_kregular(ii, N, K).tolist()
    wf = [O.tf1_weight_factor(K, ii, int(j), N - 1) for j in nbr]
    W = O.tf1_mix(local, [prev[int(j)] for j in nbr], eps, wf)
    ost = [s.copy() for s in states]
    # the update reads slot ii of each neighbour's [..., devices] gradient (cfa_ge_2stage.py:575-589)
    W = O.tf1_mewma(W, ost, [[g[..., ii] for g in grads[int(j)]] for j in nbr], rho, lr1, lr2,
                    variant == "fast", variant == "4stage_e1")
    for t in range(4):
        want = np.asarray(res[t])
        assert np.array_equal(np.asarray(W[t]).reshape(want.shape), want), (variant, K, N, ii, t)
    for t, r in zip((0, 2, 1, 3), res[4:8]):
        assert np.array_equal(ost[t], np.asarray(r)), (variant, K, N, ii, "state", t)
