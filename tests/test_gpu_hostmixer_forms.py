"""Every HostMixer operation in both memory forms of its row plan (consensus/_runtime._RowPlan):
mapped (the kernel reads and writes the pinned rows over PCIe; the default) and staged (the same
rows through a device mirror: one H2D, the same launches, one D2H; ``SINGLE_ZERO_COPY`` /
``TF1_ZERO_COPY`` off). Each result is compared with the numpy oracle, bit for bit, and never
with the other form, so the staged side of the ``*_zero_copy_equals_staged`` tests has a
reference of its own.

One layout, P = 1577: odd, so the row pitch is padded for fp32 (1580) and for fp64 (1578) rows.
Fan-ins 1, 3 and 17 (above CFA_MAX_FANIN: two passes). Reference rules: TF2
consensus_v3.py:153-155 (sequential fp32 mix), parameter_server_v2.py:159-161 (FedAvg fold),
TF1 cfa.py:69-76 (fp32 first subtraction, fp64 after), cfa_ongraphs.py:225-273 (compression and
its count), cfa_ge_2stage.py:591-621 (MEWMA).
"""
import functools

import numpy as np
import pytest

from oracle import cfa_oracle as O

pytestmark = pytest.mark.gpu

SHAPES = [(3, 3, 1, 4), (4,), (255, 6), (7,)]
FANINS = [1, 3, 17]
LAYER, MODE = 2, 2  # compression of W2 (255 x 6), sparse DPCM: both branches taken in this regime


@functools.lru_cache(maxsize=None)
def _models(n, alternate=False):
    """(local, neighbours) close to one base model (so the DPCM threshold splits the layer);
    fp32, or with ``alternate`` every odd layer fp64. Shared by the tests: never written to."""
    rng = np.random.default_rng(8800 + n)
    base = [rng.standard_normal(s) * 0.01 for s in SHAPES]

    def model():
        return tuple((b + rng.standard_normal(b.shape) * 3e-4).astype(np.float64 if alternate and k % 2
                                                                       else np.float32)
                     for k, b in enumerate(base))
    local, nbrs = model(), tuple(model() for _ in range(n))
    for a in (local, *nbrs):
        for x in a:
            x.setflags(write=False)
    return local, nbrs


def _flat(models, k):
    return [m[k].reshape(-1) for m in models]


@pytest.fixture(params=["mapped", "staged"])
def mx(request, gpu, monkeypatch):
    from federated_amd.consensus import _runtime as R
    mapped = request.param == "mapped"
    monkeypatch.setattr(R, "SINGLE_ZERO_COPY", mapped)
    monkeypatch.setattr(R, "TF1_ZERO_COPY", mapped)
    return R.mixer()


def _same(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == SHAPES[k], (k, g.dtype, w.dtype)
        assert np.array_equal(g.reshape(-1), np.asarray(w).reshape(-1)), k


def _compressed(layers, local):
    """The oracle's epilogue on layer LAYER of ``layers`` (in place); returns the kept count."""
    seg = layers[LAYER].reshape(SHAPES[LAYER]).copy()
    kept = O.tf1_compress(seg, local[LAYER], MODE)
    layers[LAYER] = seg.reshape(-1)
    assert 0 < kept < seg.size
    return kept


def test_the_switch_selects_the_form(mx, request):
    from federated_amd.consensus import _runtime as R
    local, nbrs = _models(1)
    mx.mix(local, nbrs, [0.5])
    plan = mx._zc_plan("f32", R._layout_of(local), 1, np.float32, staged=not R.SINGLE_ZERO_COPY)
    assert plan.staged == ("staged" in request.node.name) and plan.pitch == 1580
    if plan.staged:
        assert (plan.hb, plan.ob) == (plan.dev.data_ptr(), plan.dev_out.data_ptr())


@pytest.mark.parametrize("n", FANINS)
def test_mix_plain(mx, n):
    local, nbrs = _models(n)
    al = [1.0 / (n + 1)] * n
    got, kept = mx.mix(local, nbrs, al)
    assert kept is None
    _same(got, [O.sequential_mix(local[k], [x[k] for x in nbrs], al) for k in range(len(SHAPES))])


@pytest.mark.parametrize("n", FANINS)
def test_mix_divisors(mx, n):
    local, nbrs = _models(n)
    got, kept = mx.mix(local, nbrs, [0.9] * n, divisors=[float(n)] * n)
    assert kept is None
    _same(got, O.ps_fedavg(list(local), [list(x) for x in nbrs], 0.9))


@pytest.mark.parametrize("n", FANINS)
@pytest.mark.parametrize("compress", [None, (MODE, LAYER)])
def test_mix_tf1_rule_on_fp32_rows(mx, n, compress):
    """mix(tf1=True): the TF1 chain (and its fp64 epilogue), rounded once to fp32."""
    local, nbrs = _models(n)
    al = [0.9 / (n + 1)] * n
    want = [O.tf1_mix_flat(local[k].reshape(-1), _flat(nbrs, k), al) for k in range(len(SHAPES))]
    want_kept = _compressed(want, local) if compress else None
    got, kept = mx.mix(local, nbrs, al, compress=compress, tf1=True)
    assert kept == want_kept
    _same(got, [w.astype(np.float32) for w in want])


@pytest.mark.parametrize("n", FANINS)
def test_mix_compress_fp32_rule(mx, n):
    """mix(compress=...): the fp32 sequential chain, then the epilogue as numpy evaluates it on
    fp32 arrays."""
    local, nbrs = _models(n)
    al = [1.0 / (n + 1)] * n
    want = [O.sequential_mix(local[k].reshape(-1), _flat(nbrs, k), al) for k in range(len(SHAPES))]
    want_kept = _compressed(want, local)
    got, kept = mx.mix(local, nbrs, al, compress=(MODE, LAYER))
    assert kept == want_kept
    _same(got, want)


@pytest.mark.parametrize("n", FANINS)
@pytest.mark.parametrize("compress", [None, (MODE, LAYER)])
@pytest.mark.parametrize("alternate", [False, True])
def test_mix_tf1(mx, n, compress, alternate):
    """mix_tf1 returns the reference's fp64 arrays. All-fp32 arrays: one wide launch in the mapped
    form, the fp64-row kernel in the staged one. Alternating fp32 / fp64 layers: four runs of one
    launch each, step 0 in fp32 only where local and first neighbour are both fp32 (numpy's own
    promotion, which the oracle gets from the arrays' dtypes)."""
    local, nbrs = _models(n, alternate)
    al = [0.9 / (n + 1)] * n
    want = [O.tf1_mix_flat(local[k].reshape(-1), _flat(nbrs, k), al) for k in range(len(SHAPES))]
    want_kept = _compressed(want, local) if compress else None
    got, kept = mx.mix_tf1(local, nbrs, al, compress=compress)
    assert kept == want_kept
    assert all(w.dtype == np.float64 for w in want)
    _same(got, want)


@pytest.mark.parametrize("n", FANINS)
@pytest.mark.parametrize("rule", [0, 2, 3])
def test_fold64(mx, n, rule):
    local = [np.asarray(a, dtype=np.float64) for a in _models(n)[0]]
    nbrs = [[np.asarray(a, dtype=np.float64) * (j + 2) for a in x] for j, x in enumerate(_models(n)[1])]
    al = [0.9] * n
    if rule == 0:
        want = [O.sequential_mix(local[k], [x[k] for x in nbrs], al) for k in range(len(SHAPES))]
    elif rule == 2:
        want = O.ps_fedavg(local, nbrs, 0.9)
    else:
        want = [a.copy() for a in local]
        for x in nbrs:
            want = [w + 0.9 * x[k] for k, w in enumerate(want)]
    last = np.concatenate([a.reshape(-1) for a in nbrs[-1]])
    fills = nbrs[:-1] + [lambda dst: np.copyto(dst, last)]  # a payload decoder writes its row itself
    got = mx.fold64(local, fills, al, rule, [float(n)] * n if rule == 2 else None)
    _same(got, want)


@pytest.mark.parametrize("n", FANINS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("init,use_filtered", [(False, True), (False, False), (True, False)])
def test_mewma_tf1(mx, n, dtype, init, use_filtered):
    rng = np.random.default_rng(8900 + n)
    N = n + 1  # the saved states hold one more slot than this call fills
    W = _models(n)[0]
    grads = [[rng.standard_normal(s).astype(dtype) for s in SHAPES] for _ in range(n)]
    states = [rng.standard_normal(s + (N,)).astype(dtype) for s in SHAPES]
    want_states = [s.copy() for s in states]
    want = O.tf1_mewma(list(W), want_states, grads, 0.99, 0.025, 0.001, use_filtered, init)
    got = mx.mewma_tf1(W, states, grads, 0.99, (0.025, 0.025, 0.001, 0.001), init, use_filtered)
    _same(got, want)
    assert got[0].dtype == dtype  # fp32 throughout stays fp32; fp64 updates widen the model
    for k, (s, w) in enumerate(zip(states, want_states)):
        assert s.dtype == dtype and np.array_equal(s, w), k


def test_mewma_tf1_without_gradients_launches_nothing(mx, monkeypatch):
    from federated_amd.consensus import _runtime as R

    def refuse(*a, **k):
        raise AssertionError("a launch with no gradient")
    monkeypatch.setattr(R._RowPlan, "launch", refuse)
    W = _models(1, alternate=True)[0]
    states = [np.ones(s + (2,)) for s in SHAPES]
    got = mx.mewma_tf1(W, states, [], 0.99, (0.1, 0.1, 0.2, 0.2), False, True)
    _same(got, W)
    assert [g.dtype for g in got] == [np.float32, np.float64, np.float32, np.float64]
    assert all(np.array_equal(s, np.ones_like(s)) for s in states)
