"""The completion word of the zero-copy drop-in calls (cfa_stream_signal / cfa_wait_signal,
consensus/_runtime._RowPlan.finish) on the GPU: the host returns only once the mix's
output is in pinned memory, whichever way the wait ends.

- the spin path (default): back-to-back calls on changing inputs, each result read right after
  the call, equal to the oracle (a wait that returned early would hand back the previous call's
  output);
- the fallback path: a zero spin budget goes straight to hipStreamSynchronize and must still see
  the word;
- hipStreamSynchronize alone (SIGNAL_COMPLETION off): the same values;
- TF1 (fp64 rows), the MEWMA update and the compression count through the same wait.
Reference rules: TF2 consensus_v3.py:153-155 (sequential fp32 mix), TF1 cfa.py:66-76,
cfa_ongraphs.py:225-273 (compression count), cfa_ge_2stage.py:594-606 (MEWMA).
"""
import numpy as np
import pytest

from oracle import cfa_oracle as O

pytestmark = pytest.mark.gpu

SHAPES = [(512, 32), (32,), (32, 8), (8,)]  # C1 (federated_sample_2NN_CFA.py), P = 16 680


def _model(rng, scale=1.0):
    return [(rng.standard_normal(s) * scale).astype(np.float32) for s in SHAPES]


@pytest.fixture
def runtime(monkeypatch):
    from federated_amd.consensus import _runtime as R
    monkeypatch.setattr(R, "SINGLE_ZERO_COPY", True)
    monkeypatch.setattr(R, "TF1_ZERO_COPY", True)
    return R


@pytest.mark.parametrize("mode", ["spin", "fallback", "synchronize"])
def test_back_to_back_calls_return_their_own_result(runtime, monkeypatch, mode):
    R = runtime
    monkeypatch.setattr(R, "SIGNAL_COMPLETION", mode != "synchronize")
    monkeypatch.setattr(R, "SIGNAL_SPIN_US", 0 if mode == "fallback" else 2000)
    rng = np.random.default_rng(4100)
    mx = R.mixer()
    for call in range(40):
        local, nbrs = _model(rng), [_model(rng) for _ in range(2)]
        al = [0.5, 1.0 / 3]
        got, _ = mx.mix(local, nbrs, al)
        for k in range(len(SHAPES)):
            want = O.sequential_mix(local[k], [x[k] for x in nbrs], al)
            assert got[k].dtype == np.float32 and np.array_equal(got[k].reshape(want.shape), want), (call, k)


def test_tf1_rows_and_compression_count_through_the_word(runtime):
    R = runtime
    rng = np.random.default_rng(4101)
    mx = R.mixer()
    for call in range(12):
        local, nbrs = _model(rng, 1e-3), [_model(rng, 1e-3) for _ in range(3)]
        al = [np.float64(0.25)] * 3
        got, kept = mx.mix_tf1(local, nbrs, [float(a) for a in al], compress=(2, 2))
        want = O.tf1_mix([x.copy() for x in local], nbrs, 1.0, al)
        want_kept = O.tf1_compress(want[2], local[2], 2)  # in place, returns counter_param
        for k in range(len(SHAPES)):
            assert np.array_equal(np.asarray(got[k], dtype=np.float64).reshape(np.shape(want[k])),
                                  np.asarray(want[k], dtype=np.float64)), (call, k)
        assert kept == want_kept, call


def test_mewma_through_the_word(runtime):
    R = runtime
    rng = np.random.default_rng(4102)
    mx = R.mixer()
    N = 2
    for call in range(6):
        W = [rng.standard_normal(s) for s in SHAPES]
        states = [rng.standard_normal(s + (N,)) for s in SHAPES]
        grads = [[rng.standard_normal(s) for s in SHAPES] for _ in range(N)]
        want_states = [s.copy() for s in states]
        want = O.tf1_mewma([w.copy() for w in W], want_states, grads, 0.99, 0.1, 0.2, True, False)
        got = mx.mewma_tf1(W, states, grads, 0.99, (0.1, 0.1, 0.2, 0.2), False, True)
        for k in range(len(SHAPES)):
            assert np.array_equal(np.asarray(got[k]).reshape(np.shape(want[k])), want[k]), (call, k)
            assert np.array_equal(states[k], want_states[k]), (call, k)
