"""Topology schedules on the host (no GPU): the table layout ``schedule_csr`` emits for
cfa_mix_population_sched_f32 / _sched_tf1_f32, the schedule check of ``set_schedule``, and the
argument validation of the two entry points, which runs before any HIP call."""
import numpy as np
import pytest
import torch

from federated_amd import topology as T

D = 5
# three tables of different total length: an empty row (table 0, device 2), a repeated neighbour
# (table 1, device 0: random.choices draws with replacement), a single-neighbour table
TABLES = [
    [[1, 2], [0], [], [4, 0, 1], [3]],
    [[3, 3], [2, 0], [1], [0], [0, 1, 2, 3]],
    [[1], [2], [3], [4], [0]],
]


def _policy(nb, d, devices):  # distinct per entry, so a misplaced coefficient shows
    return [0.1 * (d + 1) + 0.01 * k + 0.001 * int(j) for k, j in enumerate(nb)]


def test_schedule_csr_is_the_per_table_csr_with_shifted_offsets():
    ptr, idx, coef = T.schedule_csr(TABLES, _policy, D)
    assert ptr.dtype == np.int32 and idx.dtype == np.int32 and coef.dtype == np.float32
    assert ptr.shape == (len(TABLES) * (D + 1),)
    parts = [T.csr(lists, _policy, D) for lists in TABLES]
    assert len({len(p[1]) for p in parts}) == len(TABLES)  # every table its own length
    off = 0
    for t, (p, i, c) in enumerate(parts):
        assert np.array_equal(ptr[t * (D + 1):(t + 1) * (D + 1)], p + off), t
        off += len(i)
    assert np.array_equal(idx, np.concatenate([p[1] for p in parts]))
    assert np.array_equal(coef, np.concatenate([p[2] for p in parts]))
    assert off == len(idx) == len(coef)
    # the rows themselves: the empty one holds the device alone, the repeated neighbour twice
    e = ptr[2]
    assert ptr[3] - e == 1 and idx[e] == 2 and coef[e] == 1.0
    e = ptr[D + 1]
    assert idx[e:ptr[D + 2]].tolist() == [0, 3, 3]


def test_csr_is_the_one_table_schedule():
    for lists in TABLES:
        for a, b in zip(T.csr(lists, T.alphas_tf2), T.schedule_csr([lists], T.alphas_tf2)):
            assert a.dtype == b.dtype and np.array_equal(a, b)
    p, i, c = T.csr(TABLES[0], T.alphas_tf2, D, np.float64)
    assert p.tolist() == [0, 3, 5, 6, 10, 12] and c.dtype == np.float64
    assert i.tolist() == [0, 1, 2, 1, 0, 2, 3, 4, 0, 1, 4, 3]


def _tf1_layout(lists, policy):
    """The Tf1PopulationRound table: local d with coefficient 0.0, neighbour j at D + j, fp64."""
    ptr, idx, coef = [0], [], []
    for d, nb in enumerate(lists):
        idx += [d] + [D + int(j) for j in nb]
        coef += [0.0] + [float(a) for a in policy(nb, d, D)]
        ptr.append(len(idx))
    return np.asarray(ptr, np.int32), np.asarray(idx, np.int32), np.asarray(coef, np.float64)


def test_tf1_layout_equals_set_topology_per_table():
    policy = T.alphas_tf1_ongraphs(0.7)
    sched = T.Tf1PopulationRound(None, D, 8, device="cpu")
    sched.set_schedule(TABLES, policy, sched=[2, 0, 1, 1])
    ptr, idx, coef = (a.numpy() for a in sched._csr)
    assert coef.dtype == np.float64 and ptr.shape == (len(TABLES) * (D + 1),)
    assert sched._sched[0].tolist() == [2, 0, 1, 1] and sched._sched[0].dtype == torch.int32
    assert sched._sched[1].tolist() == [0] and sched._sched[1].dtype == torch.int64
    for t, lists in enumerate(TABLES):
        one = T.Tf1PopulationRound(None, D, 8, device="cpu")
        one.set_topology(lists, policy)
        p, i, c = (a.numpy() for a in one._csr)
        wp, wi, wc = _tf1_layout(lists, policy)
        assert np.array_equal(p, wp) and np.array_equal(i, wi) and np.array_equal(c, wc), t
        assert (p.dtype, i.dtype, c.dtype) == (np.int32, np.int32, np.float64)
        tp = ptr[t * (D + 1):(t + 1) * (D + 1)]
        assert np.array_equal(tp - tp[0], p), t
        assert np.array_equal(idx[tp[0]:tp[-1]], i) and np.array_equal(coef[tp[0]:tp[-1]], c), t
    # set_topology afterwards: one table again, no schedule
    sched.set_topology(TABLES[1], policy)
    assert sched._sched is None and np.array_equal(sched._csr[0].numpy(), _tf1_layout(TABLES[1], policy)[0])


def _host_population():
    pr = T.PopulationRound.__new__(T.PopulationRound)  # its constructor wants CUDA buckets
    pr.models = torch.zeros(D, 8)
    return pr


@pytest.mark.parametrize("bad", [[0, 3], [-1], [0, 1, 2, 7], []])
def test_set_schedule_rejects_a_slot_outside_the_tables(bad):
    with pytest.raises(ValueError, match="outside the 3 tables|at least one slot"):
        T.Tf1PopulationRound(None, D, 8, device="cpu").set_schedule(TABLES, T.alphas_tf1_cfa(1.0, 2), sched=bad)
    with pytest.raises(ValueError, match="outside the 3 tables|at least one slot"):
        _host_population().set_schedule(TABLES, T.alphas_tf2, sched=bad)


def test_set_schedule_defaults_to_every_table_in_turn_and_checks_the_tables():
    pr = _host_population()
    pr.set_schedule(TABLES, T.alphas_tf2)
    assert pr._sched[0].tolist() == [0, 1, 2] and pr.window is None
    assert pr.tables[2].dtype == torch.float32
    pr.set_schedule(TABLES, T.alphas_tf1_ongraphs(1.0), numerics="tf1", compression=(2, 0, 4))
    assert pr.tables[2].dtype == torch.float64 and pr._compress == (2, 0, 4)
    with pytest.raises(ValueError, match="at least one table"):
        pr.set_schedule([], T.alphas_tf2)
    with pytest.raises(ValueError, match="5 neighbour lists"):
        pr.set_schedule([TABLES[0][:4]], T.alphas_tf2)
    with pytest.raises(ValueError, match="compression epilogue"):
        pr.set_schedule(TABLES, T.alphas_tf2, compression=(2, 0, 4))
    with pytest.raises(RuntimeError, match="set_schedule"):
        T.Tf1PopulationRound(None, D, 8, device="cpu").reset_round(1)


def test_scheduled_entry_points_validate_before_any_hip_call():
    """S = 0, T = 0, a null sched and a null round each return CFA_E_INVALID with a message (no
    GPU here: nothing is launched, no pointer is followed)."""
    from federated_amd import _lib
    p = 1 << 20  # stands for a device pointer: never dereferenced
    f32 = lambda sched, S, Tn, rnd: _lib.call("cfa_mix_population_sched_f32", p, p, p, p, p, sched, S, Tn, rnd, 4,
                                              _lib.RULE_SEQUENTIAL, 64, None)
    tf1 = lambda sched, S, Tn, rnd: _lib.call("cfa_mix_population_sched_tf1_f32", p, p, p, p, p, sched, S, Tn, rnd,
                                              4, 64, 0, 0, 0, None, None)
    for call in (f32, tf1):
        with pytest.raises(_lib.CFAError, match="schedule of 0 slots over 3 tables") as e:
            call(p, 0, 3, p)
        assert e.value.code == _lib.CFA_E_INVALID
        with pytest.raises(_lib.CFAError, match="schedule of 2 slots over 0 tables"):
            call(p, 2, 0, p)
        with pytest.raises(_lib.CFAError, match="schedule of -1 slots"):
            call(p, -1, 3, p)
        with pytest.raises(_lib.CFAError, match="null schedule or round counter"):
            call(None, 2, 3, p)
        with pytest.raises(_lib.CFAError, match="null schedule or round counter"):
            call(p, 2, 3, None)
        with pytest.raises(_lib.CFAError, match="null schedule or round counter"):
            call(None, 2, 3, None)
    with pytest.raises(_lib.CFAError, match="unknown rule 9"):
        _lib.call("cfa_mix_population_sched_f32", p, p, p, p, p, p, 2, 3, p, 4, 9, 64, None)
    # D == 0 or P == 0: nothing to mix, CFA_OK, nothing launched (the counter is not advanced)
    _lib.call("cfa_mix_population_sched_f32", p, p, p, p, p, p, 2, 3, p, 0, _lib.RULE_SEQUENTIAL, 64, None)
    _lib.call("cfa_mix_population_sched_f32", p, p, p, p, p, p, 2, 3, p, 4, _lib.RULE_SEQUENTIAL, 0, None)
    _lib.call("cfa_mix_population_sched_tf1_f32", p, p, p, p, p, p, 2, 3, p, 0, 64, 0, 0, 0, None, None)
    _lib.call("cfa_mix_population_sched_tf1_f32", p, p, p, p, p, p, 2, 3, p, 4, 0, 0, 0, 0, None, None)
