"""Host side of the FedAvg population round: ``topology.active_schedule`` (the active tables of
``cfa_fedavg_population_round_f32`` from the reference's ``indexes_tx`` or from ragged lists) and
the argument checks of ``FedAvgPopulation.set_schedule`` (``check_schedule``, its host half). No
GPU."""
import numpy as np
import pytest

from federated_amd import topology as T
from federated_amd.fedavg_population import FedAvgPopulation


def test_indexes_tx_columns_become_tables():
    """parameter_server_v2.py:88: active_devices = indexes_tx[:, epoch]. Column e is table e, in
    row order, duplicates kept; offsets are absolute."""
    tx = np.array([[3, 0, 5],
                   [1, 0, 2],
                   [4, 2, 2],
                   [0, 5, 1]], dtype=np.int64)  # A = 4 active devices, E = 3 epochs
    ptr, idx, div, rdiv = T.active_schedule(tx, 6)
    assert ptr.dtype == np.int32 and idx.dtype == np.int32 and div.dtype == np.float32 and rdiv.dtype == np.float64
    assert ptr.tolist() == [0, 4, 8, 12]
    assert idx.tolist() == [3, 1, 4, 0, 0, 0, 2, 5, 5, 2, 2, 1]
    for e in range(3):
        assert idx[ptr[e]:ptr[e + 1]].tolist() == tx[:, e].tolist()
    assert div.tolist() == [4.0, 4.0, 4.0] and rdiv.tolist() == [0.25, 0.25, 0.25]


def test_ragged_lists_with_an_empty_one():
    lists = [[2, 0, 1], [], [4], [1, 1, 3, 0, 2, 4, 4]]
    ptr, idx, div, rdiv = T.active_schedule(lists, 5)
    assert ptr.tolist() == [0, 3, 3, 4, 11]
    assert idx.tolist() == [2, 0, 1, 4, 1, 1, 3, 0, 2, 4, 4]
    for t, ids in enumerate(lists):
        assert idx[ptr[t]:ptr[t + 1]].tolist() == ids
        if ids:
            assert div[t] == np.float32(float(len(ids)))
            assert rdiv[t] == 1.0 / float(len(ids))  # the arithmetic of set_reciprocals: 1.0 / (double)d
    # the empty list's divisor is never used, but the kernel loads it: finite, and so is 1 / it
    assert np.isfinite(div[1]) and np.isfinite(rdiv[1]) and div[1] != 0


def test_reciprocals_are_the_fp64_reciprocal_of_the_fp32_count():
    lists = [list(range(c)) for c in (1, 3, 7, 17, 100)]
    _, _, div, rdiv = T.active_schedule(lists, 100)
    for c, d, r in zip((1, 3, 7, 17, 100), div, rdiv):
        assert d == np.float32(c) and r == np.float64(1.0) / np.float64(np.float32(c))


@pytest.mark.parametrize("lists", [[[0, 5]], [[-1]], [[0], [1, 2, 7]], np.array([[0, 1], [2, 5]])])
def test_out_of_range_ids_are_refused(lists):
    with pytest.raises(ValueError, match="outside"):
        T.active_schedule(lists, 5)


def test_indexes_tx_must_be_a_2d_integer_array():
    with pytest.raises(ValueError, match="2-D"):
        T.active_schedule(np.zeros(4, dtype=np.int64), 5)
    with pytest.raises(ValueError, match="2-D"):
        T.active_schedule(np.zeros((2, 2), dtype=np.float32), 5)


def test_set_schedule_argument_errors():
    chk = FedAvgPopulation.check_schedule
    lists = [[0, 1], [2]]
    with pytest.raises(ValueError, match="client must be"):
        chk(3, lists, client="average")
    for bad in (0.0, 1e-60, float("inf"), float("nan"), 1e60):  # zero, or not finite, once in fp32
        with pytest.raises(ValueError, match="client_divisor"):
            chk(3, lists, client="mix", client_divisor=bad)
    chk(3, lists, client="copy", client_divisor=0.0)  # unused by the copy client
    with pytest.raises(ValueError, match="outside"):
        chk(2, lists)
    with pytest.raises(ValueError, match="at least one table"):
        chk(3, [])
    with pytest.raises(ValueError, match="at least one slot"):
        chk(3, lists, sched=[])
    with pytest.raises(ValueError, match=r"sched\[1\] = 2"):
        chk(3, lists, sched=[0, 2])
    with pytest.raises(ValueError, match=r"sched\[0\] = -1"):
        chk(3, lists, sched=[-1])


def test_check_schedule_returns_the_upload():
    (ptr, idx, div, rdiv), sched, client = FedAvgPopulation.check_schedule(
        4, [[3, 3, 0], [1]], sched=None, client="mix", client_factor=1, client_divisor=2)
    assert ptr.tolist() == [0, 3, 4] and idx.tolist() == [3, 3, 0, 1] and sched == [0, 1]
    assert div.tolist() == [3.0, 1.0] and rdiv.tolist() == [1.0 / 3.0, 1.0]
    assert client[1:] == (1.0, 2.0)
    # every list empty: the index table still has an entry to upload
    (ptr, idx, _, _), sched, _ = FedAvgPopulation.check_schedule(4, [[], []], sched=[1, 1, 0])
    assert ptr.tolist() == [0, 0, 0] and idx.size == 1 and sched == [1, 1, 0]
