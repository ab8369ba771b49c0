"""CPU checks of the fused round's host logic: how a shard's devices split into runs, the size
gate, and that an engine without ring_slide keeps one mix per device."""
import pytest
import torch

from federated_amd.population import (INFINITY_CACHE_BYTES, RingPopulationShard, RingShardPlan, scattered_order,
                                      split_runs, window_exceeds_cache)


def test_whole_ring_is_one_run():
    assert split_runs(list(range(6)), lambda i: True) == [([0, 1, 2, 3, 4, 5], True)]


def test_interior_run_between_boundary_devices():
    plan = RingShardPlan(1, 4, 10, 3, 2)
    runs = split_runs(plan.interior() + plan.boundary(), lambda i: not plan.needs_halo(i))
    assert runs == [([3, 4, 5, 6, 7], True), ([0], False), ([1], False), ([2], False), ([8], False), ([9], False)]


def test_gaps_descending_and_repeated_devices_cut_runs():
    whole = lambda i: True  # noqa: E731
    assert split_runs([0, 1, 3, 4, 5, 7], whole) == [([0, 1], True), ([3, 4, 5], True), ([7], True)]
    assert split_runs([5, 4, 3], whole) == [([5], True), ([4], True), ([3], True)]
    assert split_runs([2, 2, 3], whole) == [([2], True), ([2, 3], True)]
    assert split_runs([4, 5, 0, 1], whole) == [([4, 5], True), ([0, 1], True)]
    assert split_runs([], whole) == []


def test_a_device_that_needs_the_halo_splits_a_run():
    assert split_runs([0, 1, 2, 3, 4], lambda i: i != 2) == [([0, 1], True), ([2], False), ([3, 4], True)]


def test_single_device_and_scattered_order():
    assert split_runs([7], lambda i: True) == [([7], True)]
    order = scattered_order(list(range(64)), 2)
    assert all(len(run) == 1 for run, _ in split_runs(order, lambda i: True))


def test_size_gate_is_the_infinity_cache():
    assert INFINITY_CACHE_BYTES == 256 * 2**20
    assert window_exceeds_cache(25_000_000, 8)
    assert not window_exceeds_cache(1_000_000, 8)
    edge = INFINITY_CACHE_BYTES // (9 * 4)
    assert not window_exceeds_cache(edge, 8) and window_exceeds_cache(edge + 1, 8)


class StubEngine:
    """An engine of the per-device round only (no ring_slide)."""

    def __init__(self):
        self.mixed = []

    def prepare_mix_seq(self, out, local, nbrs, alphas):
        def launch(stream=None):
            self.mixed.append(int(out.data_ptr()))
        return launch


@pytest.mark.parametrize("fused", ["auto", True, False])
def test_stub_engine_takes_the_per_device_path(fused):
    L, P = 6, 16
    eng = StubEngine()
    shard = RingPopulationShard(RingShardPlan(0, 1, L, 1), P, "cpu", None, eng, fused=fused)
    assert not shard.fuses()
    seen = []
    shard._mix_set(shard.interior_order(), None, lambda i, start: seen.append((i, start)))
    assert eng.mixed == [int(shard.mixed[i].data_ptr()) for i in range(L)]
    assert seen == [(i, s) for i in range(L) for s in (True, False)]


def test_mix_runs_fuses_only_runs_of_two_or_more():
    shard = RingPopulationShard(RingShardPlan(0, 2, 6, 2, 2), 16, "cpu", None, StubEngine())
    assert shard.mix_runs([2, 3, 0, 1, 4, 5]) == [([2, 3], True), ([0], False), ([1], False), ([4], False),
                                                  ([5], False)]
    assert shard.mix_runs([2]) == [([2], False)]
    assert shard.mix_runs([3, 2]) == [([3], False), ([2], False)]


def test_fused_argument_is_checked():
    with pytest.raises(ValueError):
        RingPopulationShard(RingShardPlan(0, 1, 4, 1), 16, "cpu", None, None, fused="yes")
