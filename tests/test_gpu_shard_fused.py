"""RingPopulationShard's fused round (one cfa_mix_ring_slide_f32 call per run of consecutive
devices whose windows lie in the shard's stack) against the per-device round and the oracle."""
import numpy as np
import pytest
import torch

from federated_amd.population import RingPopulationShard, RingShardPlan, scattered_order
from oracle.cfa_oracle import sequential_mix

pytestmark = pytest.mark.gpu

WORLD1 = [(9, 4, 4, 1028), (13, 4, 4, 24624), (12, 2, 2, 4100), (10, 1, 0, 4096), (7, 0, 2, 1028), (5, 0, 0, 260),
          (128, 4, 4, 4096), (9, 4, 4, 4), (9, 4, 4, 2_000_148)]


class Counting:
    """The engine with its ring_slide and prepare_mix_seq calls recorded."""

    def __init__(self, eng):
        self._eng, self.slides, self.prepared = eng, [], []

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def ring_slide(self, out, models, alphas, first, count, hl, hr, stream=None):
        self.slides.append((int(first), int(count)))
        return self._eng.ring_slide(out, models, alphas, first, count, hl, hr, stream)

    def prepare_mix_seq(self, out, local, nbrs, alphas):
        self.prepared.append(out.data_ptr())
        return self._eng.prepare_mix_seq(out, local, nbrs, alphas)


def _fill(shard, D):
    """A global population [D, P] (host) with this shard's rows and halo rows filled from it."""
    p = shard.plan
    rng = np.random.default_rng(D * 1009 + shard.P + 10 * p.hl + p.hr)
    pop = rng.standard_normal((D, shard.P)).astype(np.float32)
    shard.models.copy_(torch.from_numpy(pop[p.first:p.first + p.L]))
    if p.world > 1:
        for q in range(p.hl):
            shard.halo["left"][q].copy_(torch.from_numpy(pop[(p.first - p.hl + q) % D]))
        for q in range(p.hr):
            shard.halo["right"][q].copy_(torch.from_numpy(pop[(p.first + p.L + q) % D]))
    shard.mixed.fill_(float("nan"))
    return pop


def _oracle(plan, pop, alphas):
    return np.stack([sequential_mix(pop[g], [pop[j] for j in plan.neighbours(g)], alphas)
                     for g in range(plan.first, plan.first + plan.L)])


@pytest.mark.parametrize("L,hl,hr,P", WORLD1)
def test_fused_round_equals_per_device_round_and_oracle(gpu, L, hl, hr, P):
    plan = RingShardPlan(0, 1, L, hl, hr)
    eng = Counting(gpu)
    fused = RingPopulationShard(plan, P, torch.device("cuda"), None, eng, fused=True)
    pop = _fill(fused, L)
    plain = RingPopulationShard(plan, P, torch.device("cuda"), None, gpu, fused=False,
                                stacks=(fused.models, torch.full((L, P), float("nan"), device="cuda")))
    fused.round()
    plain.round()
    torch.cuda.synchronize()
    assert eng.slides == [(0, L)] and not eng.prepared
    got = fused.mixed.cpu().numpy()
    assert np.array_equal(got, plain.mixed.cpu().numpy())
    assert np.array_equal(got, _oracle(plan, pop, fused.alphas))


@pytest.mark.parametrize("rank", [0, 1])
def test_world2_interior_fused_boundary_per_device(gpu, rank):
    L, hl, hr, P = 11, 3, 2, 4100
    plan = RingShardPlan(rank, 2, L, hl, hr)
    eng = Counting(gpu)
    shard = RingPopulationShard(plan, P, torch.device("cuda"), None, eng, fused=True)
    pop = _fill(shard, 2 * L)
    shard.compute_round()
    torch.cuda.synchronize()
    assert eng.slides == [(hl, L - hl - hr)]
    assert len(eng.prepared) == hl + hr  # the boundary devices, one mix each
    assert np.array_equal(shard.mixed.cpu().numpy(), _oracle(plan, pop, shard.alphas))


def test_scattered_order_takes_no_fused_call(gpu):
    L, h, P = 64, 1, 1028
    plan = RingShardPlan(0, 1, L, h)
    eng = Counting(gpu)
    shard = RingPopulationShard(plan, P, torch.device("cuda"), None, eng, fused=True)
    pop = _fill(shard, L)
    shard.mix_order = scattered_order(plan.interior(), plan.K)
    assert all(b != a + 1 for a, b in zip(shard.mix_order, shard.mix_order[1:]))
    shard.round()
    torch.cuda.synchronize()
    assert not eng.slides and len(eng.prepared) == L
    assert np.array_equal(shard.mixed.cpu().numpy(), _oracle(plan, pop, shard.alphas))


def test_timer_sees_one_start_and_one_end(gpu):
    L, hl, hr, P = 12, 2, 2, 4100
    calls = []
    shard = RingPopulationShard(RingShardPlan(0, 1, L, hl, hr), P, torch.device("cuda"), None, gpu, fused=True)
    _fill(shard, L)
    shard.round(timer=lambda i, start: calls.append((i, start)))
    assert calls == [(0, True), (L - 1, False)]
    shard2 = RingPopulationShard(RingShardPlan(1, 2, L, hl, hr), P, torch.device("cuda"), None, gpu, fused=True)
    _fill(shard2, 2 * L)
    calls.clear()
    shard2._mix_set(shard2.interior_order(), torch.cuda.current_stream(), lambda i, start: calls.append((i, start)))
    torch.cuda.synchronize()
    assert calls == [(hl, True), (L - hr - 1, False)]


def test_auto_keeps_per_device_mixes_for_cache_resident_rows(gpu):
    L, h, P = 4, 1, 1_000_000
    eng = Counting(gpu)
    shard = RingPopulationShard(RingShardPlan(0, 1, L, h), P, torch.device("cuda"), None, eng)
    assert shard.fused == "auto"
    pop = _fill(shard, L)
    shard.round()
    torch.cuda.synchronize()
    assert not eng.slides and len(eng.prepared) == L
    assert np.array_equal(shard.mixed.cpu().numpy(), _oracle(shard.plan, pop, shard.alphas))


@pytest.mark.parametrize("late", [False, True])
def test_fused_round_on_a_stream_that_is_not_current(gpu, late):
    """round(cs) and compute_round(cs) on a side stream while the current stream is busy: the fused
    call's coefficients are final before any stream uses them (``late``: ``fused`` switched on
    after construction, so they are built at the first fused call)."""
    L, hl, hr, P = 12, 2, 2, 4100
    plan = RingShardPlan(0, 1, L, hl, hr)
    eng = Counting(gpu)
    shard = RingPopulationShard(plan, P, torch.device("cuda"), None, eng, fused=False if late else True)
    shard.fused = True
    pop = _fill(shard, L)
    ref = _oracle(plan, pop, shard.alphas)
    torch.cuda.synchronize()
    busy = torch.empty(64 * 2**20, device="cuda")
    cs = torch.cuda.Stream()
    for run in (lambda: shard.round(cs), lambda: shard.compute_round(cs)):
        for _ in range(8):
            busy.normal_()  # keeps the current stream busy while the round is enqueued on cs
        run()
        cs.synchronize()
        assert np.array_equal(shard.mixed.cpu().numpy(), ref)
        shard.mixed.fill_(float("nan"))
        torch.cuda.synchronize()
    assert eng.slides == [(0, L), (0, L)]
