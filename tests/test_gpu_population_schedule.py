"""Topology schedules on the device (cfa_mix_population_sched_f32 / _sched_tf1_f32): a population
whose neighbour lists change from round to round, with all tables and the round counter resident
on the GPU, equals the same population given each round's topology with ``set_topology``, bit
for bit: eager, replayed from graphs, and against the mobile-network drop-in's trajectory."""
import functools
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

D, TABLES = 5, 7
SCHED = [3, 0, 6, 6, 1, 5, 0, 2, 4]  # 9 slots over 7 tables: 0 and 6 twice
# one float4 past a whole tile of each kernel (fp32: 256 lanes x 2 float4, TF1: 256 x 1) plus a
# 3-element tail; rows of a [D, P] stack are then not 16-byte aligned either (as P = 777 of
# test_gpu_graph_rounds, and the odd sizes of test_gpu_population_fuzz)
P_FP32, P_TF1 = 2048 + 4 + 3, 1024 + 4 + 3


@functools.lru_cache(maxsize=None)
def _tables():
    """7 tables from topology.mobile on a seeded random adjacency tensor, max_neighbors = 2 on a
    seeded random.Random: rows of 3 or 4 neighbours are drawn down to 2 with replacement."""
    from federated_amd import topology as T
    rng = np.random.default_rng(2024)
    graph = (rng.random((D, D, TABLES)) < 0.7).astype(np.uint8)
    for g in range(TABLES):
        np.fill_diagonal(graph[:, :, g], 0)
    graph[2, :, 4] = 0  # device 2 has no neighbour in table 4
    draw = random.Random(7)
    tables = [T.mobile(graph, g, max_neighbors=2, rng=draw) for g in range(TABLES)]
    assert tables[4][2] == []
    assert any(len(nb) == 2 and nb[0] == nb[1] for lists in tables for nb in lists)  # a repeated neighbour
    assert len({tuple(map(tuple, lists)) for lists in tables}) == TABLES  # the tables differ
    return tables


KINDS = {
    "fp32": dict(P=P_FP32, numerics="fp32", compression=None, scale=1.0),
    "tf1": dict(P=P_TF1, numerics="tf1", compression=None, scale=1.0),
    # DPCM against the pre-mix local on [40, 900): weights near the mode's 1e-4 threshold
    "tf1-dpcm": dict(P=P_TF1, numerics="tf1", compression=(2, 40, 900), scale=1e-4),
}


def _policy(kind):
    from federated_amd import topology as T
    return T.alphas_tf2 if KINDS[kind]["numerics"] == "fp32" else T.alphas_tf1_ongraphs(0.9)


def _start(kind):
    k = KINDS[kind]
    rng = np.random.default_rng(len(kind))
    return (rng.standard_normal((D, k["P"])) * k["scale"]).astype(np.float32)


def _population(gpu, kind, models):
    from federated_amd import topology as T
    return T.PopulationRound(gpu, torch.tensor(models, device="cuda"))


R_MAX = 42  # the longest run any test compares


@functools.lru_cache(maxsize=None)
def _reference(kind, sched, R=R_MAX):
    """The parent's only route: per round set_topology(lists[sched[r % S]]) and run(). Returns
    every round's models and kept counters (numpy, read-only); computed once per (kind, sched)."""
    from federated_amd.engine import get_engine
    k = KINDS[kind]
    pr = _population(get_engine(), kind, _start(kind))
    rounds, kept = [], []
    for r in range(R):
        pr.set_topology(_tables()[sched[r % len(sched)]], _policy(kind), use_window=False, numerics=k["numerics"],
                        compression=k["compression"])
        pr.models.copy_(pr.run())
        rounds.append(pr.models.cpu().numpy())
        kept.append(pr.kept.cpu().numpy())
        rounds[-1].setflags(write=False)
    return rounds, kept


def _scheduled(gpu, kind, sched=SCHED):
    k = KINDS[kind]
    pr = _population(gpu, kind, _start(kind))
    pr.set_schedule(_tables(), _policy(kind), sched=list(sched), numerics=k["numerics"], compression=k["compression"])
    return pr


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_scheduled_rounds_equal_per_round_set_topology(gpu, kind):
    R = 2 * len(SCHED) + 1  # wraps the schedule twice
    ref, ref_kept = _reference(kind, tuple(SCHED))
    pr = _scheduled(gpu, kind)
    assert pr.round_index == 0 and pr.window is None
    for r in range(R):
        got = pr.rounds(1, graph=False).cpu().numpy()
        assert np.array_equal(got, ref[r]), (kind, r)
        if KINDS[kind]["compression"]:
            assert np.array_equal(pr.kept.cpu().numpy(), ref_kept[r]), (kind, r)
    assert pr.round_index == R
    if KINDS[kind]["compression"]:  # the epilogue did something: neither nothing nor everything kept
        print("kept per round:", [int(k.sum()) for k in ref_kept])
        assert 0 < int(ref_kept[0].sum()) < D * (900 - 40)
    assert not np.array_equal(ref[0], ref[1])
    # all R rounds in one call, and run() alone (one round, models -> out)
    whole = _scheduled(gpu, kind)
    assert np.array_equal(whole.rounds(R, graph=False).cpu().numpy(), ref[R - 1]), kind
    assert whole.round_index == R
    one = _scheduled(gpu, kind)
    assert np.array_equal(one.run().cpu().numpy(), ref[0]) and one.round_index == 1


def test_population_graph_replay_equals_eager(gpu):
    """37 = two 16-round blocks + two single periods + one eager round: the 9-slot schedule wraps
    four times and crosses every boundary between graphs."""
    R, R2 = 37, 5
    ref, _ = _reference("fp32", tuple(SCHED))
    eager, graph = _scheduled(gpu, "fp32"), _scheduled(gpu, "fp32")
    e = eager.rounds(R, graph=False).cpu().numpy()
    g = graph.rounds(R, graph=True).cpu().numpy()
    assert np.array_equal(g, e) and np.array_equal(e, ref[R - 1])
    assert graph.round_index == R and eager.round_index == R
    # a second call goes on from round 37 (the captured graphs are reused)
    g = graph.rounds(R2, graph=True).cpu().numpy()
    e = eager.rounds(R2, graph=False).cpu().numpy()
    assert np.array_equal(g, e) and np.array_equal(e, ref[R + R2 - 1])
    assert graph.round_index == R + R2


def test_scheduled_linear_rule_equals_static_linear_rounds(gpu):
    """``PopulationRound`` only passes the sequential rule, so the scheduled kernel's linear
    instance is reached through ``Engine.population_sched`` itself: every round equals the static
    linear kernel (checked against numpy in test_gpu_population.py) on that round's one table,
    and the counter, which wraps the 9-slot schedule, ends at the number of rounds."""
    from federated_amd import _lib
    from federated_amd import topology as T
    upload = lambda arrays: tuple(torch.from_numpy(a).cuda() for a in arrays)
    pointers = lambda m: torch.tensor([m[d].data_ptr() for d in range(D)], dtype=torch.int64, device="cuda")
    tables = upload(T.schedule_csr(_tables(), T.alphas_tf2, D))
    sched = torch.tensor(SCHED, dtype=torch.int32, device="cuda")
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    models = torch.tensor(_start("fp32"), device="cuda")
    got, want = torch.empty_like(models), torch.empty_like(models)
    src, dst_got, dst_want = pointers(models), pointers(got), pointers(want)
    R = len(SCHED) + 2
    for r in range(R):
        gpu.population_sched(dst_got, src, *tables, sched, counter, D, _lib.RULE_LINEAR, P_FP32)
        one = upload(T.csr(_tables()[SCHED[r % len(SCHED)]], T.alphas_tf2, D))
        gpu.population(dst_want, src, *one, D, _lib.RULE_LINEAR, P_FP32)
        assert torch.equal(got, want), r
        assert not torch.equal(got, models), r  # the round mixed something
        models.copy_(got)
    assert int(counter.item()) == R


def _tf1_inputs():
    g = torch.Generator(device="cuda").manual_seed(53)
    return (torch.randn(D, P_TF1, device="cuda", generator=g) * 1e-4,
            torch.randn(D, P_TF1, device="cuda", generator=g) * 1e-4)


def _tf1_pair(gpu, compression):
    from federated_amd import topology as T
    cur, prev = _tf1_inputs()
    pops = []
    for _ in range(2):
        p = T.Tf1PopulationRound(gpu, D, P_TF1)
        p.set_schedule(_tables(), T.alphas_tf1_ongraphs(0.9), sched=SCHED, compression=compression)
        p.load(cur, prev)
        pops.append(p)
    return pops


@pytest.mark.parametrize("compression", [None, (2, 40, 900)], ids=["plain", "dpcm"])
def test_tf1_population_graph_replay_equals_eager(gpu, compression):
    """53 = two 24-round blocks + one period + two eager rounds; with compression every captured
    round also holds the zeroing of ``kept`` ahead of its launch."""
    R, R2 = 53, 7
    eager, graph = _tf1_pair(gpu, compression)
    for n, total in ((R, R), (R2, R + R2)):
        eager.rounds(n, graph=False)
        graph.rounds(n, graph=True)
        assert torch.equal(graph.current, eager.current) and torch.equal(graph.previous, eager.previous), total
        assert torch.equal(graph.kept, eager.kept)
        assert graph.round_index == total and eager.round_index == total
    # ... and eager is the per-round set_topology route
    from federated_amd import topology as T
    ref, _ = _tf1_pair(gpu, compression)
    for r in range(R + R2):
        ref.set_topology(_tables()[SCHED[r % len(SCHED)]], T.alphas_tf1_ongraphs(0.9), compression=compression)
        ref.round()
    assert torch.equal(ref.current, eager.current) and torch.equal(ref.previous, eager.previous)
    assert torch.equal(ref.kept, eager.kept)


TF1_SHAPES = [(16, 1, 8), (8,), (168, 8), (8,)]  # CFA-GE CNN bucket, P = 1 488 (cfa.py's tensors)


@pytest.fixture
def mobile_workdir(tmp_path, monkeypatch):
    """A working directory with its own consensus/vGraph.mat: a seeded random symmetric uint8
    [5, 5, 6] adjacency tensor in which every device has a neighbour in every graph (a device
    without one fails in the reference, cfa.py:141)."""
    import scipy.io as sio
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("FEDERATED_AMD_PAUSE_SCALE", "0")
    os.makedirs("results")
    os.makedirs("consensus")
    rng = np.random.default_rng(5)  # a seed at which the row property below holds
    upper = np.triu((rng.random((6, D, D)) < 0.5).astype(np.uint8), 1)
    graph = np.ascontiguousarray((upper + upper.transpose(0, 2, 1)).transpose(1, 2, 0))
    assert graph.shape == (D, D, 6) and graph.dtype == np.uint8
    assert np.array_equal(graph, graph.transpose(1, 0, 2)) and graph.sum(axis=1).min() >= 1
    assert len({graph[:, :, g].tobytes() for g in range(1, 5)}) == 4  # epochs 1..4 differ
    sio.savemat("consensus/vGraph.mat", {"graph": graph})
    return graph


def test_mobilenet_dropin_trajectory(gpu, mobile_workdir):
    """cfa_mobilenet.py:136-138: epoch e mixes with the neighbours of graph e. Four epochs of
    per-device drop-in calls through the .mat protocol (as
    test_tf1_population_reproduces_dropin_trajectory) equal four scheduled Tf1PopulationRound
    rounds, every device at every epoch; reset_round(1) makes the first round use graph 1."""
    from federated_amd import topology as T
    from federated_amd.consensus.cfa_mobilenet import CFA_process
    graph, N, eps = mobile_workdir, 2, 0.7
    rng = np.random.default_rng(5)
    sizes = [int(np.prod(s)) for s in TF1_SHAPES]
    flat = lambda m: np.concatenate([np.asarray(a, dtype=np.float32).reshape(-1) for a in m])
    split = lambda v: [v[o:o + n].reshape(s) for o, n, s in zip(np.cumsum([0] + sizes[:-1]), sizes, TF1_SHAPES)]
    m0 = [[(rng.standard_normal(s) * 0.1).astype(np.float32) for s in TF1_SHAPES] for _ in range(D)]
    m1 = [[(rng.standard_normal(s) * 0.1).astype(np.float32) for s in TF1_SHAPES] for _ in range(D)]
    procs = [CFA_process(True, D, d, N) for d in range(D)]
    for d in range(D):  # epoch 0 publishes
        W1, b1, W2, b2 = m0[d]
        procs[d].getFederatedWeight(W1, W2, b1, b2, 0, np.zeros(3), eps)
    pr = T.Tf1PopulationRound(gpu, D, sum(sizes))
    pr.set_schedule([T.mobile(graph, e) for e in range(graph.shape[2])], T.alphas_tf1_cfa(eps, N))
    pr.load(torch.from_numpy(np.stack([flat(m) for m in m1])).cuda(), torch.from_numpy(np.stack([flat(m) for m in m0])).cuda())
    pr.reset_round(1)
    models = m1
    for epoch in range(1, 5):
        new = []
        for d in range(D):
            W1, b1, W2, b2 = models[d]
            out = procs[d].getFederatedWeight(W1, W2, b1, b2, epoch, np.zeros(3), eps)
            assert procs[d].neighbor_vec.tolist() == T.mobile(graph, epoch)[d]
            new.append(split(flat([np.float32(a) if np.ndim(a) == 0 else np.asarray(a).astype(np.float32) for a in out])))
        models = new  # the driver's fp32 TF variables
        pr.round()
        got = pr.current.cpu().numpy()
        for d in range(D):
            assert np.array_equal(got[d], flat(models[d])), (epoch, d)
    assert pr.round_index == 5


def test_counters_are_per_population(gpu):
    """Two scheduled populations on one engine, advanced alternately, each follow their own
    schedule; reset_round(3) makes the next round use sched[3]."""
    sa, sb = tuple(SCHED), (5, 2, 2, 6)
    ra, _ = _reference("fp32", sa)
    rb, _ = _reference("fp32", sb, 6)
    a, b = _scheduled(gpu, "fp32", sa), _scheduled(gpu, "fp32", sb)
    for r in range(4):
        assert np.array_equal(a.rounds(1, graph=False).cpu().numpy(), ra[r]), r
        assert np.array_equal(b.rounds(1, graph=False).cpu().numpy(), rb[r]), r
    b.rounds(2)  # one captured period of b alone
    assert np.array_equal(b.models.cpu().numpy(), rb[5])
    assert (a.round_index, b.round_index) == (4, 6)
    # round 3 of the schedule again, on the models of round 4
    from federated_amd import topology as T
    want = _population(gpu, "fp32", ra[3])
    want.set_topology(_tables()[sa[3]], T.alphas_tf2, use_window=False)
    a.reset_round(3)
    assert np.array_equal(a.run().cpu().numpy(), want.run().cpu().numpy())
    assert (a.round_index, b.round_index) == (4, 6)


def test_set_topology_after_set_schedule_is_the_static_path(gpu):
    from federated_amd import topology as T
    lists = T.kregular_v3(D, 2)
    m0 = _start("fp32")
    plain, was = _population(gpu, "fp32", m0), _scheduled(gpu, "fp32")
    was.rounds(3)  # scheduled rounds, graphs captured
    was.models.copy_(torch.from_numpy(m0))
    for p in (plain, was):
        p.set_topology(lists, T.alphas_tf2, use_window=False)
    assert np.array_equal(was.run().cpu().numpy(), plain.run().cpu().numpy())
    assert np.array_equal(was.rounds(5).cpu().numpy(), plain.rounds(5).cpu().numpy())
    assert np.array_equal(was.rounds(3, graph=False).cpu().numpy(), plain.rounds(3, graph=False).cpu().numpy())
    with pytest.raises(RuntimeError, match="set_schedule"):
        was.round_index
    # the same for the TF1 protocol population
    was = _tf1_pair(gpu, None)[0]
    was.rounds(4)
    plain = T.Tf1PopulationRound(gpu, D, P_TF1)
    plain.load(*_tf1_inputs())
    was.load(*_tf1_inputs())
    for p in (plain, was):
        p.set_topology(T.kregular_tf1(D, 2), T.alphas_tf1_cfa(0.9, 2))
    plain.rounds(7)
    was.rounds(7)
    assert torch.equal(was.current, plain.current) and torch.equal(was.previous, plain.previous)
