"""The TF2 protocol's training_end rule on a device-resident population
(``PopulationRound.set_ended_rule``, cfa_mix_population_ended_f32). A population round is D
per-device calls on the previous round's rows and flags, and those calls are pinned to the
reference by test_oracle_reference_fuzz / test_oracle_golden, so the reference of every case here
is built from the oracle, per device, and compared bit for bit (uint32 views: NaN payloads count).
"""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import cfa_oracle as O

pytestmark = pytest.mark.gpu

RULES = ("copy", "truncate", "truncate_eps")
EPS = 0.3  # the caller's eps of consensus_v4's gradients ("truncate")


def _policy(rule):
    """The eps policy a run with ``rule`` uses: 1/(n+1) for federated weights (consensus_v3.py:145);
    the caller's one eps for v4's gradients; anything for v3's gradients, which recompute it."""
    from federated_amd import topology as T
    return (lambda nbrs, ii, devices: [EPS] * len(nbrs)) if rule == "truncate" else T.alphas_tf2


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _ref_round(rows, flags, lists, rule):
    """One round by the oracle, device by device, on the previous round's rows and flags:
    (rows, saw). ``upto`` as test_oracle_reference_fuzz.py:189."""
    out, saw = np.empty_like(rows), np.zeros(len(lists), dtype=np.int32)
    for d, nbr in enumerate(lists):
        if flags[d]:  # the device has left its loop
            out[d] = rows[d]
            continue
        upto = next((i + 1 for i, j in enumerate(nbr) if flags[j]), len(nbr))
        found = any(flags[j] for j in nbr)
        local, nbrs = [rows[d]], [[rows[j]] for j in nbr[:upto]]
        if rule == "copy":
            out[d] = O.tf2_weights(local, nbrs, training_end=found)[0]
        elif rule == "truncate":
            out[d] = O.tf2_grads_v4(local, nbrs, EPS)[0]
        else:
            out[d] = O.tf2_grads_v3(local, nbrs)[0]
        saw[d] = found
    return out, saw


def _population(gpu, rows, lists, rule, propagate=False):
    from federated_amd import topology as T
    pr = T.PopulationRound(gpu, torch.from_numpy(np.array(rows)).cuda())
    pr.set_ended_rule(rule, propagate)
    pr.set_topology(lists, _policy(rule))  # the rule survives set_topology
    return pr


def _flags(ids, D):
    f = np.zeros(D, dtype=np.int32)
    f[list(ids)] = 1
    return f


def _lists(rng, D):
    """Random lists of fan-in 0..5 over all D ids (duplicates and the device itself allowed);
    device 0 has 5 entries with itself and a duplicate among them, the last device none."""
    lists = [[int(j) for j in rng.integers(0, D, size=int(rng.integers(0, 6)))] for _ in range(D)]
    lists[0] = [1 % D, 0, D // 2, D // 2, D - 1]
    if D > 1:
        lists[-1] = []
    return lists


def _ended_sets(lists, D):
    """Empty; one device; the first, a middle and the last position of device 0's list; several of
    its neighbours (the first in list order wins); the device itself; everyone."""
    nbr = lists[0]
    return [[], [D - 1], [nbr[0]], [nbr[2]], [nbr[-1]], sorted(set(nbr[2:])), [0], list(range(D))]


@pytest.mark.parametrize("D", [1, 2, 9])
@pytest.mark.parametrize("P", [1, 3, 4, 2051, 4101])
def test_round_equals_the_oracle_per_device(gpu, P, D):
    """P: tail only, tail only, one float4, one tile plus a float4 and a tail, a grid-stride over
    several tiles plus tail."""
    rng = np.random.default_rng(1000 * D + P)
    rows = rng.standard_normal((D, P)).astype(np.float32)
    lists = _lists(rng, D)
    for rule in RULES:
        pr = _population(gpu, rows, lists, rule)
        for ids in _ended_sets(lists, D):
            flags = _flags(ids, D)
            want, want_saw = _ref_round(rows, flags, lists, rule)
            pr.set_ended(ids)
            got = pr.run().cpu().numpy()
            assert np.array_equal(_bits(got), _bits(want)), (rule, ids)
            assert pr.saw_ended.cpu().tolist() == want_saw.tolist(), (rule, ids)
            assert pr.ended.cpu().tolist() == flags.tolist(), (rule, ids)  # propagate=False
            assert np.array_equal(_bits(pr.models.cpu().numpy()), _bits(rows))


@pytest.mark.parametrize("rule", RULES)
def test_list_longer_than_a_workgroup(gpu, rule):
    """A 300-entry list: the 256 lanes of a workgroup stride over it. Device 3 sits only at
    position 270; flagged, the fold (or the copy) stops there, and with nobody flagged all 300
    entries are folded."""
    D, P = 4, 64
    rng = np.random.default_rng(300)
    rows = rng.standard_normal((D, P)).astype(np.float32)
    long = [int(j) for j in rng.integers(1, 3, size=300)]
    long[270] = 3
    assert long.count(3) == 1 and {1, 2} <= set(long)
    lists = [long, [0], [], [1, 1]]
    pr = _population(gpu, rows, lists, rule)
    for ids in ([3], []):
        want, want_saw = _ref_round(rows, _flags(ids, D), lists, rule)
        pr.set_ended(ids)
        assert np.array_equal(_bits(pr.run().cpu().numpy()), _bits(want)), ids
        assert pr.saw_ended.cpu().tolist() == want_saw.tolist() == [int(bool(ids)), 0, 0, 0]
    long_flagged, long_all = (_ref_round(rows, _flags(ids, D), lists, rule)[0][0] for ids in ([3], []))
    assert not np.array_equal(long_flagged, long_all)  # the prefix of 271 is not the whole list


def test_copy_keeps_every_bit_pattern(gpu):
    """The copied row passes through no arithmetic: NaNs with distinct payloads, both zeros, both
    infinities and subnormals arrive as they were (w + 1 * (x - w) would not deliver them)."""
    special = np.array([0x7FC00000, 0x7FC00001, 0xFFC12345, 0x7F800001, 0xFF9ABCDE, 0x7FFFFFFF,  # quiet / signalling NaNs
                        0x00000000, 0x80000000, 0x7F800000, 0xFF800000,                          # +-0, +-inf
                        0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00400000,              # subnormals
                        0x00800000, 0x7F7FFFFF, 0x3F800000, 0xBF800001], dtype=np.uint32)
    P = 4 * 256 * 2 + 4 + 3  # one tile, one float4 more, a tail: every path of the body copies
    rng = np.random.default_rng(77)
    rows = rng.standard_normal((3, P)).astype(np.float32)
    rows[2] = np.resize(special, P).view(np.float32)
    lists = [[1, 2], [2], [0, 1]]  # device 0 collects 1, then the ended 2; device 1 the ended 2 at once
    pr = _population(gpu, rows, lists, "copy")
    pr.set_ended([2])
    got = _bits(pr.run().cpu().numpy())
    for d in range(3):  # two copies and the ended device's own row
        assert np.array_equal(got[d], _bits(rows[2])), d
    assert np.array_equal(got, _bits(_ref_round(rows, _flags([2], 3), lists, "copy")[0]))
    assert pr.saw_ended.cpu().tolist() == [1, 1, 0]


@pytest.mark.parametrize("scheduled", [False, True], ids=["topology", "schedule"])
def test_no_flags_is_the_existing_round(gpu, scheduled):
    """With every flag clear "copy" and "truncate" are today's round (rule off, CSR kernel) bit
    for bit, whatever the eps policy: existing behaviour is kept."""
    from federated_amd import topology as T
    D, P = 9, 2051
    rng = np.random.default_rng(9)
    rows = rng.standard_normal((D, P)).astype(np.float32)
    lists = _lists(rng, D)
    policy = T.alphas_tf1_ongraphs(0.9)  # a coefficient per neighbour count: not one eps

    def run(rule):
        pr = T.PopulationRound(gpu, torch.from_numpy(rows.copy()).cuda())
        pr.set_ended_rule(rule)
        if scheduled:
            pr.set_schedule([lists[::-1], lists], policy, sched=[1, 0])
        else:
            pr.set_topology(lists, policy, use_window=False)
        one = pr.run().cpu().numpy()
        return one, pr.rounds(3, graph=False).cpu().numpy(), pr.saw_ended.cpu().tolist()

    base = run(None)
    assert base[2] == [0] * D
    for rule in ("copy", "truncate"):
        got = run(rule)
        assert np.array_equal(_bits(got[0]), _bits(base[0])), rule
        assert np.array_equal(_bits(got[1]), _bits(base[1])), rule
        assert got[2] == [0] * D


def _ring(D):
    return [[(d - 1) % D, (d + 1) % D] for d in range(D)]


def test_status_and_propagation_on_a_ring(gpu):
    """One device of a 9-ring has ended. propagate=True: every device of round r reads round
    r - 1's flags, so the flags spread one hop per round and the solved model with them;
    propagate=False: the flags stay as set_ended left them."""
    D, P = 9, 2051
    rng = np.random.default_rng(4)
    rows = rng.standard_normal((D, P)).astype(np.float32)
    lists = _ring(D)
    pr = _population(gpu, rows, lists, "copy", propagate=True)
    assert pr.ended.cpu().tolist() == [0] * D  # all clear at the start
    pr.set_ended([4])
    flags, models = _flags([4], D), rows
    for r in range(4):
        models, saw = _ref_round(models, flags, lists, "copy")
        hop = [int(abs(d - 4) == r + 1) for d in range(D)]  # exactly the devices r + 1 hops away
        assert saw.tolist() == hop
        flags = flags | saw
        got = pr.rounds(1, graph=False).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(models)), r
        assert pr.saw_ended.cpu().tolist() == hop, r
        assert pr.ended.cpu().tolist() == flags.tolist() == [int(abs(d - 4) <= r + 1) for d in range(D)], r
    assert pr.ended.cpu().tolist() == [1] * D
    for d in range(D):  # everyone holds the ended device's model
        assert np.array_equal(_bits(models[d]), _bits(rows[4]))
    # run() alone: one round into out, the flags of that round in ``ended``
    pr.set_ended([0])
    models, saw = _ref_round(models, _flags([0], D), lists, "copy")
    assert np.array_equal(_bits(pr.run().cpu().numpy()), _bits(models))
    assert pr.ended.cpu().tolist() == (_flags([0], D) | saw).tolist() == [1, 1, 0, 0, 0, 0, 0, 0, 1]

    still = _population(gpu, rows, lists, "copy", propagate=False)
    still.set_ended([4])
    flags, models = _flags([4], D), rows
    for r in range(4):
        models, saw = _ref_round(models, flags, lists, "copy")
        got = still.rounds(1, graph=False).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(models)), r
        assert still.saw_ended.cpu().tolist() == saw.tolist() == [int(abs(d - 4) == 1) for d in range(D)]
        assert still.ended.cpu().tolist() == flags.tolist()


@functools.lru_cache(maxsize=None)
def _sched_tables():
    rng = np.random.default_rng(31)
    tables = [_lists(rng, 9) for _ in range(3)]
    assert len({str(t) for t in tables}) == 3
    return tables


@pytest.mark.parametrize("rule,propagate", [("copy", True), ("truncate", False), ("truncate_eps", False)])
def test_schedule_with_flags(gpu, rule, propagate):
    """Three tables, sched = [0, 2, 1, 1], six rounds: flags before round 0 and again between
    rounds 3 and 4. Every round equals the oracle on that round's table and the flags of the
    round before; rounds 4 and 5 are replayed from a captured graph."""
    D, P, sched = 9, 4101, [0, 2, 1, 1]
    tables = _sched_tables()
    rows = np.random.default_rng(32).standard_normal((D, P)).astype(np.float32)
    from federated_amd import topology as T
    pr = T.PopulationRound(gpu, torch.from_numpy(rows.copy()).cuda())
    pr.set_schedule(tables, _policy(rule), sched=sched)
    pr.set_ended_rule(rule, propagate)  # after set_schedule this time
    assert pr.window is None and pr.round_index == 0
    first, second = [7], [2, 5]
    flags, models = _flags(first, D), rows
    pr.set_ended(first)
    for r in range(6):
        if r == 4:
            flags = _flags(second, D)
            pr.set_ended(second)
        models, saw = _ref_round(models, flags, tables[sched[r % 4]], rule)
        if propagate:
            flags = flags | saw
        if r < 4:
            got = pr.rounds(1, graph=False)
        elif r == 4:
            continue  # rounds 4 and 5 together, below
        else:
            got = pr.rounds(2)
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(models)), r
        assert pr.saw_ended.cpu().tolist() == saw.tolist(), r
        assert pr.ended.cpu().tolist() == flags.tolist(), r
        assert pr.round_index == r + 1
    assert pr.round_index == 6


@pytest.mark.parametrize("rule", RULES)
def test_graph_replay_equals_eager(gpu, rule):
    """rounds(R) replayed from graphs equals rounds(R, graph=False): models, ``ended`` and
    ``saw_ended``, for an odd, an even and a mixed R with propagate=True; then three more rounds
    after set_ended on the same objects (the captured graphs are reused), and against the oracle."""
    D, P = 9, 2051
    rng = np.random.default_rng(55)
    rows = rng.standard_normal((D, P)).astype(np.float32)
    lists = _ring(D)
    lists[3] = [1, 8, 8, 3]

    def same(a, b, what):
        assert np.array_equal(_bits(a.models.cpu().numpy()), _bits(b.models.cpu().numpy())), what
        assert torch.equal(a.ended, b.ended) and torch.equal(a.saw_ended, b.saw_ended), what

    for R in (1, 2, 5):
        eager, graph = (_population(gpu, rows, lists, rule, propagate=True) for _ in range(2))
        flags, models = _flags([6], D), rows
        for pr in (eager, graph):
            pr.set_ended([6])
        eager.rounds(R, graph=False)
        graph.rounds(R)
        same(graph, eager, R)
        for _ in range(R):
            models, saw = _ref_round(models, flags, lists, rule)
            flags = flags | saw
        assert np.array_equal(_bits(eager.models.cpu().numpy()), _bits(models)), R
        assert eager.ended.cpu().tolist() == flags.tolist() and eager.saw_ended.cpu().tolist() == saw.tolist()
    flags = _flags([0], D)
    for pr in (eager, graph):
        pr.set_ended([0])
    eager.rounds(3, graph=False)
    graph.rounds(3)
    same(graph, eager, "second call")
    for _ in range(3):
        models, saw = _ref_round(models, flags, lists, rule)
        flags = flags | saw
    assert np.array_equal(_bits(graph.models.cpu().numpy()), _bits(models))
    assert graph.ended.cpu().tolist() == flags.tolist() and graph.saw_ended.cpu().tolist() == saw.tolist()


def test_argument_errors(gpu):
    from federated_amd import topology as T
    pr = T.PopulationRound(gpu, torch.zeros(4, 8, device="cuda"))
    with pytest.raises(ValueError, match="rule must be None"):
        pr.set_ended_rule("stop")
    with pytest.raises(ValueError, match="outside \\[0, 4\\)"):
        pr.set_ended([4])
    pr.set_ended_rule("copy")
    with pytest.raises(ValueError, match="TF2 numerics"):  # the rule first, TF1 numerics second
        pr.set_topology(_ring(4), T.alphas_tf1_cfa(0.5, 2), numerics="tf1")
    with pytest.raises(ValueError, match="TF2 numerics"):
        pr.set_schedule([_ring(4)], T.alphas_tf1_cfa(0.5, 2), numerics="tf1")
    pr.set_ended_rule(None)
    pr.set_topology(_ring(4), T.alphas_tf1_cfa(0.5, 2), numerics="tf1")
    with pytest.raises(ValueError, match="TF2 numerics"):  # TF1 numerics first, the rule second
        pr.set_ended_rule("truncate")
    pr.set_ended_rule(None)  # off is always accepted
    pr.run()


SHAPES = [(3, 3, 1, 4), (4,), (36, 5), (5,)]  # small layers, P = 225: a float4 body and a 1-element tail


@pytest.fixture
def workdir(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("FEDERATED_AMD_PAUSE_SCALE", "0")
    os.makedirs("results")
    return tmp_path


def _obj(layers):
    a = np.empty(len(layers), dtype=object)
    for i, l in enumerate(layers):
        a[i] = l
    return a


def test_population_follows_the_dropin_through_training_end(gpu, workdir):
    """Three rounds of consensus_v3.CFA_process through its file protocol, as
    test_gpu_trajectory, with device 2 publishing training_end from round 1 on and leaving its
    loop: the "copy" population with set_ended([2]) at the same round follows every device bit for
    bit, and saw_ended is every device's getTrainingStatusFromNeightbor()."""
    from federated_amd import topology as T
    from federated_amd.consensus.consensus_v3 import CFA_process
    D, N, E = 6, 2, 2
    lists = T.kregular_v3(D, N)
    assert sum(E in nb for nb in lists) >= 2 and any(E not in nb for d, nb in enumerate(lists) if d != E)
    rng = np.random.default_rng(62)
    models = [[rng.standard_normal(s).astype(np.float32) for s in SHAPES] for _ in range(D)]
    flat = lambda m: np.concatenate([np.asarray(a, dtype=np.float32).reshape(-1) for a in m])
    pr = T.PopulationRound(gpu, torch.from_numpy(np.stack([flat(m) for m in models])).cuda())
    pr.set_topology(lists, T.alphas_tf2)
    pr.set_ended_rule("copy")
    procs = [CFA_process(D, d, N) for d in range(D)]
    for rnd in range(3):
        ended = {E} if rnd >= 1 else set()
        for d in range(D):
            np.save(f"results/dump_train_model{d}.npy", _obj(models[d]), allow_pickle=True)
            np.savez(f"results/dump_train_variables{d}.npz", frame_count=rnd, epoch_count=rnd,
                     training_end=d in ended, loss=0.5)
        new, status = [], []
        for d in range(D):
            if d in ended:  # it has left its loop: the model stays, no status is read
                new.append(models[d])
                status.append(0)
                continue
            p = procs[d]
            p.update_local_model(_obj([a.copy() for a in models[d]]))
            out = p.federated_weights_computing(np.asarray(lists[d]), N, rnd, 0.5, 0, 30)
            new.append([np.asarray(a, dtype=np.float32) for a in out])
            status.append(int(bool(p.getTrainingStatusFromNeightbor())))
        models = new
        pr.set_ended(sorted(ended))
        got = pr.rounds(1, graph=False).cpu().numpy()
        for d in range(D):
            assert np.array_equal(_bits(got[d]), _bits(flat(models[d]))), (rnd, d)
        assert pr.saw_ended.cpu().tolist() == status, rnd
        assert status == [int(E in nb and d not in ended and bool(ended)) for d, nb in enumerate(lists)], rnd
    for d, nb in enumerate(lists):  # whoever listed device 2 holds its model now
        if E in nb and d != E:
            assert np.array_equal(_bits(flat(models[d])), _bits(flat(models[E])))
