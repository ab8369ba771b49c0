"""FedAvg parameter-server rounds on a device-resident population
(cfa_fedavg_population_round_f32, FedAvgPopulation): bit for bit against the oracle's server fold
(ps_fedavg: parameter_server_v2.py:146-161) and the MQTT learner's mix (learner_consensus_mix:
learner_consensus.py:151-152). Every comparison is on the fp32 bit patterns; where IEEE specials
are in play a NaN matches a NaN (payloads are not specified, as tests/test_gpu_kernels.py)."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle import cfa_oracle as O

pytestmark = pytest.mark.gpu

D = 20


@functools.lru_cache(maxsize=None)
def _shape():
    """(block, U below the long-row size, batch depth) of the kernel's default launch shape, from
    its shape header."""
    with open(os.path.join(ROOT, "federated_amd", "csrc", "cfa_fedavg_shape.h")) as fh:
        text = fh.read()
    block = int(re.search(r"kFedavgBlock\s*=\s*(\d+)", text).group(1))
    u, _, batch = (int(v) for v in re.search(r"kFedavgDefault\{(\d+),\s*(\d+),\s*(\d+),", text).groups())
    return block, u, batch


def _tile():  # float4 of a full tile
    block, u, _ = _shape()
    return block * u


def _fanin_lists():
    """C = 0, 1, b-1, b, b+1, 16, 17, 20 around the load batch b and the mix's 16-wide pass, in a
    scrambled device order, plus one list with duplicates and a non-monotone order."""
    b = _shape()[2]
    order = np.random.default_rng(3).permutation(D).tolist()
    lists = [order[:c] for c in sorted({0, 1, b - 1, b, b + 1, 16, 17, 20})]
    lists.append([7, 2, 7, 19, 0, 2, 7])
    return lists


CLIENTS = [("none", 1.0, 1.0), ("copy", 1.0, 1.0), ("mix", 1.0, 2.0), ("mix", 0.75, 1.0)]
SENTINEL = np.float32(-12345.5)


def _oracle_round(models, params, ids, u, ended=(), client=("copy", 1.0, 1.0)):
    """One reference round on numpy fp32 arrays: (models', params')."""
    with np.errstate(all="ignore"):
        flagged = [k for k in ids if k in ended]
        if flagged:  # parameter_server_v2.py:150-157: the first ended device in fold order, no division
            params = O.ps_fedavg([params], [[models[flagged[0]]]], u, divide=False)[0]
        elif ids:
            params = O.ps_fedavg([params], [[models[k]] for k in ids], u, divide=True)[0]
        rule, cf, cd = client
        if rule == "copy":
            models = np.tile(params, (models.shape[0], 1))
        elif rule == "mix":
            models = np.stack([O.learner_consensus_mix([w], [params], cf, cd)[0] for w in models])
    return models.astype(np.float32, copy=False), params.astype(np.float32, copy=False)


def _same(got, ref):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    both_nan = np.isnan(got) & np.isnan(ref)
    return got.shape == ref.shape and bool(np.all(both_nan | (got.view(np.uint32) == ref.view(np.uint32))))


def _population(gpu, models, params, u, pad=0):
    """A FedAvgPopulation on copies of the numpy arrays; pad > 0 (or a P that is no multiple of 4)
    puts the rows in a wider buffer whose padding columns hold SENTINEL."""
    from federated_amd.fedavg_population import FedAvgPopulation
    Dn, P = models.shape
    pitch = (P + 3) // 4 * 4 + pad
    buf = torch.full((Dn, pitch), float(SENTINEL), device="cuda")
    buf[:, :P] = torch.from_numpy(models).cuda()
    pop = FedAvgPopulation(gpu, buf[:, :P], torch.from_numpy(params.copy()).cuda(), u)
    pop._buf = buf
    return pop


def _padding_untouched(pop):
    P = pop.models.shape[1]
    return bool((pop._buf[:, P:] == float(SENTINEL)).all().item())


@pytest.mark.parametrize("tail", [0, 1, 2, 3])
@pytest.mark.parametrize("vecs", ["one", "tile", "tile+3"])
def test_sizes_fanins_and_clients(gpu, vecs, tail):
    """P = one vector, one full tile, one tile plus 3 vectors, each with 0-3 trailing scalars; for
    every client rule, one round per fan-in list (a schedule of all of them), each checked against
    the oracle: params, every row (devices that were not active too), and the padding columns."""
    nvec = {"one": 1, "tile": _tile(), "tile+3": _tile() + 3}[vecs]
    P = 4 * nvec + tail
    lists = _fanin_lists()
    rng = np.random.default_rng(P)
    m0 = rng.standard_normal((D, P)).astype(np.float32)
    p0 = rng.standard_normal(P).astype(np.float32)
    u = 0.9
    for client in CLIENTS:
        for pad in ((0, 8) if tail == 0 else (0,)):  # rows at pitch == P, and inside a wider buffer
            pop = _population(gpu, m0, p0, u, pad)
            pop.set_schedule(lists, client=client[0], client_factor=client[1], client_divisor=client[2])
            m, p = m0, p0
            for r, ids in enumerate(lists):
                pop.round()
                m, p = _oracle_round(m, p, ids, u, client=client)
                assert _same(pop.params, p), (client, pad, r, len(ids))
                assert _same(pop.models, m), (client, pad, r, len(ids))
                if client[0] == "none":
                    assert m is m0
            assert _padding_untouched(pop) and pop.round_index == len(lists)


@pytest.mark.parametrize("u,batch", [(1, 8), (4, 4), (4, 8)])
def test_other_launch_shapes(gpu, monkeypatch, u, batch):
    """The kernel's other tile widths and batch depth (the long-row width among them), through the
    library's per-launch overrides: a full tile of that width plus 3 vectors and 3 scalars, every
    fan-in list, the mix client."""
    monkeypatch.setenv("CFA_FEDAVG_U", str(u))
    monkeypatch.setenv("CFA_FEDAVG_BATCH", str(batch))
    P = 4 * (_shape()[0] * u + 3) + 3
    lists = _fanin_lists()
    rng = np.random.default_rng(P + batch)
    m = rng.standard_normal((D, P)).astype(np.float32)
    p = rng.standard_normal(P).astype(np.float32)
    pop = _population(gpu, m, p, 0.9)
    pop.set_schedule(lists, client="mix", client_factor=1.0, client_divisor=2.0)
    for r, ids in enumerate(lists):
        pop.round()
        m, p = _oracle_round(m, p, ids, 0.9, client=("mix", 1.0, 2.0))
        assert _same(pop.params, p) and _same(pop.models, m), (u, batch, r)
    assert _padding_untouched(pop)


def test_ended_flags(gpu):
    """No flag; a flagged device outside the active list (the normal fold); two flagged active
    devices (the first in LIST order is used, not the lowest id)."""
    P = 4 * (_tile() + 3) + 3
    rng = np.random.default_rng(11)
    m0 = rng.standard_normal((D, P)).astype(np.float32)
    p0 = rng.standard_normal(P).astype(np.float32)
    ids = [9, 14, 3, 17, 5, 0]
    for ended in ([], [11], [3, 17], [5, 14, 0]):
        pop = _population(gpu, m0, p0, 0.5)
        pop.set_schedule([ids], client="mix", client_factor=1.0, client_divisor=2.0)
        pop.set_ended(ended)
        pop.round()
        m, p = _oracle_round(m0, p0, ids, 0.5, ended, ("mix", 1.0, 2.0))
        assert _same(pop.params, p) and _same(pop.models, m), ended
    # the first in list order: 14 for {5, 14, 0}, not device 0
    want = O.ps_fedavg([p0], [[m0[14]]], 0.5, divide=False)[0]
    assert _same(pop.params, want)
    assert not _same(pop.params, O.ps_fedavg([p0], [[m0[0]]], 0.5, divide=False)[0])


def test_set_ended_between_replayed_rounds(gpu):
    """set_ended is ordered with the replayed rounds on the stream: two replayed rounds fold, the
    next two take the transfer-learning step, the last two fold again."""
    P = 4 * _tile() + 4 + 2
    rng = np.random.default_rng(12)
    m0 = rng.standard_normal((D, P)).astype(np.float32)
    p0 = rng.standard_normal(P).astype(np.float32)
    lists = [[4, 8, 15, 16], [2, 3, 4]]
    client = ("mix", 1.0, 2.0)
    pop = _population(gpu, m0, p0, 0.8)
    pop.set_schedule(lists, client="mix", client_factor=1.0, client_divisor=2.0)
    m, p, r = m0, p0, 0
    for ended in ([], [4], []):
        pop.set_ended(ended)
        pop.rounds(2, graph=True)
        for _ in range(2):
            m, p = _oracle_round(m, p, lists[r % 2], 0.8, ended, client)
            r += 1
        assert _same(pop.params, p) and _same(pop.models, m), ended
    assert pop.round_index == 6


def _binades(rng, P):
    """fp32 values in every binade (every biased exponent but inf / NaN, subnormals included)."""
    mant = rng.integers(0, 1 << 23, P, dtype=np.uint32)
    expo = (np.arange(P, dtype=np.uint32) % 255)
    sign = rng.integers(0, 2, P, dtype=np.uint32) << 31
    return (sign | (expo << 23) | mant).view(np.float32)


def _specials(rng, P):
    fi = np.finfo(np.float32)
    a = rng.standard_normal(P).astype(np.float32)
    sp = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, fi.smallest_subnormal, -fi.smallest_subnormal,
                   fi.smallest_normal * 0.5, fi.tiny, fi.max, -fi.max, 1e-40], dtype=np.float32)
    idx = rng.choice(P, size=3 * sp.size, replace=False)
    a[idx] = np.resize(sp, idx.size)
    return a


@pytest.mark.parametrize("C", [3, 7])
@pytest.mark.parametrize("client", [("copy", 1.0, 1.0), ("mix", 1.0, 2.0)], ids=["copy", "mix"])
def test_specials_and_every_binade(gpu, C, client):
    """NaN / inf / -0.0 / subnormals / the largest finite values in rows and params, and values in
    every fp32 binade: numpy's results (no flush to zero, IEEE propagation, overflow to inf)."""
    P = 4 * (_tile() + 3) + 1
    rng = np.random.default_rng(40 + C)
    m0 = np.stack([_specials(rng, P) if d % 2 else _binades(rng, P) for d in range(D)])
    for p0 in (_specials(rng, P), _binades(rng, P)):
        ids = rng.permutation(D)[:C].tolist()
        pop = _population(gpu, m0, p0, 1.0)
        pop.set_schedule([ids], client=client[0], client_factor=client[1], client_divisor=client[2])
        pop.round()
        m, p = _oracle_round(m0, p0, ids, 1.0, client=client)
        assert _same(pop.params, p) and _same(pop.models, m)


# odd k per o: t = k * o * 2^-149 over 2o is k / 2 units of the last subnormal place, an exact tie. For
# o = 1, 3, 5, 7 (k / 2 = 0.5, 1.5, 2.5, 3.5: ties-to-even goes down, up, down, up) the fp64
# reciprocal multiply happens to round every tie correctly; for o = 49 and 75 the listed k are ties
# it rounds the WRONG way (_multiply_alone_misses), so those cases fail without the IEEE re-walk.
TIES = {1: [1, 3, 5, 7], 3: [1, 3, 5, 7], 5: [1, 3, 5, 7], 7: [1, 3, 5, 7], 49: [3, 7, 15, 23], 75: [29, 57, 61, 113]}


def _tie(o):
    return (np.array(TIES[o], dtype=np.float64) * o * 2.0 ** -149).astype(np.float32)


def _multiply_alone_misses(o):
    """Whether (float)((double)t * RN_64(1 / 2o)) differs from the IEEE t / 2o on every tie of o."""
    t, d = _tie(o), np.float32(2 * o)
    fast = (t.astype(np.float64) * (1.0 / np.float64(d))).astype(np.float32)
    return bool(np.all(fast.view(np.uint32) != (t / d).view(np.uint32)))


def test_the_large_o_ties_discriminate():
    assert _multiply_alone_misses(49) and _multiply_alone_misses(75)
    assert not any(_multiply_alone_misses(o) for o in (1, 3, 5, 7))


def _tie_vectors(P):
    """Element ranges of the two float4 that hold the ties: vector 37 of the first (full) tile and
    vector 1 of the partial tile behind it."""
    assert P >= 4 * (_tile() + 2)
    return slice(4 * 37, 4 * 38), slice(4 * (_tile() + 1), 4 * (_tile() + 2))


@pytest.mark.parametrize("o", sorted(TIES))
@pytest.mark.parametrize("step", ["first", "last"])
def test_server_fold_exact_subnormal_ties(gpu, o, step):
    """t = odd k * o * 2^-149 over C = 2o is exactly a subnormal rounding midpoint: the fp64
    reciprocal multiply alone rounds some of these the wrong way, the lane's IEEE re-walk decides
    by ties-to-even as numpy. The ties sit in one float4 of a full tile (positive) and one of the
    partial tile (negative); every other lane holds normal data. At the first step p is 0 there; at
    the last step every earlier row is 0 there too, so p is still 0 when the tie row is folded.
    C = 2o entries over D devices: the list repeats devices, the tie row appears once."""
    C = 2 * o
    P = 4 * (_tile() + 3) + 2
    rng = np.random.default_rng(60 + o)
    m0 = rng.standard_normal((D, P)).astype(np.float32)
    p0 = rng.standard_normal(P).astype(np.float32)
    perm = rng.permutation(D).tolist()
    others, tied = [perm[i % (D - 1)] for i in range(C - 1)], perm[-1]
    ids = [tied] + others if step == "first" else others + [tied]
    pos, neg = _tie_vectors(P)
    for cols, sign in ((pos, 1.0), (neg, -1.0)):
        p0[cols] = 0.0
        if step == "last":
            m0[:, cols] = 0.0
        m0[tied, cols] = sign * _tie(o)
    pop = _population(gpu, m0, p0, 1.0)
    pop.set_schedule([ids], client="none")
    pop.round()
    _, p = _oracle_round(m0, p0, ids, 1.0, client=("none", 1.0, 1.0))
    if step == "last":  # the oracle's own result there is the IEEE quotient of the tie
        assert np.array_equal(p[pos], _tie(o) / np.float32(C)) and np.array_equal(p[neg], -_tie(o) / np.float32(C))
    assert _same(pop.params, p), (o, step, pop.params[pos].cpu().numpy().view(np.uint32), p[pos].view(np.uint32))


@pytest.mark.parametrize("o", sorted(TIES))
def test_mix_client_exact_subnormal_ties(gpu, o):
    """The same ties in the mix client's step w + 1 * (g - w) / d_c with d_c = 2o: g holds the tie
    values where every row holds 0 (an empty active list leaves params as they are)."""
    P = 4 * (_tile() + 3) + 2
    rng = np.random.default_rng(70 + o)
    m0 = rng.standard_normal((D, P)).astype(np.float32)
    p0 = rng.standard_normal(P).astype(np.float32)
    pos, neg = _tie_vectors(P)
    m0[:, pos] = m0[:, neg] = 0.0
    p0[pos], p0[neg] = _tie(o), -_tie(o)
    client = ("mix", 1.0, float(2 * o))
    pop = _population(gpu, m0, p0, 1.0)
    pop.set_schedule([[]], client="mix", client_factor=1.0, client_divisor=float(2 * o))
    pop.round()
    m, p = _oracle_round(m0, p0, [], 1.0, client=client)
    assert np.array_equal(m[3, pos], _tie(o) / np.float32(2 * o))
    assert _same(pop.params, p0) and _same(pop.models, m), o


SCHED, TABLES = [1, 0, 1], [[3, 1, 4, 1, 5], [9, 2, 6]]  # S = 3 slots over T = 2 tables


@functools.lru_cache(maxsize=None)
def _schedule_reference(R=9):
    """A host loop over the oracle: (models, params) after each of R rounds, read-only."""
    rng = np.random.default_rng(80)
    P = 4 * _tile() + 4 + 3
    m = rng.standard_normal((D, P)).astype(np.float32)
    p = rng.standard_normal(P).astype(np.float32)
    out = [(m, p)]
    for r in range(R):
        m, p = _oracle_round(m, p, TABLES[SCHED[r % 3]], 0.7, client=("mix", 1.0, 2.0))
        m.setflags(write=False)
        p.setflags(write=False)
        out.append((m, p))
    return out


def _scheduled(gpu):
    m0, p0 = _schedule_reference()[0]
    pop = _population(gpu, m0, p0, 0.7)
    pop.set_schedule(TABLES, sched=SCHED, client="mix", client_factor=1.0, client_divisor=2.0)
    return pop


def test_schedule_eager_graph_and_reset(gpu):
    """7 rounds of S = 3 slots over T = 2 tables: replayed from graphs == eager == the host loop
    over the oracle; reset_round(1) makes the next round use sched[1]."""
    ref = _schedule_reference()
    eager, graph = _scheduled(gpu), _scheduled(gpu)
    for r in range(7):
        eager.round()
        assert _same(eager.models, ref[r + 1][0]) and _same(eager.params, ref[r + 1][1]), r
    graph.rounds(7, graph=True)
    assert torch.equal(graph.models.view(torch.int32), eager.models.view(torch.int32))
    assert torch.equal(graph.params.view(torch.int32), eager.params.view(torch.int32))
    assert graph.round_index == 7 and eager.round_index == 7
    graph.rounds(2, graph=True)  # goes on from round 7
    assert _same(graph.models, ref[9][0]) and _same(graph.params, ref[9][1]) and graph.round_index == 9
    # reset_round(3): the next round folds sched[0] = table 1 into the models of round 7 (round 7
    # itself would have folded sched[1] = table 0)
    m7, p7 = ref[7]
    eager.reset_round(3)
    eager.round()
    m, p = _oracle_round(m7, p7, TABLES[SCHED[0]], 0.7, client=("mix", 1.0, 2.0))
    assert _same(eager.models, m) and _same(eager.params, p) and eager.round_index == 4
    assert not _same(eager.params, ref[8][1])  # table 0 would have given another model
    assert eager.bytes_per_round() == (len(TABLES[SCHED[4 % 3]]) + 1 + D + 1 + D) * m7.shape[1] * 4


def test_counters_are_per_population(gpu):
    ref = _schedule_reference()
    a, b = _scheduled(gpu), _scheduled(gpu)
    a.round()
    a.round()
    b.round()
    a.rounds(1, graph=True)
    b.rounds(1, graph=False)
    assert (a.round_index, b.round_index) == (3, 2)
    assert _same(a.params, ref[3][1]) and _same(a.models, ref[3][0])
    assert _same(b.params, ref[2][1]) and _same(b.models, ref[2][0])


def test_server_fold_equals_mix_seq_div(gpu):
    """One round with client="none" == Engine.mix_seq_div over the same rows, bit for bit, at
    C = 17 (two passes of the 16-wide mix) and P = 3M + 7 rounded down to a multiple of 4."""
    C, P = 17, (3 * (1 << 20) + 7) // 4 * 4
    g = torch.Generator(device="cuda").manual_seed(90)
    models = torch.randn(D, P, device="cuda", generator=g)
    params = torch.randn(P, device="cuda", generator=g)
    ids = np.random.default_rng(90).permutation(D)[:C].tolist()
    want = torch.empty(P, device="cuda")
    gpu.mix_seq_div(want, params, [models[k] for k in ids], [0.9] * C, [float(C)] * C)
    from federated_amd.fedavg_population import FedAvgPopulation
    before = models.clone()
    pop = FedAvgPopulation(gpu, models, params, 0.9)
    pop.set_schedule([ids], client="none")
    pop.round()
    assert torch.equal(params.view(torch.int32), want.view(torch.int32))
    assert torch.equal(models.view(torch.int32), before.view(torch.int32))
    assert pop.bytes_per_round() == (C + 2) * P * 4


def test_engine_argument_errors(gpu):
    from federated_amd import _lib
    P = 1024
    models = torch.zeros(4, P, device="cuda")
    params = torch.zeros(P, device="cuda")
    tabs = [torch.tensor(a, device="cuda") for a in ([0, 2], [1, 3])]
    tabs = [t.to(torch.int32) for t in tabs] + [torch.tensor([2.0], device="cuda"),
                                                 torch.tensor([0.5], dtype=torch.float64, device="cuda")]
    sched = torch.zeros(1, dtype=torch.int32, device="cuda")
    rnd = torch.zeros(1, dtype=torch.int64, device="cuda")

    def call(models=models, params=params, tabs=tabs, sched=sched, rnd=rnd, **kw):
        gpu.fedavg_round(models, params, *tabs, 1.0, sched, rnd, **kw)

    call()  # the arguments are fine as they are
    assert int(rnd.item()) == 1
    with pytest.raises((TypeError, ValueError)):  # a wrong device
        call(models=models.cpu())
    with pytest.raises((TypeError, ValueError)):
        call(params=params.cpu())
    with pytest.raises(TypeError):
        call(tabs=[tabs[0].cpu()] + tabs[1:])
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="this engine runs on"):
            call(params=params.to("cuda:1"))
    with pytest.raises(TypeError):  # a wrong dtype
        call(models=models.double())
    with pytest.raises(TypeError):
        call(tabs=[tabs[0].long()] + tabs[1:])
    with pytest.raises(TypeError):
        call(tabs=tabs[:3] + [tabs[3].float()])
    with pytest.raises(TypeError):
        call(sched=sched.long())
    with pytest.raises(TypeError):
        call(ended=torch.zeros(4, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        call(ended=torch.zeros(5, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        call(params=torch.zeros(P + 4, device="cuda"))
    with pytest.raises(_lib.CFAError, match="16-byte aligned"):  # a misaligned pitch
        call(models=torch.zeros(4, P + 1, device="cuda")[:, :P])
    with pytest.raises(_lib.CFAError, match="16-byte aligned"):  # a misaligned base
        call(models=torch.zeros(4, P + 4, device="cuda")[:, 1:P + 1])
    with pytest.raises(_lib.CFAError, match="below P"):  # pitch < P: overlapping rows
        call(models=torch.as_strided(torch.zeros(4 * P, device="cuda"), (4, P), (P - 4, 1)))
    with pytest.raises(_lib.CFAError, match="unknown client rule"):
        call(client=7)
    with pytest.raises(_lib.CFAError, match="d_c is 0"):
        call(client=_lib.CLIENT_MIX, client_divisor=0.0)
    assert int(rnd.item()) == 1  # no refused call advanced the counter
