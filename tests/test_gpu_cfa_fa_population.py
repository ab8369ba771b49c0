"""The TF1 CFA-FA server epoch on a device-resident population (cfa_fa_population_round_f32,
federated_amd/cfa_fa_population.py). The reference of every case is numpy fp64 built from
oracle.cfa_oracle.cfa_fa_server_init / cfa_fa_server_round / cfa_fa_client_mix (the driver's lines
:86-89, :103-110 / :130-133, :280-283), the client result cast by .astype(np.float32). Parity is bit
for bit on the rows and on the server model: the chain has one order, so there is nothing to
tolerate."""
import os

import numpy as np
import pytest
import torch

from oracle import cfa_oracle as orc

pytestmark = pytest.mark.gpu

KEYS = ("weights1", "biases1", "weights2", "biases2")
EPS, EPS2 = 0.37, 0.61  # not powers of two
DS = (1, 2, 4, 5, 8, 9, 19)  # below, at and beyond both load batches (4 and 8)


@pytest.fixture
def workdir(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("FEDERATED_AMD_PAUSE_SCALE", "0")
    os.makedirs("results")
    return tmp_path


def _bal(D, seed=0):
    return np.random.default_rng(100 + seed + D).uniform(0.05, 0.4, D)  # non-uniform balancing_vect


def _parts(v):
    """A [P] vector as the four arrays the oracle's functions take (the operations are per element)."""
    return dict(zip(KEYS, np.array_split(v, 4)))


def _ref_epoch(x, s, bal, eps, eps2, init):
    """One server epoch in numpy: x [D, P] fp32, s [P] fp64 -> (rows fp32 [D, P], s fp64 [P])."""
    contents = [_parts(row) for row in x]
    s4 = [_parts(s)[k] for k in KEYS]
    if init:
        s4 = orc.cfa_fa_server_init(s4, contents, bal)
        return x.copy(), np.concatenate(s4)
    s4 = orc.cfa_fa_server_round(s4, contents, eps, bal)
    srv = dict(zip(KEYS, s4))
    rows = []
    for c in contents:
        w = orc.cfa_fa_client_mix(c["weights1"], c["biases1"], c["weights2"], c["biases2"], srv, eps2)
        rows.append(np.concatenate([np.atleast_1d(a) for a in w]).astype(np.float32))
    return np.stack(rows), np.concatenate(s4)


def _inputs(D, P, seed):
    """Rows and a server model in which x_d - s, x_d - x_0 and s - W cancel exactly in some columns."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((D, P)) * 0.3).astype(np.float32)
    s = rng.standard_normal(P) * 0.3
    s[::7] = x[0, ::7]
    x[1:, ::11] = x[0, ::11]
    x[-1, ::5] = 0.0
    s[3::13] = 0.0
    return x, s


def _coef(bal, eps, init):
    return np.asarray(bal, np.float64) if init else np.asarray([eps * b for b in bal], np.float64)


SENTINEL = -7.25


def _stacks(x, s, layout):
    """(in view, out view, out stack, server view) on the device for a layout."""
    D, P = x.shape
    if layout == "pitched":  # 16-byte aligned rows, pitch > P: the float4 form with its scalar tail
        pitch = (P + 4) // 4 * 4 + 4
        src = torch.full((D, pitch), SENTINEL, device="cuda")
        dst = torch.full((D, pitch), SENTINEL, device="cuda")
        src[:, :P] = torch.from_numpy(x)
        sv = torch.from_numpy(s).cuda()
        return src[:, :P], dst[:, :P], dst, sv
    src = torch.from_numpy(x).cuda()  # contiguous: rows of an odd P are not 16-byte aligned
    dst = torch.full((D, P), SENTINEL, device="cuda")
    if layout == "server_offset":  # the server model one double into its allocation
        buf = torch.zeros(P + 1, dtype=torch.float64, device="cuda")
        buf[1:] = torch.from_numpy(s)
        return src, dst, dst, buf[1:]
    return src, dst, dst, torch.from_numpy(s).cuda()


def _sizes(lib):
    t4, t1 = int(lib.cfa_fa_round_tile(1, 1)), int(lib.cfa_fa_round_tile(1, 0))
    assert t4 % 1024 == 0 and t1 % 256 == 0
    return sorted({1, 3, 4, 5, 1488, 1489, 4095, 4096, 4097, 8191, 8193, t4 - 1, t4 + 1, 2 * t4 + 1, t1 + 1})


@pytest.mark.parametrize("batch", ["4", "8"])
@pytest.mark.parametrize("layout", ["contiguous", "pitched", "server_offset"])
@pytest.mark.parametrize("init", [True, False], ids=["init", "round"])
def test_server_epoch_bit_for_bit(gpu, monkeypatch, init, layout, batch):
    """Both modes, every D around both load batches, sizes around the tile, aligned and unaligned
    rows, a pitched stack and an offset server model, non-uniform balancing."""
    from federated_amd import _lib
    monkeypatch.setenv("CFA_FA_BATCH", batch)
    mode = _lib.FA_INIT if init else _lib.FA_ROUND
    for D in DS:
        bal = _bal(D)
        coef = torch.from_numpy(_coef(bal, EPS, init)).cuda()
        for P in _sizes(_lib.load()):
            x, s = _inputs(D, P, 1000 * D + P)
            want_rows, want_s = _ref_epoch(x, s, bal, EPS, EPS2, init)
            src, dst, dst_stack, sv = _stacks(x, s, layout)
            gpu.cfa_fa_round(dst, src, sv, coef, EPS2, mode)
            torch.cuda.synchronize()
            assert np.array_equal(sv.cpu().numpy(), want_s), ("server", D, P)
            assert np.array_equal(dst.cpu().numpy(), want_rows), ("rows", D, P)
            assert np.array_equal(src.cpu().numpy(), x), ("in is only read", D, P)
            if layout == "pitched":
                assert bool((dst_stack[:, P:] == SENTINEL).all()), ("columns past P", D, P)
    if not init:  # the inputs do exercise the cancellations
        assert np.any(want_rows != x) and np.any(x[0] == s.astype(np.float32))


@pytest.mark.parametrize("layout", ["pitched", "contiguous"])
@pytest.mark.parametrize("D", [3, 9])
def test_grid_stride_loop(gpu, monkeypatch, D, layout):
    """Two workgroups walk five tiles and a partial one (CFA_FA_MAX_GRID caps the grid): several
    strides per workgroup, the partial tile owned by the second, the < 4-element tail."""
    from federated_amd import _lib
    monkeypatch.setenv("CFA_FA_MAX_GRID", "2")
    tile = int(_lib.load().cfa_fa_round_tile(1, 1 if layout == "pitched" else 0))
    P = 5 * tile + tile // 2 + 3
    x, s = _inputs(D, P, 77 + D)
    bal = _bal(D)
    want_rows, want_s = _ref_epoch(x, s, bal, EPS, EPS2, False)
    src, dst, _, sv = _stacks(x, s, layout)
    gpu.cfa_fa_round(dst, src, sv, torch.from_numpy(_coef(bal, EPS, False)).cuda(), EPS2, _lib.FA_ROUND)
    torch.cuda.synchronize()
    assert np.array_equal(sv.cpu().numpy(), want_s) and np.array_equal(dst.cpu().numpy(), want_rows)


def test_empty_population_and_empty_rows(gpu):
    """D == 0 leaves the server model as it is; P == 0 launches nothing."""
    from federated_amd import _lib
    s = torch.arange(40, dtype=torch.float64, device="cuda")
    e = torch.empty(0, 40, device="cuda")
    gpu.cfa_fa_round(torch.empty(0, 40, device="cuda"), e, s, torch.empty(0, dtype=torch.float64, device="cuda"), EPS2,
                     _lib.FA_ROUND)
    torch.cuda.synchronize()
    assert torch.equal(s, torch.arange(40, dtype=torch.float64, device="cuda"))
    gpu.cfa_fa_round(torch.empty(3, 0, device="cuda"), torch.empty(3, 0, device="cuda"),
                     torch.empty(0, dtype=torch.float64, device="cuda"), torch.ones(3, dtype=torch.float64, device="cuda"),
                     EPS2, _lib.FA_INIT)


def test_refusals(gpu):
    """The C entry returns CFA_E_INVALID with a message, Engine raises, and nothing is launched."""
    import ctypes
    from federated_amd import _lib
    lib = _lib.load()
    D, P = 3, 40
    src = torch.zeros(D, P, device="cuda")
    dst = torch.full((D, P), SENTINEL, device="cuda")
    s = torch.zeros(P, dtype=torch.float64, device="cuda")
    coef = torch.ones(D, dtype=torch.float64, device="cuda")
    last = lambda: lib.cfa_last_error().decode()
    call = lambda *a: lib.cfa_fa_population_round_f32(*a)
    good = [dst.data_ptr(), P, src.data_ptr(), P, s.data_ptr(), coef.data_ptr(), ctypes.c_double(EPS2), _lib.FA_ROUND, D, P,
            None]

    def bad(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return call(*a)

    INVALID = lib.cfa_fa_population_round_f32(None, 0, None, 0, None, None, ctypes.c_double(0.0), 7, 0, 0, None)
    assert INVALID != 0 and "mode" in last()
    assert bad(a0=None) == INVALID and "null" in last()
    assert bad(a2=None) == INVALID and bad(a4=None) == INVALID and bad(a5=None) == INVALID
    assert bad(a8=-1) == INVALID and "negative" in last()
    assert bad(a1=P - 1) == INVALID and "pitch" in last()
    assert bad(a3=P - 1) == INVALID and "pitch" in last()
    assert bad(a7=2) == INVALID and "mode" in last()
    assert bad(a0=src.data_ptr()) == INVALID and "overlaps" in last()
    assert bad(a0=src.data_ptr() + 4 * (D * P - 1)) == INVALID and "overlaps" in last()
    assert bad(a9=0) == 0  # P == 0: CFA_OK
    torch.cuda.synchronize()
    assert bool((dst == SENTINEL).all()) and bool((s == 0).all())
    with pytest.raises(ValueError, match="like models"):
        gpu.cfa_fa_round(dst[:2], src, s, coef, EPS2)
    with pytest.raises(ValueError, match="expected 40"):
        gpu.cfa_fa_round(dst, src, s[:39], coef, EPS2)
    with pytest.raises(TypeError, match="server"):
        gpu.cfa_fa_round(dst, src, s.float(), coef, EPS2)
    with pytest.raises(ValueError, match="one fp64 coefficient per device"):
        gpu.cfa_fa_round(dst, src, s, coef[:2], EPS2)
    with pytest.raises(TypeError, match="coef"):
        gpu.cfa_fa_round(dst, src, s, coef.float(), EPS2)
    with pytest.raises(ValueError, match="mode"):
        gpu.cfa_fa_round(dst, src, s, coef, EPS2, 5)
    with pytest.raises(TypeError, match="unit element stride"):
        gpu.cfa_fa_round(dst, src.t().contiguous().t(), s, coef, EPS2)
    from federated_amd._lib import CFAError
    with pytest.raises(CFAError, match="overlaps"):
        gpu.cfa_fa_round(src, src, s, coef, EPS2)
    torch.cuda.synchronize()
    assert bool((dst == SENTINEL).all()) and bool((s == 0).all())


# ------------------------------------------------------------------ the population class
TF1_SHAPES = [(16, 1, 8), (8,), (168, 8), (8,)]  # the driver's CNN bucket, P = 1 488
P_TF1 = 1488


def _population(gpu, D, P, N, cycle, seed, topology=True, balancing="default"):
    from federated_amd import topology as T
    from federated_amd.cfa_fa_population import CfaFaPopulation
    bal = None if isinstance(balancing, str) else balancing
    p = CfaFaPopulation(gpu, D, P, EPS, EPS2, bal)
    p.set_cycle(cycle)
    if topology:
        p.set_topology(T.kregular_tf1(D, N), T.alphas_tf1_cfa(EPS, N))
    rng = np.random.default_rng(seed)
    cur = (rng.standard_normal((D, P)) * 0.1).astype(np.float32)
    prev = (rng.standard_normal((D, P)) * 0.1).astype(np.float32)
    p.load(torch.from_numpy(cur).cuda(), torch.from_numpy(prev).cuda())
    return p, cur, prev


def test_whole_run_reproduces_the_dropin(gpu, workdir):
    """D = 5, N = 2, P = 1 488, cfa_fa_cycle(3, 3), 13 epochs; the "training" of an epoch is a fixed
    fp32 perturbation of every model. Beside it every device calls the drop-in CFA_process through
    the .mat files (consensus disabled in server epochs) and the server's and clients' steps are
    server.cfa_fa_server_init / _round / cfa_fa_client_mix on the published files. Server model and
    rows agree bit for bit after every epoch, consensus epochs included (the Tf1PopulationRound
    path is bit for bit against the drop-in: test_gpu_trajectory)."""
    import scipy.io as sio
    from federated_amd import server as srv
    from federated_amd.cfa_fa_population import cfa_fa_cycle
    from federated_amd.consensus.cfa import CFA_process
    D, N, E = 5, 2, 13
    cycle = cfa_fa_cycle(3, 3)
    sizes = [int(np.prod(s)) for s in TF1_SHAPES]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    split = lambda v: [v[offs[k]:offs[k + 1]].reshape(TF1_SHAPES[k]) for k in range(4)]
    flat = lambda m: np.concatenate([np.asarray(a).reshape(-1) for a in m])
    pop, cur, _ = _population(gpu, D, P_TF1, N, cycle, 5)
    rng = np.random.default_rng(55)
    pert = (rng.standard_normal((E, D, P_TF1)) * 0.01).astype(np.float32)
    procs = [CFA_process(True, D, d, N) for d in range(D)]
    bal = np.ones(D) * (1 / D)
    server4 = [np.zeros(s) for s in TF1_SHAPES]
    models = cur
    for e in range(E):
        trained = models + pert[e]  # fp32
        pop.current.add_(torch.from_numpy(pert[e]).cuda())
        is_server = cycle[e % len(cycle)] == "server"
        outs = []
        for d in range(D):
            W1, b1, W2, b2 = split(trained[d])
            procs[d].disable_consensus(not is_server)
            outs.append(procs[d].getFederatedWeight(W1, W2, b1, b2, e, np.zeros(3), EPS))
        if is_server:
            contents = [sio.loadmat(f"datamat{d}_{e}.mat") for d in range(D)]
            if e == 0:
                server4 = srv.cfa_fa_server_init(server4, contents, bal)
            else:
                server4 = srv.cfa_fa_server_round(server4, contents, EPS, bal)
                content = dict(zip(KEYS, server4))
                outs = [srv.cfa_fa_client_mix(*o, content, EPS2) for o in outs]
        models = np.stack([flat([np.asarray(a).astype(np.float32) for a in o]) for o in outs])  # the fp32 placeholders
        assert pop.phase() == cycle[e % len(cycle)] and pop.epoch_index == e
        pop.round()
        torch.cuda.synchronize()
        assert np.array_equal(pop.current.cpu().numpy(), models), ("rows", e)
        assert np.array_equal(pop.previous.cpu().numpy(), trained), ("published", e)
        assert np.array_equal(pop.server.cpu().numpy(), flat(server4)), ("server", e)
    assert pop.epoch_index == E


@pytest.mark.parametrize("start", [0, 4])
@pytest.mark.parametrize("R", [1, 7, 40])
def test_rounds_graph_equals_eager(gpu, R, start):
    """rounds(R, graph=True) against R eager round() calls, from epoch 0 (the init epoch runs outside
    the graphs) and from a mid-cycle reset_epoch: rows, previous, server and epoch_index."""
    cycle = ["server", "server", "consensus", "server", "consensus"]
    D, P = 5, 1489
    pops = [_population(gpu, D, P, 2, cycle, 9, balancing=_bal(D))[0] for _ in range(2)]
    for p in pops:
        p.server.copy_(torch.linspace(-1, 1, P, dtype=torch.float64))
        p.reset_epoch(start)
    a, b = pops
    a.rounds(R, graph=True)
    b.rounds(R, graph=False)
    torch.cuda.synchronize()
    assert a.epoch_index == b.epoch_index == start + R
    assert torch.equal(a.current, b.current) and torch.equal(a.previous, b.previous) and torch.equal(a.server, b.server)
    a.rounds(len(cycle) + 1, graph=True)  # again, now from cached graphs of another rotation
    b.rounds(len(cycle) + 1, graph=False)
    torch.cuda.synchronize()
    assert a.epoch_index == b.epoch_index
    assert torch.equal(a.current, b.current) and torch.equal(a.previous, b.previous) and torch.equal(a.server, b.server)
    assert bool(torch.isfinite(a.current).all())


def test_bytes_per_round(gpu):
    D, P = 5, 1488
    p = _population(gpu, D, P, 2, ["server", "consensus"], 3)[0]
    assert p.bytes_per_round() == 2 * D * P * 4 + 16 * P
    p.round()
    assert p.phase() == "consensus" and p.bytes_per_round() == (D * 3 + D) * P * 4


CNN_ODD = {"filter": 4, "number": 6, "stride": 4, "input_data": 37, "classes": 5}


def test_epochs_with_local_training_graph_equals_eager(gpu):
    """epochs(R) with a real LocalSgd (the CNN at a small geometry) chained to the cycle: graph
    replay equals eager epochs bit for bit, models, server model and both cost logs."""
    from federated_amd.local_training import LocalSgd, model_size
    D, Ns, Nt, R = 4, 14, 9, 11
    L, C = CNN_ODD["input_data"], CNN_ODD["classes"]
    geom = {k: v for k, v in CNN_ODD.items() if k not in ("input_data", "classes")}
    P = model_size(1, geom, L, C)
    rng = np.random.default_rng(21)
    cuda = lambda a: torch.from_numpy(a).cuda()
    x, xt = (rng.standard_normal((D, n, L)).astype(np.float32) for n in (Ns, Nt))
    y, yt = (np.eye(C, dtype=np.float32)[rng.integers(0, C, (D, n))] for n in (Ns, Nt))
    pops = []
    for _ in range(2):
        p = _population(gpu, D, P, 2, ["server", "server", "consensus"], 31)[0]
        p.set_local_training(LocalSgd(gpu, 1, geom, cuda(x), cuda(y), 0.05, cuda(xt), cuda(yt), log_cap=R))
        pops.append(p)
    a, b = pops
    start = a.current.clone()
    a.epochs(R, graph=True)
    b.epochs(R, graph=False)
    torch.cuda.synchronize()
    assert a.epoch_index == b.epoch_index == R
    assert torch.equal(a.current, b.current) and torch.equal(a.previous, b.previous) and torch.equal(a.server, b.server)
    assert not torch.equal(a.current, start)
    for name in ("train_log", "val_log", "train_cost", "val_cost"):
        assert torch.equal(getattr(a._local, name), getattr(b._local, name)), name
    assert a._local.epochs_done == R and bool(torch.isfinite(a._local.val_log).all())


def test_strict_capture_and_identical_runs(gpu):
    """The launch captures under the strict mode (nothing is queried or allocated at launch) and a
    replay, a second replay from the same state and an eager launch give identical bits."""
    from federated_amd import _lib
    D, P = 9, 4 * 1024 + 3
    x, s = _inputs(D, P, 4)
    coef = torch.from_numpy(_coef(_bal(D), EPS, False)).cuda()
    src = torch.from_numpy(x).cuda()
    outs, servers = [], []
    sv, dst = torch.from_numpy(s).cuda(), torch.empty(D, P, device="cuda")
    g = torch.cuda.CUDAGraph()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=st, capture_error_mode="global"):
        gpu.cfa_fa_round(dst, src, sv, coef, EPS2, _lib.FA_ROUND)
    for k in range(3):
        sv.copy_(torch.from_numpy(s))
        dst.fill_(SENTINEL)
        if k < 2:
            g.replay()
        else:
            gpu.cfa_fa_round(dst, src, sv, coef, EPS2, _lib.FA_ROUND)
        torch.cuda.synchronize()
        outs.append(dst.clone()), servers.append(sv.clone())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert torch.equal(servers[0], servers[1]) and torch.equal(servers[0], servers[2])
    want_rows, want_s = _ref_epoch(x, s, _bal(D), EPS, EPS2, False)
    assert np.array_equal(outs[0].cpu().numpy(), want_rows) and np.array_equal(servers[0].cpu().numpy(), want_s)


def test_population_refusals(gpu):
    from federated_amd.cfa_fa_population import CfaFaPopulation
    p = CfaFaPopulation(gpu, 4, 64, EPS, EPS2)
    with pytest.raises(RuntimeError, match="set_cycle"):
        p.round()
    with pytest.raises(ValueError, match='must be "server"'):
        p.set_cycle(["consensus"])
    p.set_cycle(["server", "consensus"])
    p.round()
    before = (p.current.clone(), p.server.clone())
    with pytest.raises(RuntimeError, match="set_topology"):
        p.round()  # a consensus epoch without a topology
    with pytest.raises(RuntimeError, match="set_topology"):
        p.rounds(4)
    assert p.epoch_index == 1 and torch.equal(p.current, before[0]) and torch.equal(p.server, before[1])
    with pytest.raises(ValueError, match="each of the 4 devices"):
        CfaFaPopulation(gpu, 4, 64, EPS, EPS2, [0.5, 0.5])
    with pytest.raises(ValueError, match=">= 0"):
        p.reset_epoch(-1)


def test_tf1_population_is_unchanged_beside_the_new_class(gpu):
    """Tf1PopulationRound rounds on a fixed seed: the same bits before and after the new class is
    imported, constructed and run, and the same bits as the new class's consensus epochs."""
    from federated_amd import topology as T
    D, P, N = 6, 1488, 2
    rng = np.random.default_rng(12)
    cur = torch.from_numpy((rng.standard_normal((D, P)) * 0.1).astype(np.float32)).cuda()
    prev = torch.from_numpy((rng.standard_normal((D, P)) * 0.1).astype(np.float32)).cuda()

    def run():
        p = T.Tf1PopulationRound(gpu, D, P)
        p.set_topology(T.kregular_tf1(D, N), T.alphas_tf1_cfa(EPS, N))
        p.load(cur, prev)
        p.rounds(4, graph=False)
        torch.cuda.synchronize()
        return p.current.clone(), p.previous.clone()

    first = run()
    q = _population(gpu, D, P, N, ["server", "consensus", "consensus", "consensus", "consensus"], 1)[0]
    q.load(cur, prev)
    q.reset_epoch(1)
    q.rounds(4, graph=False)
    torch.cuda.synchronize()
    again = run()
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    assert torch.equal(q.current, first[0]) and torch.equal(q.previous, first[1])
    assert bool((q.server == 0).all())
