"""Local training on the device (cfa_local_sgd_{cnn,2nn}_f32, Engine.local_sgd, LocalSgd and the
epoch() / epochs() hooks of CfaGePopulation and Tf1PopulationRound) against the reference epoch
restated here: the loop of federated_sample_CNN_CFA-GE.py:137-173 over minibatches with
``w -= lr * g``, the gradients from oracle.cfa_oracle.tf1_cnn_grads / tf1_2nn_grads as they are.

Tolerance. One step is held to the project's standing bar, 1e-5 normwise per tensor against the
float64 restatement. Over several steps a rounding difference passes through the later gradients,
so the test measures the arithmetic's own spread: the restated epoch is run twice on the CPU, in
float64 and with every quantity that crosses a step held in fp32 (the model, each gradient, the
update ``w - lr * g`` and the minibatch cost are rounded to fp32; the gradient itself is the
oracle's), and ``s`` is their normwise distance per tensor. The kernel is allowed
``max(1e-5, 4 * s)`` against the float64 result (4: another summation order inside a minibatch),
and ``s`` itself must stay below 1e-4, so the allowance cannot swallow a wrong gradient. The mean
cost is held to 1e-5 relative.

``s`` on the CPU for the cases below (lr 0.05, unit-variance samples; the largest over devices,
tensors, both slicings and steps 1, 2, 7):

    shape                           1 step     2 steps    7 steps
    CNN C3 (P 1 488)                4.9e-08    8.5e-08    1.8e-07
    CNN odd (L 37, S 4, F 4)        5.0e-08    1.0e-07    1.8e-07
    2NN C1 (P 16 680)               5.6e-08    7.3e-08    1.7e-07
    2NN tiny (L 20, H 5, C 3)       5.5e-08    7.9e-08    1.4e-07

and at most 7.0e-08 per tensor for the two-step epochs of the whole-epoch case, so 4 * s is
below 1e-6 and the allowance is the standing 1e-5 in every case here.
"""
import numpy as np
import pytest
import torch

from conftest import normwise_close
from oracle import cfa_oracle as orc

pytestmark = pytest.mark.gpu

CNN_C3 = {"filter": 16, "number": 8, "stride": 5, "input_data": 512, "classes": 8}   # the <16, 5> kernel
CNN_ODD = {"filter": 4, "number": 6, "stride": 4, "input_data": 37, "classes": 5}    # runtime loops, L % S != 0
NN_C1 = {"intermediate_nodes": 32, "input_data": 512, "classes": 8}
NN_TINY = {"intermediate_nodes": 5, "input_data": 20, "classes": 3}
SHAPES = {"cnn_c3": (1, CNN_C3), "cnn_odd": (1, CNN_ODD), "2nn_c1": (2, NN_C1), "2nn_tiny": (2, NN_TINY)}
NAMES = ("W1", "b1", "W2", "b2")
LR = 0.05
S_MAX = 1e-4


def _layout(ml, geom):
    shapes = orc.tf1_flat_shapes(ml, geom)
    offs = [int(o) for o in np.concatenate([[0], np.cumsum([int(np.prod(s)) for s in shapes])])]
    return shapes, offs


def _kernel_geom(geom):
    return {k: v for k, v in geom.items() if k not in ("input_data", "classes")}


def _split4(w, shapes, offs):
    return [w[offs[k]:offs[k + 1]].reshape(shapes[k]) for k in range(4)]


def _cost(ml, geom, xb, yb, w4):
    """The clipped cross-entropy of one minibatch, float64 (:425-426)."""
    if ml == 1:
        logits = orc.tf1_cnn_forward(xb, *w4, stride=geom["stride"])[0]
    else:
        W1, b1, W2, b2 = (np.asarray(a, np.float64) for a in w4)
        logits = np.maximum(np.asarray(xb, np.float64) @ W1 + b1, 0.0) @ W2 + b2
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    pred = e / e.sum(axis=1, keepdims=True)
    return float(np.mean(-np.sum(np.asarray(yb, np.float64) * np.log(np.clip(pred, 1e-15, 0.99)), axis=1)))


def ref_epoch(ml, geom, x, y, w0, stride, rows, steps, lr, dtype, update=True):
    """One device's epoch: (final flat model, mean minibatch cost). ``dtype`` float64: the
    reference; float32: everything that crosses a step is rounded to fp32 (see the docstring).
    The learning rate is the fp32 value the kernel receives."""
    shapes, offs = _layout(ml, geom)
    w = np.asarray(w0, dtype).copy()
    lr = dtype(np.float32(lr))
    mean = 0.0
    for i in range(steps):
        xb, yb = x[i * stride:i * stride + rows], y[i * stride:i * stride + rows]
        w4 = _split4(w, shapes, offs)
        if update:
            if ml == 1:
                g, c = orc.tf1_cnn_grads(xb, yb, *w4, stride=geom["stride"])
            else:
                g, c = orc.tf1_2nn_grads(xb, yb, *w4)
            g = np.concatenate([a.reshape(-1) for a in g]).astype(dtype)
            w = (w - lr * g).astype(dtype)
        else:
            c = _cost(ml, geom, xb, yb, w4)
        mean += float(dtype(c)) / steps
    return w, mean


def _data(seed, ml, geom, D, Ns, scale_w=0.2):
    rng = np.random.default_rng(seed)
    P = _layout(ml, geom)[1][4]
    L, C = geom["input_data"], geom["classes"]
    x = rng.standard_normal((D, Ns, L)).astype(np.float32)
    y = np.eye(C, dtype=np.float32)[rng.integers(0, C, (D, Ns))]
    W = (rng.standard_normal((D, P)) * scale_w).astype(np.float32)
    return x, y, W


def _cuda(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()  # a copy: the shared reference arrays are read-only


_REF = {}


def reference(name, stride, rows, steps, update=True):
    """The restated epochs of one case, computed once and shared: the data, the float64 and
    fp32 results per device and the allowance per (device, tensor)."""
    key = (name, stride, rows, steps, update)
    if key not in _REF:
        ml, geom = SHAPES[name]
        D, Ns = 3, 6 * 5 + 4  # room for 7 minibatches at a stride of 5
        x, y, W = _data(sorted(SHAPES).index(name), ml, geom, D, Ns)
        _, offs = _layout(ml, geom)
        w64, w32, c64, allow, spread = [], [], [], [], []
        for d in range(D):
            a, ca = ref_epoch(ml, geom, x[d], y[d], W[d], stride, rows, steps, LR, np.float64, update)
            b, _ = ref_epoch(ml, geom, x[d], y[d], W[d], stride, rows, steps, LR, np.float32, update)
            s = [np.max(np.abs(b[offs[k]:offs[k + 1]] - a[offs[k]:offs[k + 1]]))
                 / np.max(np.abs(a[offs[k]:offs[k + 1]])) for k in range(4)]
            w64.append(a), w32.append(b), c64.append(ca), spread.append(s)
            allow.append([max(1e-5, 4 * v) for v in s])
        for a in (x, y, W):
            a.setflags(write=False)
        _REF[key] = dict(x=x, y=y, W=W, w64=np.stack(w64), c64=np.array(c64), allow=allow, spread=spread)
    return _REF[key]


def _assert_models(got, ref, offs, allow, what):
    for k in range(4):
        a, r = got[offs[k]:offs[k + 1]].astype(np.float64), ref[offs[k]:offs[k + 1]]
        err = np.max(np.abs(a - r)) / np.max(np.abs(r))
        print(f"{what} {NAMES[k]}: normwise error {err:.3e}, allowed {allow[k]:.3e}")
        assert err <= allow[k], (what, NAMES[k], err, allow[k])


def _run(gpu, ml, geom, x, y, W, stride, rows, steps, update=True, pad=3, **kw):
    """One launch on a pitched stack: (models [D, P], padding [D, pad], cost [D])."""
    D, P = W.shape
    stack = torch.full((D, P + pad), 7.5, device="cuda")
    stack[:, :P] = _cuda(W)
    cost = torch.full((D,), float("nan"), dtype=torch.float64, device="cuda")
    gpu.local_sgd(ml, _cuda(x), _cuda(y), stack[:, :P], _kernel_geom(geom), stride, rows, steps, LR, update, cost, **kw)
    torch.cuda.synchronize()
    out = stack.cpu().numpy()
    return out[:, :P], out[:, P:], cost.cpu().numpy()


@pytest.mark.parametrize("stride,rows", [(5, 4), (3, 3)])
@pytest.mark.parametrize("steps", [1, 2, 7])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_epoch_matches_the_restated_loop(gpu, name, steps, stride, rows):
    """Three devices with their own data and starting models, on a pitched stack: every tensor
    within the allowance of the float64 epoch, the cost within 1e-5, the padding untouched."""
    ml, geom = SHAPES[name]
    ref = reference(name, stride, rows, steps)
    _, offs = _layout(ml, geom)
    assert max(max(s) for s in ref["spread"]) < S_MAX
    if steps == 1:
        assert all(a == 1e-5 for dev in ref["allow"] for a in dev)  # the standing bar
    got, padding, cost = _run(gpu, ml, geom, ref["x"], ref["y"], ref["W"], stride, rows, steps)
    assert np.all(padding == 7.5)
    for d in range(got.shape[0]):
        _assert_models(got[d], ref["w64"][d], offs, ref["allow"][d], f"{name} steps {steps} device {d}")
        assert not np.array_equal(got[d], ref["W"][d])
    print("cost", cost, ref["c64"])
    assert np.all(np.abs(cost - ref["c64"]) <= 1e-5 * np.abs(ref["c64"]))


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_validation_mode_leaves_the_models_alone(gpu, name):
    ml, geom = SHAPES[name]
    ref = reference(name, 5, 4, 7, update=False)
    got, padding, cost = _run(gpu, ml, geom, ref["x"], ref["y"], ref["W"], 5, 4, 7, update=False)
    assert np.array_equal(got, ref["W"]) and np.all(padding == 7.5)
    assert np.all(np.abs(cost - ref["c64"]) <= 1e-5 * np.abs(ref["c64"]))


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_two_launches_give_the_same_bits(gpu, name):
    ml, geom = SHAPES[name]
    ref = reference(name, 5, 4, 7)
    a = _run(gpu, ml, geom, ref["x"], ref["y"], ref["W"], 5, 4, 7)
    b = _run(gpu, ml, geom, ref["x"], ref["y"], ref["W"], 5, 4, 7)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("name", ["cnn_c3", "2nn_tiny"])
def test_cost_log_of_chained_epochs(gpu, name):
    """Three chained epochs with a log of two rows: epoch 0 in row 0, epoch 2 in row 1 (the last
    row takes every later epoch), the counter at 3."""
    ml, geom = SHAPES[name]
    ref = reference(name, 5, 4, 2)
    D, P = ref["W"].shape
    x, y, W = _cuda(ref["x"]), _cuda(ref["y"]), _cuda(ref["W"])
    log = torch.full((2, D), float("nan"), dtype=torch.float64, device="cuda")
    epoch = torch.zeros(1, dtype=torch.int64, device="cuda")
    costs = []
    for _ in range(3):
        cost = torch.empty(D, dtype=torch.float64, device="cuda")
        gpu.local_sgd(ml, x, y, W, _kernel_geom(geom), 5, 4, 2, LR, True, cost, log, epoch)
        costs.append(cost)
    torch.cuda.synchronize()
    assert int(epoch.item()) == 3
    assert torch.equal(log[0], costs[0]) and torch.equal(log[1], costs[2])
    assert np.all(np.abs(costs[0].cpu().numpy() - ref["c64"]) <= 1e-5 * np.abs(ref["c64"]))
    assert float(costs[2].sum()) < float(costs[0].sum())  # three epochs of SGD on the same samples


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_one_launch_agrees_with_the_launch_chain(gpu, name):
    """7 steps in one launch against the parent's only on-device path, 7 x (Engine.grad_rows on
    the minibatch's rows + torch W - lr * G), within the same allowance."""
    ml, geom = SHAPES[name]
    ref = reference(name, 5, 4, 7)
    _, offs = _layout(ml, geom)
    D, P = ref["W"].shape
    got, _, _ = _run(gpu, ml, geom, ref["x"], ref["y"], ref["W"], 5, 4, 7)
    x, y, W = _cuda(ref["x"]), _cuda(ref["y"]), _cuda(ref["W"])
    rows = torch.arange(D, dtype=torch.int32, device="cuda")
    G = torch.empty(D, P, device="cuda")
    for i in range(7):
        xb, yb = x[:, 5 * i:5 * i + 4].contiguous(), y[:, 5 * i:5 * i + 4].contiguous()
        gpu.grad_rows(ml, xb, yb, W, rows, rows, G, _kernel_geom(geom))
        W = W - np.float32(LR) * G
    torch.cuda.synchronize()
    chain = W.cpu().numpy()
    for d in range(D):
        _assert_models(chain[d], ref["w64"][d], offs, ref["allow"][d], f"{name} chain device {d}")
        for k in range(4):
            a, b = got[d, offs[k]:offs[k + 1]], chain[d, offs[k]:offs[k + 1]]
            assert normwise_close(a, b, 2 * ref["allow"][d][k]), (d, NAMES[k])


def test_refusals_before_any_launch(gpu):
    ml, geom = SHAPES["2nn_tiny"]
    ref = reference("2nn_tiny", 5, 4, 1)
    x, y, W = _cuda(ref["x"]), _cuda(ref["y"]), _cuda(ref["W"])
    g = _kernel_geom(geom)
    with pytest.raises(ValueError, match="ends at row 39"):
        gpu.local_sgd(ml, x, y, W, g, 5, 4, 8, LR)  # 34 samples hold 7 minibatches
    with pytest.raises(TypeError):
        gpu.local_sgd(ml, x, y, W.double(), g, 5, 4, 1, LR)
    with pytest.raises((TypeError, ValueError)):
        gpu.local_sgd(ml, x, y, W.cpu(), g, 5, 4, 1, LR)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="this engine runs on"):
            gpu.local_sgd(ml, x, y, W.to("cuda:1"), g, 5, 4, 1, LR)
    with pytest.raises(ValueError, match="geometry"):
        gpu.local_sgd(ml, x, y, W[:, :-1], g, 5, 4, 1, LR)
    with pytest.raises(ValueError, match="together"):
        gpu.local_sgd(ml, x, y, W, g, 5, 4, 1, LR, cost_log=torch.zeros(2, 3, dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    assert torch.equal(W, _cuda(ref["W"]))


# ------------------------------------------------------------------ whole epochs
LISTS = [[1, 3], [0, 2], [1, 3], [2, 0]]
EPS, NEIGHBORS, RHO, LR1, LR2 = 0.7, 2, 0.9, 0.1, 0.03


def _ge_population(gpu, x, y, xt, yt, state, log_cap=0):
    from federated_amd.cfa_ge_population import CfaGePopulation
    from federated_amd.local_training import LocalSgd
    g = _kernel_geom(CNN_C3)
    pop = CfaGePopulation(gpu, 1, g, _cuda(x), _cuda(y), LISTS, eps=EPS, neighbors=NEIGHBORS, rho=RHO, lr1=LR1, lr2=LR2)
    pop.load(*(_cuda(a) for a in state))
    pop.set_local_training(LocalSgd(gpu, 1, g, _cuda(x), _cuda(y), LR, _cuda(xt), _cuda(yt), log_cap=log_cap))
    return pop


def _ge_state(seed, D=4, Ns=10, Nt=5):
    rng = np.random.default_rng(seed)
    x, y, W = _data(seed, 1, CNN_C3, D, Ns, scale_w=0.1)
    xt, yt, pub = _data(seed + 1, 1, CNN_C3, D, Nt, scale_w=0.1)
    N, P = 2, W.shape[1]
    S = (rng.standard_normal((D, N, P)) * 0.01).astype(np.float32)
    G = (rng.standard_normal((D, N, P)) * 0.01).astype(np.float32)
    return x, y, xt, yt, (W, pub, S, G)


def test_cfa_ge_epochs_follow_the_restated_loop(gpu):
    """Three eager CfaGePopulation.epoch() calls at D = 4 (C3 geometry, 10 samples: two
    minibatches; 5 test samples: one) beside "local epoch, validation cost, then
    oracle.cfa_ge_population_round". Per epoch: the trained models (they become ``pub``) within
    the local allowance, W after the round within that plus the round's 1e-5, S within 1e-5, G
    within 1e-5 of its bucket (the bound of test_gpu_cfa_ge_rounds.py). As there, each epoch
    starts from the GPU's state, so the bounds do not compound in the comparison."""
    x, y, xt, yt, state = _ge_state(40)
    pop = _ge_population(gpu, x, y, xt, yt, state)
    _, offs = _layout(1, CNN_C3)
    D = 4
    rW, rpub, rS, rG = (a.astype(np.float64) for a in state)
    for e in range(3):
        pop.epoch()
        torch.cuda.synchronize()
        trained, allow, tcost, vcost = [], [], [], []
        for d in range(D):
            w64, c = ref_epoch(1, CNN_C3, x[d], y[d], rW[d], 5, 4, 2, LR, np.float64)
            w32, _ = ref_epoch(1, CNN_C3, x[d], y[d], rW[d], 5, 4, 2, LR, np.float32)
            s = [np.max(np.abs(w32[offs[k]:offs[k + 1]] - w64[offs[k]:offs[k + 1]]))
                 / np.max(np.abs(w64[offs[k]:offs[k + 1]])) for k in range(4)]
            assert max(s) < S_MAX
            trained.append(w64), allow.append([max(1e-5, 4 * v) for v in s]), tcost.append(c)
            vcost.append(ref_epoch(1, CNN_C3, xt[d], yt[d], w64, 5, 4, 1, LR, np.float64, update=False)[1])
        rW, rS, rG, rpub = orc.cfa_ge_population_round(np.stack(trained), rpub, rG, rS, LISTS, x, y, 1, CNN_C3, EPS,
                                                       NEIGHBORS, RHO, LR1, LR2)
        gW, gpub, gS = pop.W.cpu().numpy(), pop.pub.cpu().numpy(), pop.S.cpu().numpy()
        gG = pop.G.cpu().numpy().reshape(D, 2, -1)
        local = pop._local
        assert np.all(np.abs(local.train_cost.cpu().numpy() - tcost) <= 1e-5 * np.abs(tcost))
        assert np.all(np.abs(local.val_cost.cpu().numpy() - vcost) <= 1e-5 * np.abs(vcost))
        for d in range(D):
            _assert_models(gpub[d], rpub[d], offs, allow[d], f"epoch {e} pub[{d}]")
            _assert_models(gW[d], rW[d], offs, [a + 1e-5 for a in allow[d]], f"epoch {e} W[{d}]")
            for n in range(2):
                _assert_models(gS[d, n], rS[d, n], offs, [1e-5] * 4, f"epoch {e} S[{d},{n}]")
                err = np.max(np.abs(gG[d, n] - rG[d, n])) / np.max(np.abs(rG[d, n]))
                assert err <= 1e-5, (e, d, n, err)
        rW, rpub, rS, rG = (a.astype(np.float64) for a in (gW, gpub, gS, gG))


def test_cfa_ge_epochs_graph_equals_eager(gpu):
    """epochs(12, graph=True): two replays of the captured 6-epoch period; models, states,
    gradients and both cost logs equal 12 eager epochs bit for bit."""
    x, y, xt, yt, state = _ge_state(41)
    a, b = (_ge_population(gpu, x, y, xt, yt, state, log_cap=12) for _ in range(2))
    a.epochs(12, graph=True)
    b.epochs(12, graph=False)
    torch.cuda.synchronize()
    for name in ("W", "pub", "S", "G"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    la, lb = a._local, b._local
    assert la.epochs_done == lb.epochs_done == 12
    for name in ("train_log", "val_log", "train_cost", "val_cost"):
        assert torch.equal(getattr(la, name), getattr(lb, name)), name
    assert torch.isfinite(la.train_log).all() and torch.isfinite(la.val_log).all()
    assert not torch.equal(la.train_log[0], la.train_log[11])


def test_tf1_population_epochs_graph_equals_eager(gpu):
    """Tf1PopulationRound.epochs(6) with the tiny 2NN: two replays of the 3-epoch period equal 6
    eager epochs bit for bit, models and cost logs alike."""
    from federated_amd import topology as T
    from federated_amd.local_training import LocalSgd
    D = 4
    x, y, W = _data(50, 2, NN_TINY, D, 10)
    xt, yt, prev = _data(51, 2, NN_TINY, D, 5)
    P = W.shape[1]
    pops = []
    for _ in range(2):
        p = T.Tf1PopulationRound(gpu, D, P)
        p.set_topology(T.kregular_tf1(D, 2), T.alphas_tf1_cfa(0.5, 2))
        p.load(_cuda(W), _cuda(prev))
        p.set_local_training(LocalSgd(gpu, 2, _kernel_geom(NN_TINY), _cuda(x), _cuda(y), LR, _cuda(xt), _cuda(yt),
                                      log_cap=6))
        pops.append(p)
    a, b = pops
    a.epochs(6, graph=True)
    b.epochs(6, graph=False)
    torch.cuda.synchronize()
    assert torch.equal(a.current, b.current) and torch.equal(a.previous, b.previous)
    assert not torch.equal(a.current, _cuda(W))
    for name in ("train_log", "val_log"):
        assert torch.equal(getattr(a._local, name), getattr(b._local, name)), name
    assert a._local.epochs_done == 6 and torch.isfinite(a._local.val_log).all()
    with pytest.raises(ValueError, match="does not match"):
        a.set_local_training(LocalSgd(gpu, 2, _kernel_geom(NN_TINY), _cuda(x[:3]), _cuda(y[:3]), LR))
