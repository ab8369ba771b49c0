"""The local optimizer step of a TF2 population on the device (cfa_optim_step_f32,
Engine.optim_step, PopulationOptimizer) against restatements of the Keras rules kept in this file.
TensorFlow is not installed: parity is to the formulas of the reference's three optimizers
(SGD, SGD with momentum, Adam with clipnorm), not to a TF run.

SGD and momentum are compared bit for bit with an fp32 numpy restatement (the same IEEE
operations in the same order). Adam is compared with a float64 restatement, normwise per
(device, layer) for w, m and v. The allowance is the project's standing 1e-5 as long as the
spread between an fp32 and the float64 restatement on the same inputs stays below it
(measured on these inputs: 1.9e-7 at most; the kernel's largest error is in docs/history.md);
otherwise ten times that spread."""
import gc

import numpy as np
import pytest
import torch

from conftest import normwise_close

pytestmark = pytest.mark.gpu

D = 3
LR, MOM, B1, B2, EPS = 1e-3, 0.9, 0.9, 0.999, 1e-7


def _tile():
    from federated_amd import _lib
    return int(_lib.load().cfa_optim_tile())


def _sizes(pad=0):
    T = _tile()
    return [1, 3, 5, 4, T, T + 1, 2 * T - 3 + pad]


def _table(pad=0):
    return np.concatenate(([0], np.cumsum(_sizes(pad)))).astype(np.int32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


# ---- the restatements ------------------------------------------------------------------------
class Ref:
    """The three rules on numpy arrays [D, P] of ``dtype`` (fp32: every operation rounded to fp32
    in the kernel's order; fp64: the formulas in double). t and the running powers per device."""

    def __init__(self, rule, lp, Dn, dtype, clipnorm=None, trainable=None):
        self.rule, self.lp, self.dt, self.clip = rule, np.asarray(lp, dtype=np.int64), dtype, clipnorm
        n = len(lp) - 1
        self.trainable = np.ones(n, bool) if trainable is None else np.asarray(trainable, bool)
        P = int(lp[-1])
        self.m, self.v = np.zeros((Dn, P), dtype), np.zeros((Dn, P), dtype)
        self.t = np.zeros(Dn, np.int64)
        self.pow = np.ones((Dn, 2), np.float64)
        self.scales = []  # the clip factors of the last step, per stepped device and trainable layer

    def step(self, w, g, skip=None):
        f = self.dt
        lr, mom, eps = f(np.float32(LR)), f(np.float32(MOM)), f(np.float32(EPS))
        omb1, omb2 = (f(np.float32(1.0 - B1)), f(np.float32(1.0 - B2))) if f is np.float32 else (1.0 - B1, 1.0 - B2)
        self.scales = []
        for d in range(w.shape[0]):
            if skip is not None and skip[d]:
                continue
            b1p, b2p = self.pow[d, 0] * B1, self.pow[d, 1] * B2
            lr_t = float(np.float32(LR)) * np.sqrt(1.0 - b2p) / (1.0 - b1p)
            lr_t = np.float32(lr_t) if f is np.float32 else lr_t
            for l in range(len(self.lp) - 1):
                if not self.trainable[l]:
                    continue
                s = slice(self.lp[l], self.lp[l + 1])
                gl = g[d, s].astype(f)
                if self.rule == "sgd":
                    w[d, s] = w[d, s] - lr * gl
                elif self.rule == "momentum":
                    self.m[d, s] = mom * self.m[d, s] - lr * gl
                    w[d, s] = w[d, s] + self.m[d, s]
                else:
                    if self.clip:
                        norm = np.sqrt(np.sum(g[d, s].astype(np.float64) ** 2))
                        scale = self.clip / max(norm, self.clip)
                        self.scales.append(scale)
                        gl = gl * (np.float32(scale) if f is np.float32 else scale)
                    self.m[d, s] = self.m[d, s] + (gl - self.m[d, s]) * omb1
                    self.v[d, s] = self.v[d, s] + (gl * gl - self.v[d, s]) * omb2
                    w[d, s] = w[d, s] - lr_t * self.m[d, s] / (np.sqrt(self.v[d, s]) + eps)
            self.t[d] += 1
            self.pow[d] = (b1p, b2p)
        return w


def _spread_and_allowance(lp, pairs):
    """Largest normwise difference per (device, layer) between the fp32 and the float64
    restatement over ``pairs`` of arrays, and the allowance that follows from it."""
    worst = 0.0
    for a32, a64 in pairs:
        for d in range(a64.shape[0]):
            for l in range(len(lp) - 1):
                r = a64[d, lp[l]:lp[l + 1]]
                scale = np.max(np.abs(r))
                if scale > 0:
                    worst = max(worst, float(np.max(np.abs(a32[d, lp[l]:lp[l + 1]].astype(np.float64) - r)) / scale))
    return worst, (1e-5 if worst < 1e-5 else 10 * worst)


def _assert_close(name, got, ref, lp, tol):
    worst = 0.0
    for d in range(ref.shape[0]):
        for l in range(len(lp) - 1):
            y, r = got[d, lp[l]:lp[l + 1]], ref[d, lp[l]:lp[l + 1]]
            scale = np.max(np.abs(r))
            if scale > 0:
                worst = max(worst, float(np.max(np.abs(y.astype(np.float64) - r)) / scale))
            assert normwise_close(y, r, tol), (name, d, l)
    print(f"{name}: largest normwise error per (device, layer) {worst:.3e} (allowance {tol:.1e})")
    return worst


# ---- inputs ------------------------------------------------------------------------------------
LAYOUTS = ["contiguous", "pitch_P_plus_4", "aligned_rows"]


def _stack(a, layout):
    """``a`` [D, P] on the device: contiguous (odd P: rows 1 and 2 are not 16-byte aligned, the
    element path, row 0 the vector path), with a row pitch of P + 4, or with a pitch rounded up
    to 16 bytes (every row on the vector path, odd P: a scalar tail)."""
    P = a.shape[1]
    pitch = {"contiguous": P, "pitch_P_plus_4": P + 4, "aligned_rows": (P + 3) // 4 * 4 + 4}[layout]
    buf = torch.full((a.shape[0], pitch), float("nan"), dtype=torch.float32, device="cuda")
    view = buf[:, :P]
    view.copy_(torch.from_numpy(a))
    return view


def _inputs(seed, steps, kind="normal", pad=0):
    """w [D, P] and steps gradients [steps, D, P]. ``below``: every layer's norm at most 0.5;
    ``mixed``: layers 3, 4 and 6 far above 1, layers 0, 1 and 5 far below, layer 2 all zero."""
    lp = _table(pad)
    P = int(lp[-1])
    rng = np.random.default_rng(seed)
    w = rng.standard_normal((D, P)).astype(np.float32)
    if kind == "below":
        g = rng.uniform(-1, 1, (steps, D, P))
        for l in range(len(lp) - 1):
            g[..., lp[l]:lp[l + 1]] *= 0.5 / np.sqrt(lp[l + 1] - lp[l])
    else:
        g = rng.standard_normal((steps, D, P))
        if kind == "mixed":
            for l, s in enumerate([0.1, 0.1, 0.0, 5.0, 1.0, 1e-3, 1.0]):
                g[..., lp[l]:lp[l + 1]] *= s
    return lp, w, g.astype(np.float32)


def _opt(gpu, rule, lp, Dn=D, **kw):
    from federated_amd.local_optim import PopulationOptimizer
    return PopulationOptimizer(gpu, Dn, lp, rule, LR, momentum=MOM, beta_1=B1, beta_2=B2, epsilon=EPS, **kw)


def _run(gpu, rule, lp, w, g, layout="contiguous", **kw):
    opt = _opt(gpu, rule, lp, **kw)
    models = _stack(w, layout)
    grads = [_stack(g[s], layout) for s in range(g.shape[0])]
    for gs in grads:
        opt.step(models, gs)
    torch.cuda.synchronize()
    assert torch.isnan(models._base[:, w.shape[1]:]).all()  # the columns past P are never touched
    return opt, models.cpu().numpy()


def _state(opt):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in opt.state_dict().items()}


# ---- SGD and momentum: bit for bit ---------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("rule", ["sgd", "momentum"])
def test_sgd_and_momentum_are_bit_identical_to_fp32_numpy(gpu, rule, layout):
    lp, w, g = _inputs(11, 4)
    assert int(lp[-1]) % 4 == 3  # P is no multiple of 4: scalar tail, odd inner boundaries
    opt, got = _run(gpu, rule, lp, w, g, layout)
    ref = Ref(rule, lp, D, np.float32)
    want = w.copy()
    for s in range(4):
        ref.step(want, g[s])
    assert _same(got, want)
    if rule == "momentum":
        assert _same(opt.m.cpu().numpy(), ref.m)
    assert opt.steps_done.tolist() == [4] * D


# ---- Adam ----------------------------------------------------------------------------------------
def _adam_refs(lp, w, g, clip, trainable=None):
    refs = {}
    for f in (np.float32, np.float64):
        r = Ref("adam", lp, w.shape[0], f, clip, trainable)
        x = w.astype(f)
        for s in range(g.shape[0]):
            r.step(x, g[s])
        refs[f] = (x, r)
    (w32, r32), (w64, r64) = refs[np.float32], refs[np.float64]
    spread, tol = _spread_and_allowance(lp, [(w32, w64), (r32.m, r64.m), (r32.v, r64.v)])
    print(f"fp32 against float64 restatement: spread {spread:.3e}, allowance {tol:.1e}")
    return w64, r64, tol


@pytest.mark.parametrize("layout", LAYOUTS)
def test_adam_without_clip_and_below_the_norm(gpu, layout):
    """No clip, and clipnorm = 1.0 with every layer's norm at most 0.5: the factor is exactly 1,
    so the two runs agree bit for bit; each is within the allowance of the float64 restatement
    after 5 steps."""
    lp, w, g = _inputs(12, 5, "below")
    w64, r64, tol = _adam_refs(lp, w, g, 1.0)
    assert r64.scales and all(s == 1.0 for s in r64.scales)
    off, got_off = _run(gpu, "adam", lp, w, g, layout)
    on, got_on = _run(gpu, "adam", lp, w, g, layout, clipnorm=1.0)
    so, sn = _state(off), _state(on)
    assert _same(got_off, got_on) and all(_same(so[k], sn[k]) for k in ("m", "v", "t", "pow"))
    _assert_close("w", got_on, w64, lp, tol)
    _assert_close("m", sn["m"], r64.m, lp, tol)
    _assert_close("v", sn["v"], r64.v, lp, tol)
    assert _same(sn["pow"], r64.pow) and sn["t"].tolist() == [5] * D


@pytest.mark.parametrize("layout", LAYOUTS)
def test_adam_with_the_clip_on(gpu, layout):
    """Per device at least two layers above the norm and two below (checked on the restatement's
    factors), one all-zero layer; 5 steps against the float64 restatement, everything finite."""
    lp, w, g = _inputs(13, 5, "mixed")
    n = len(lp) - 1
    w64, r64, tol = _adam_refs(lp, w, g, 1.0)
    scales = np.array(r64.scales).reshape(D, n)
    assert np.all((scales < 1.0).sum(axis=1) >= 2) and np.all((scales == 1.0).sum(axis=1) >= 3)
    assert not g[:, :, lp[2]:lp[3]].any()
    opt, got = _run(gpu, "adam", lp, w, g, layout, clipnorm=1.0)
    st = _state(opt)
    for a in (got, st["m"], st["v"], st["pow"]):
        assert np.isfinite(a).all()
    worst = max(_assert_close("w", got, w64, lp, tol), _assert_close("m", st["m"], r64.m, lp, tol),
                _assert_close("v", st["v"], r64.v, lp, tol))
    print(f"Adam with the clip, {layout}: kernel's largest error {worst:.3e}")
    # the all-zero layer: no state, the weights as they were, bit for bit
    z = slice(lp[2], lp[3])
    assert not st["m"][:, z].any() and not st["v"][:, z].any() and _same(got[:, z], w[:, z])


# ---- skip ----------------------------------------------------------------------------------------
def test_skip_leaves_a_device_untouched_and_its_counter_behind(gpu):
    lp, w, g = _inputs(14, 2, "mixed")
    skip = torch.tensor([0, 1, 0], dtype=torch.int32, device="cuda")
    opt, models = _opt(gpu, "adam", lp, clipnorm=1.0), _stack(w, "contiguous")
    # a first state that is not all zero on device 1 would hide nothing either way; start from a step
    pre = _opt(gpu, "adam", lp, clipnorm=1.0)
    grads = [_stack(g[s], "contiguous") for s in range(2)]
    before = _state(opt)
    opt.step(models, grads[0], skip)
    after, got = _state(opt), models.cpu().numpy()
    assert _same(got[1], w[1])
    for k in ("m", "v", "t", "pow"):
        assert _same(after[k][1], before[k][1]), k
    assert after["t"].tolist() == [1, 0, 1] and after["pow"][1].tolist() == [1.0, 1.0]
    # the others as in a run without skip
    models2 = _stack(w, "contiguous")
    pre.step(models2, grads[0])
    full, st2 = models2.cpu().numpy(), _state(pre)
    for d in (0, 2):
        assert _same(got[d], full[d]) and all(_same(after[k][d], st2[k][d]) for k in ("m", "v", "t", "pow"))
    # flag cleared: device 1 takes its first step (t = 1) while the others take their second
    skip.zero_()
    opt.step(models, grads[1], skip)
    assert opt.steps_done.tolist() == [2, 1, 2]
    ref, want = Ref("adam", lp, D, np.float64, 1.0), w.astype(np.float64)
    ref.step(want, g[0], [0, 1, 0])
    ref.step(want, g[1])
    assert ref.t.tolist() == [2, 1, 2]
    st = _state(opt)
    _assert_close("w", models.cpu().numpy(), want, lp, 1e-5)
    _assert_close("m", st["m"], ref.m, lp, 1e-5)
    _assert_close("v", st["v"], ref.v, lp, 1e-5)
    assert _same(st["pow"], ref.pow)
    # device 1's bias correction is that of t = 1: its row differs from a run that had stepped it twice
    pre.step(models2, grads[1])
    assert not _same(models.cpu().numpy()[1], models2.cpu().numpy()[1])


# ---- trainable -----------------------------------------------------------------------------------
@pytest.mark.parametrize("rule,kw", [("adam", dict(clipnorm=1.0)), ("momentum", {})])
def test_frozen_layers_are_untouched_and_their_nan_gradients_do_not_leak(gpu, rule, kw):
    lp, w, g = _inputs(15, 2, "mixed")
    frozen = [1, 4]  # a layer shorter than a vector, and one that spans tiles from an odd boundary
    trainable = [0 if l in frozen else 1 for l in range(len(lp) - 1)]
    for l in frozen:
        g[:, :, lp[l]:lp[l + 1]] = np.nan
    opt, got = _run(gpu, rule, lp, w, g, trainable=trainable, **kw)
    st = _state(opt)
    for l in frozen:
        s = slice(lp[l], lp[l + 1])
        assert _same(got[:, s], w[:, s]) and not st["m"][:, s].any()
        assert st["v"] is None or not st["v"][:, s].any()
    assert np.isfinite(got).all() and np.isfinite(st["m"]).all()
    ref = Ref(rule, lp, D, np.float64, kw.get("clipnorm"), trainable)
    want = w.astype(np.float64)
    for s in range(2):
        ref.step(want, np.nan_to_num(g[s]))
    _assert_close("w", got, want, lp, 1e-5)
    _assert_close("m", st["m"], ref.m, lp, 1e-5)


# ---- determinism, capture, checkpointing ----------------------------------------------------------
def test_the_same_step_twice_gives_the_same_bits(gpu):
    lp, w, g = _inputs(16, 2, "mixed")
    opt, models, grads = _opt(gpu, "adam", lp, clipnorm=1.0), _stack(w, "contiguous"), _stack(g[1], "contiguous")
    opt.step(models, _stack(g[0], "contiguous"))
    saved, w1 = opt.state_dict(), models.clone()
    opt.step(models, grads)
    first, st1 = models.cpu().numpy(), _state(opt)
    opt.load_state_dict(saved)
    models.copy_(w1)
    opt.step(models, grads)
    st2 = _state(opt)
    assert _same(models.cpu().numpy(), first) and all(_same(st1[k], st2[k]) for k in st1)


def test_six_captured_steps_equal_six_eager_steps(gpu):
    """Strict ("global") capture: the launch path reads nothing back, allocates and reconfigures
    nothing. Counters and running powers included."""
    lp, w, g = _inputs(17, 6, "mixed")
    eager, want = _run(gpu, "adam", lp, w, g, clipnorm=1.0)  # also loads the kernels ahead of the capture
    opt, models = _opt(gpu, "adam", lp, clipnorm=1.0), _stack(w, "contiguous")
    grads = [_stack(g[s], "contiguous") for s in range(6)]
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    gc.collect()
    gc.disable()
    try:
        with torch.cuda.graph(graph, stream=side, capture_error_mode="global"):
            for gs in grads:
                opt.step(models, gs)
    finally:
        gc.enable()
    assert opt.steps_done.tolist() == [0] * D  # capturing launched nothing
    graph.replay()
    torch.cuda.synchronize()
    se, sg = _state(eager), _state(opt)
    assert _same(models.cpu().numpy(), want) and all(_same(se[k], sg[k]) for k in se)
    assert sg["t"].tolist() == [6] * D


@pytest.mark.parametrize("rule,kw", [("adam", dict(clipnorm=1.0)), ("momentum", {})])
def test_checkpoint_and_resume_equal_an_uninterrupted_run(gpu, rule, kw):
    lp, w, g = _inputs(18, 4, "mixed")
    whole, want = _run(gpu, rule, lp, w, g, **kw)
    first, mid = _run(gpu, rule, lp, w, g[:2], **kw)
    resumed = _opt(gpu, rule, lp, **kw)
    resumed.load_state_dict(first.state_dict())
    models = _stack(mid, "contiguous")
    for s in (2, 3):
        resumed.step(models, _stack(g[s], "contiguous"))
    sw, sr = _state(whole), _state(resumed)
    assert _same(models.cpu().numpy(), want)
    assert all((sw[k] is None and sr[k] is None) or _same(sw[k], sr[k]) for k in sw)
    resumed.reset()
    sz = _state(resumed)
    assert not sz["m"].any() and sz["t"].tolist() == [0] * D and (sz["pow"] is None or (sz["pow"] == 1.0).all())


# ---- with the populations ---------------------------------------------------------------------------
def _ring(n):
    return [[(d - 1) % n, (d + 1) % n] for d in range(n)]


def _population_inputs(seed):
    lp = _table(pad=1)  # the population kernels want 16-byte rows: the last layer padded, inner boundaries kept
    P, Dn = int(lp[-1]), 4
    rng = np.random.default_rng(seed)
    w = rng.standard_normal((Dn, P)).astype(np.float32)
    g = rng.standard_normal((3, Dn, P)).astype(np.float32)
    for l, s in enumerate([0.1, 0.1, 0.0, 5.0, 1.0, 1e-3, 1.0]):
        g[..., lp[l]:lp[l + 1]] *= s
    return lp, w, g


def test_adam_steps_between_population_rounds_with_propagated_training_end(gpu):
    """Three iterations of "Adam step, then one round" on a 4-device ring, "copy" rule with
    propagation, device 0 ended at the start: against the same loop with the float64
    restatement in place of the kernel. Devices 1 and 3 stop after their first step, device 2
    after its second."""
    from federated_amd import topology as T
    lp, w, g = _population_inputs(19)

    def population():
        pr = T.PopulationRound(gpu, torch.from_numpy(w.copy()).cuda())
        pr.set_ended_rule("copy", propagate=True)
        pr.set_topology(_ring(4), T.alphas_tf2, use_window=False)
        pr.set_ended([0])
        return pr

    pop, opt = population(), _opt(gpu, "adam", lp, Dn=4, clipnorm=1.0)
    twin, ref = population(), Ref("adam", lp, 4, np.float64, 1.0)
    done = []
    for it in range(3):
        opt.step(pop.models, torch.from_numpy(g[it]).cuda(), pop.ended)
        pop.rounds(1)
        done.append(opt.steps_done.tolist())
        x = twin.models.cpu().numpy().astype(np.float64)
        ref.step(x, g[it], twin.ended.cpu().numpy())
        twin.models.copy_(torch.from_numpy(x.astype(np.float32)))
        twin.rounds(1)
        # after the first round device 2 holds its own stepped model mixed with two copies of device 0's
        _assert_close(f"models after iteration {it + 1}", pop.models.cpu().numpy(),
                      twin.models.cpu().numpy().astype(np.float64), lp, 1e-5)
    assert done == [[0, 1, 1, 1], [0, 1, 2, 1], [0, 1, 2, 1]]
    assert ref.t.tolist() == done[-1] and pop.ended.cpu().tolist() == [1, 1, 1, 1]


def test_adam_steps_between_fedavg_rounds(gpu):
    """The same loop on a FedAvgPopulation with the copy client; device 1 ended from the start
    takes no step, its flag does not spread."""
    from federated_amd.fedavg_population import FedAvgPopulation
    lp, w, g = _population_inputs(20)
    p0 = np.random.default_rng(21).standard_normal(w.shape[1]).astype(np.float32)

    def population():
        pop = FedAvgPopulation(gpu, torch.from_numpy(w.copy()).cuda(), torch.from_numpy(p0.copy()).cuda(), 0.5)
        pop.set_schedule([[0, 2, 3], [3, 2, 1, 0]], client="copy")
        pop.set_ended([1])
        return pop

    pop, opt = population(), _opt(gpu, "adam", lp, Dn=4, clipnorm=1.0)
    twin, ref = population(), Ref("adam", lp, 4, np.float64, 1.0)
    for it in range(3):
        opt.step(pop.models, torch.from_numpy(g[it]).cuda(), pop.ended)
        pop.rounds(1)
        x = twin.models.cpu().numpy().astype(np.float64)
        ref.step(x, g[it], twin.ended.cpu().numpy())
        twin.models.copy_(torch.from_numpy(x.astype(np.float32)))
        twin.rounds(1)
    assert opt.steps_done.tolist() == [3, 0, 3, 3] == ref.t.tolist()
    _assert_close("models", pop.models.cpu().numpy(), twin.models.cpu().numpy().astype(np.float64), lp, 1e-5)
    _assert_close("params", pop.params.cpu().numpy()[None], twin.params.cpu().numpy().astype(np.float64)[None], lp, 1e-5)
