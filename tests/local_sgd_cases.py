"""The cases of tests/test_gpu_local_sgd_paths.py and tests/test_local_sgd_cases_host.py: the paths
of the local-SGD epoch kernels (csrc/cfa_local_sgd.hip) that the four shapes of
test_gpu_local_training.py never take. A plain helper module: the case table, the data builders,
the float64 reference and the guards, without a GPU, so that the host test checks on the CPU what
the GPU test relies on.

Reference and tolerance are those of test_gpu_local_training.py (its ref_epoch, _layout and
_split4 are imported, not restated): the float64 epoch, ``max(1e-5, 4 * s)`` per (device, tensor)
with ``s`` the fp32-vs-fp64 spread of the restated epoch, ``s < 1e-4``, the cost within 1e-5.

The launch plan of the kernels is mirrored here (softmax_width, taps_in_regs, cnn_sgd_lds,
nn_sgd_lds and the constants kGradBlock 512, kPreX 8, kPreY 2, kMaxTaps 32, kSpan 32), as
test_gpu_grad_paths.py mirrors cnn_plan, and every case asserts from the mirror alone the
condition that puts it on its path (Case.path).

An fp32 kernel and a float64 reference may take different sides of a decision (relu at 0, pool
winner against runner-up, the clip bounds) where an input sits on it, and over an epoch the
inputs of step i are the outputs of step i - 1. decision_margin() therefore evaluates
_decision_margin of test_gpu_grad_paths.py at every step of the float64 trajectory and divides
the smallest margin by the largest pre-activation; every randomised case must reach 1e-4, the bar
of that file, and its seed is fixed so that the float64 reference alone satisfies it."""
import contextlib
import functools
import types

import numpy as np

from oracle import cfa_oracle as orc
from test_gpu_grad_paths import _decision_margin, _tie_case
from test_gpu_local_training import LR, S_MAX, _data, _layout, _split4, ref_epoch

# cfa_local_sgd.hip / cfa_grad_common.h: kGradBlock, kPreX, kPreY, kMaxTaps, kSpan
K_BLOCK, K_PRE_X, K_PRE_Y, K_MAX_TAPS, K_SPAN = 512, 8, 2, 32, 32
LDS_DEFAULT = 65536      # dynamic LDS of a launch before sgd_lds raises the kernel's limit
LDS_DEVICE = 160 * 1024  # the card's LDS per workgroup: what sgd_lds refuses above
MARGIN_BAR = 1e-4


def _ceil(a, b):
    return -(-a // b)


def softmax_width(C):
    w = 1
    while w < C:
        w <<= 1
    return w


def taps_in_regs(F, NC):
    return F <= K_MAX_TAPS and K_BLOCK % NC == 0


def plan(ml, geom):
    """CnnGeom / NnGeom as the entry points fill them."""
    L, C = geom["input_data"], geom["classes"]
    if ml == 1:
        F, NC, S = geom["filter"], geom["number"], geom["stride"]
        L1 = _ceil(L, S)
        L2 = _ceil(L1, S)
        return types.SimpleNamespace(
            L=L, C=C, F=F, NC=NC, S=S, L1=L1, L2=L2, LN=L2 * NC, pl=orc._tf_same_left(L, F, S),
            ql=orc._tf_same_left(L1, S, S), P=F * NC + NC + L2 * NC * C + C, SW=softmax_width(C),
            fast=(F, S) == (16, 5), taps_in_regs=taps_in_regs(F, NC))
    H = geom["intermediate_nodes"]
    return types.SimpleNamespace(L=L, C=C, H=H, G=_ceil(L, K_SPAN), P=L * H + H + H * C + C, SW=softmax_width(C))


def cnn_sgd_lds(d, nb):
    """LDS floats of local_sgd_cnn_kernel."""
    return d.P + nb * (2 * (d.L + d.C) + 3 * d.LN + d.C + d.F * d.NC + d.NC + 1)


def nn_sgd_lds(d, nb):
    """LDS floats of local_sgd_2nn_kernel."""
    return d.P + nb * (2 * (d.L + d.C) + 2 * d.H + d.C + d.G * d.H + 1)


def lds_bytes(ml, geom, nb):
    d = plan(ml, geom)
    return 4 * (cnn_sgd_lds(d, nb) if ml == 1 else nn_sgd_lds(d, nb))


def _cnn(F, S, NC, L, C):
    return {"filter": F, "number": NC, "stride": S, "input_data": L, "classes": C}


def _nn(L, H, C):
    return {"intermediate_nodes": H, "input_data": L, "classes": C}


class Case:
    """One launch: D devices with their own samples and starting models, ``steps`` minibatches of
    ``rows`` samples ``stride`` apart. ``build`` (seed, case) -> (x, y, W) replaces the random data
    of _data; ``guard`` False exempts a built case from the margin guard."""

    def __init__(self, name, ml, geom, rows, stride, steps, seed, D=2, build=None, guard=True):
        self.name, self.ml, self.geom, self.rows, self.stride, self.steps = name, ml, geom, rows, stride, steps
        self.seed, self.D, self.build, self.guard = seed, D, build, guard
        self.Ns = (steps - 1) * stride + rows
        self.plan = plan(ml, geom)
        self.shapes, self.offs = _layout(ml, geom)
        self.P = self.offs[4]
        assert self.P == self.plan.P

    @property
    def lds(self):
        return lds_bytes(self.ml, self.geom, self.rows)

    @functools.cached_property
    def data(self):
        """(x [D, Ns, L], y [D, Ns, C], W [D, P]), fp32, read-only."""
        out = self.build(self.seed, self) if self.build else _data(self.seed, self.ml, self.geom, self.D, self.Ns)
        for a in out:
            a.setflags(write=False)
        return out

    def path(self):
        """{condition: holds}: what puts the case on the path it is in the table for."""
        return PATHS[self.name](self) if self.name in PATHS else {}


def _path_A(c):
    d, nb = c.plan, c.rows
    return {"x store tail": nb * d.L == 4250 > K_PRE_X * K_BLOCK == 4096,
            "y store tail": nb * d.C == 1088 > K_PRE_Y * K_BLOCK == 1024,
            "softmax second trip": nb * d.SW == 1088 > K_BLOCK and d.SW == 64,
            "default LDS": c.lds <= LDS_DEFAULT}


def _path_B(c):
    d = c.plan
    return {"fast kernel": d.fast, "runtime loop inside <16,5>": K_BLOCK % d.NC != 0 and not d.taps_in_regs,
            "SW 16": d.SW == 16 and d.C == 10}


def _path_C(c):
    d = c.plan
    return {"fast kernel": d.fast, "register taps": d.taps_in_regs, "L < F": d.L < d.F, "L2 = 1": d.L2 == 1,
            "windows of padding": d.L1 == 2 and d.pl == 7}


def _path_D(c):
    d = c.plan
    return {"generic kernel": not d.fast, "F > kMaxTaps": d.F == 33 > K_MAX_TAPS and not d.taps_in_regs,
            "stride above rows": c.stride > c.rows}


def _path_E1(c):
    d, nb = c.plan, c.rows
    return {"fast kernel": d.fast and d.taps_in_regs, "x store tail": nb * d.L == 4608 > K_PRE_X * K_BLOCK,
            "logits second trip": nb * d.C * 8 == 576 > K_BLOCK, "default LDS": c.lds <= LDS_DEFAULT}


def _path_E3(c):
    d, nb = c.plan, c.rows
    return {"fast kernel": d.fast and d.taps_in_regs, "x store tail": nb * d.L > K_PRE_X * K_BLOCK,
            "LDS limit raised": c.lds == 4 * (1488 + 9 * 1689) == 66756 > LDS_DEFAULT and c.lds <= LDS_DEVICE}


def _path_F(c):
    d = c.plan
    return {"G = 2, last slice of 1": d.G == 2 and d.L - K_SPAN == 1, "SW 64 with dead lanes": d.SW == 64 > d.C == 33,
            "nb = 1": c.rows == 1}


def _path_G(c):
    d = c.plan
    return {"SW 64 full": d.SW == 64 == d.C, "softmax second trip": c.rows * d.SW == 576 > K_BLOCK,
            "partial slice at G = 1": d.G == 1 and d.L < K_SPAN}


def _path_H(c):
    d = c.plan
    return {"generic kernel": not d.fast, "S = 1": d.S == 1 and d.L1 == d.L2 == d.L and d.ql == 0, "pl = 1": d.pl == 1}


PATHS = {"A": _path_A, "B": _path_B, "C": _path_C, "D": _path_D, "E1": _path_E1, "E3": _path_E3, "F": _path_F,
         "G": _path_G, "H": _path_H}

# Seeds chosen on the CPU: the one with the largest margin of those that clear the bar from the
# float64 reference alone (A, E1, E3: of seeds 100 to 159; the others: of 0 to 2).
TABLE = {c.name: c for c in (
    Case("A", 2, _nn(250, 4, 64), 17, 17, 2, 156),
    Case("B", 1, _cnn(16, 5, 6, 57, 10), 3, 3, 3, 0),
    Case("C", 1, _cnn(16, 5, 8, 7, 2), 4, 4, 3, 0),
    Case("D", 1, _cnn(33, 2, 4, 40, 3), 2, 3, 3, 2),
    Case("E1", 1, _cnn(16, 5, 2, 512, 8), 9, 9, 2, 150),
    Case("E3", 1, _cnn(16, 5, 8, 512, 8), 9, 9, 1, 124),
    Case("F", 2, _nn(33, 7, 33), 1, 1, 3, 1),
    Case("G", 2, _nn(20, 6, 64), 9, 9, 2, 1),
    Case("H", 1, _cnn(3, 1, 2, 9, 4), 2, 2, 3, 1),
)}


# ------------------------------------------------------------------------------------------
# The float64 epoch, its fp32 spread and the decision margin
# ------------------------------------------------------------------------------------------

def trajectory(c, d):
    """Device d's flat float64 model before each step of the float64 epoch (ref_epoch, one step at
    a time on the minibatch's own rows: the same arithmetic as the whole epoch)."""
    x, y, W = c.data
    w, out = W[d].astype(np.float64), []
    for i in range(c.steps):
        out.append(w)
        lo = i * c.stride
        w, _ = ref_epoch(c.ml, c.geom, x[d, lo:lo + c.rows], y[d, lo:lo + c.rows], w, c.stride, c.rows, 1, LR, np.float64)
    return out


def forward(c, xb, w):
    """(logits, pred) of the float64 forward pass of a minibatch at the flat model w."""
    w4 = _split4(np.asarray(w, np.float64), c.shapes, c.offs)
    if c.ml == 1:
        logits = orc.tf1_cnn_forward(xb, *w4, stride=c.geom["stride"])[0]
    else:
        logits = np.maximum(np.asarray(xb, np.float64) @ w4[0] + w4[1], 0.0) @ w4[2] + w4[3]
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    return logits, e / e.sum(axis=1, keepdims=True)


def decision_margin(c, keep=None):
    """Smallest decision margin over every device and step of the float64 trajectory, divided by
    the largest pre-activation met on the way. ``keep`` [D, Ns] bool: the samples that count (a
    built case leaves out the samples whose gradient the clip blocks whatever they decide)."""
    x, y, _ = c.data
    margin, scale = np.inf, 0.0
    for d in range(c.D):
        for i, w in enumerate(trajectory(c, d)):
            rows = np.arange(i * c.stride, i * c.stride + c.rows)
            if keep is not None:
                rows = rows[keep[d, rows]]
            if rows.size == 0:
                continue
            m, s = _decision_margin(c.ml, x[d, rows], y[d, rows], _split4(w, c.shapes, c.offs), c.geom.get("stride"))
            margin, scale = min(margin, m), max(scale, s)
    return margin / scale


@functools.lru_cache(maxsize=None)
def reference(c, update=True):
    """The restated epochs of a case, computed once and shared, as reference() of
    test_gpu_local_training.py: the float64 models and costs per device, the spread ``s`` and the
    allowance ``max(1e-5, 4 * s)`` per (device, tensor)."""
    x, y, W = c.data
    w64, c64, allow, spread = [], [], [], []
    for d in range(c.D):
        a, ca = ref_epoch(c.ml, c.geom, x[d], y[d], W[d], c.stride, c.rows, c.steps, LR, np.float64, update)
        b, _ = ref_epoch(c.ml, c.geom, x[d], y[d], W[d], c.stride, c.rows, c.steps, LR, np.float32, update)
        s = [float(np.max(np.abs(b[c.offs[k]:c.offs[k + 1]] - a[c.offs[k]:c.offs[k + 1]]))
                   / np.max(np.abs(a[c.offs[k]:c.offs[k + 1]]))) for k in range(4)]
        w64.append(a), c64.append(ca), spread.append(s)
        allow.append([max(1e-5, 4 * v) for v in s])
    out = dict(w64=np.stack(w64), c64=np.array(c64), allow=allow, spread=spread, s=max(max(s) for s in spread))
    out["w64"].setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------
# Built cases
# ------------------------------------------------------------------------------------------

CLIP_GEOM = {1: _cnn(16, 5, 8, 40, 4), 2: _nn(40, 8, 4)}  # _class_dims of test_gpu_grad_paths.py at C = 4


def _build_clip_above(seed, c):
    """As test_clip_blocks_predictions_above_its_bound: a small W2 and b2 = (6.5, 0, 0, 0) put
    pred_0 near e^6.5 / (e^6.5 + 3) = 0.9955 for every sample; the samples labelled 0 sit above the
    bound (gradient blocked), the others, with pred near 0.0015, below it."""
    x, y, W = _data(seed, c.ml, c.geom, c.D, c.Ns)
    W[:, c.offs[2]:c.offs[3]] *= np.float32(0.1)
    W[:, c.offs[3]:c.offs[4]] = [6.5, 0, 0, 0]
    labels = np.tile([0, 1, 0, 2, 0, 3, 0, 1], c.Ns // 8)
    y = np.broadcast_to(np.eye(4, dtype=np.float32)[labels], y.shape).copy()
    return x, y, W


def clip_above(ml):
    return Case(f"clip above ml={ml}", ml, CLIP_GEOM[ml], 8, 8, 2, {1: 2, 2: 2}[ml], build=_build_clip_above)


def clip_sides(c):
    """Per (device, step): the labelled predictions of the float64 forward pass, [rows]."""
    x, y, _ = c.data
    out = []
    for d in range(c.D):
        for i, w in enumerate(trajectory(c, d)):
            lo = i * c.stride
            pred = forward(c, x[d, lo:lo + c.rows], w)[1]
            out.append(pred[y[d, lo:lo + c.rows] != 0])
    return out


@contextlib.contextmanager
def clip_gate_open_above():
    """The oracle with the upper half of the clip's gate removed (the gradient passes wherever
    pred >= 1e-15, the cost unchanged): what a kernel without ``p <= kClipHi`` computes."""
    def ungated(logits, y):
        z = logits - logits.max(axis=1, keepdims=True)
        pred = np.exp(z) / np.exp(z).sum(axis=1, keepdims=True)
        clipped = np.clip(pred, 1e-15, 0.99)
        dpred = np.where(pred >= 1e-15, -(y / clipped) / logits.shape[0], 0.0)
        return kept(logits, y)[0], (dpred - np.sum(dpred * pred, axis=1, keepdims=True)) * pred
    kept = orc._softmax_xent_grad
    orc._softmax_xent_grad = ungated
    try:
        yield
    finally:
        orc._softmax_xent_grad = kept


def gate_effect(c):
    """Per tensor, the largest normwise distance over the devices between the float64 epoch and
    the one with the gate open above the bound."""
    x, y, W = c.data
    ref = reference(c)["w64"]
    with clip_gate_open_above():
        open_ = [ref_epoch(c.ml, c.geom, x[d], y[d], W[d], c.stride, c.rows, c.steps, LR, np.float64)[0]
                 for d in range(c.D)]
    return [max(float(np.max(np.abs(open_[d][c.offs[k]:c.offs[k + 1]] - ref[d][c.offs[k]:c.offs[k + 1]]))
                      / np.max(np.abs(ref[d][c.offs[k]:c.offs[k + 1]]))) for d in range(c.D)) for k in range(4)]


BELOW_ROWS = (1, 4)  # of the 6 rows of the minibatch: pred of the labelled class below 1e-16


def _build_clip_below(seed, c):
    """Ordinary samples, and two per device scaled up until the labelled class (the one with the
    smallest logit) sits at least 45 below the largest: pred < e^-45 = 3e-20, the gradient is
    blocked and the sample costs -log(1e-15)."""
    x, y, W = _data(seed, c.ml, c.geom, c.D, c.Ns)
    for d in range(c.D):
        for r in BELOW_ROWS:
            logits = forward(c, x[d, r:r + 1], W[d])[0][0]
            while logits.max() - logits.min() < 45.0:
                x[d, r] *= np.float32(2.0)
                logits = forward(c, x[d, r:r + 1], W[d])[0][0]
            y[d, r] = np.eye(c.geom["classes"], dtype=np.float32)[np.argmin(logits)]
    return x, y, W


def clip_below(ml):
    return Case(f"clip below ml={ml}", ml, CLIP_GEOM[ml], 6, 6, 1, {1: 1, 2: 1}[ml], build=_build_clip_below)


def clip_below_keep(c):
    keep = np.ones((c.D, c.Ns), bool)
    keep[:, list(BELOW_ROWS)] = False
    return keep


def _build_one_class(seed, c):
    x, _, W = _data(seed, c.ml, c.geom, c.D, c.Ns)
    return x, np.ones((c.D, c.Ns, 1), np.float32), W


def one_class(ml):
    """C = 1: SW = 1, pred = 1 > 0.99, every gradient blocked. Two rows, so that the minibatch's
    mean cost is an exact fp32 sum."""
    geom = _cnn(4, 4, 6, 37, 1) if ml == 1 else _nn(20, 5, 1)
    return Case(f"C=1 ml={ml}", ml, geom, 2, 2, 2, 0, build=_build_one_class, guard=False)


def _build_tie(fast):
    def build(seed, c):
        t, _, _ = _tie_case(fast)
        W = np.stack([np.concatenate([a.reshape(-1) for a in m]) for m in t.models]).astype(np.float32)
        return (np.repeat(t.x, 2, axis=0).astype(np.float32), np.repeat(t.y, 2, axis=0).astype(np.float32), W)
    return build


def pooling_tie(fast):
    """_tie_case of test_gpu_grad_paths.py as one minibatch: its two models are the two devices,
    on the same small-integer samples. Model 0 is the one with the ties."""
    t, ties, zero = _tie_case(fast)
    L, S, F, NC, C = t.dims
    c = Case(f"tie fast={fast}", 1, _cnn(F, S, NC, L, C), t.B, t.B, 1, 77, build=_build_tie(fast), guard=False)
    return c, ties, zero


DEAD_GEOM = {False: _cnn(4, 4, 6, 37, 5), True: _cnn(16, 5, 8, 57, 5)}


def _build_dead(seed, c):
    x, y, W = _data(seed, c.ml, c.geom, c.D, c.Ns)
    W[0, c.offs[1]:c.offs[2]] = -100.0  # device 0: no conv output above 0
    return x, y, W


def dead_relu(fast):
    """Device 0 with conv biases of -100: every pooled value is 0. Device 1 is ordinary."""
    return Case(f"dead relu fast={fast}", 1, DEAD_GEOM[fast], 3, 3, 2, {False: 3, True: 1}[fast], build=_build_dead)


def device_keep(c, d):
    """The samples of device d alone (the dead device's pre-activations, near -100, would
    otherwise set the scale that the ordinary device's margins are divided by)."""
    keep = np.zeros((c.D, c.Ns), bool)
    keep[d] = True
    return keep


NN_TINY = _nn(20, 5, 3)
# 300 devices of the tiny 2NN, one minibatch each: 6 000 hidden units, and seed 36 is the one of 0 to 39
# with the largest margin (2.2e-4; five of the 40 clear the bar)
MANY = Case("D=300", 2, NN_TINY, 4, 4, 1, 36, D=300)

# (ml, geometry, rows per minibatch) whose launch needs more LDS than a workgroup can have
TOO_MUCH_LDS = [(1, _cnn(4, 4, 6, 37, 5), 250), (2, NN_TINY, 700)]

CLIP_ABOVE = {ml: clip_above(ml) for ml in (1, 2)}
CLIP_BELOW = {ml: clip_below(ml) for ml in (1, 2)}
ONE_CLASS = {ml: one_class(ml) for ml in (1, 2)}
TIES = {fast: pooling_tie(fast) for fast in (False, True)}  # (case, ties, zero)
DEAD = {fast: dead_relu(fast) for fast in (False, True)}


# ------------------------------------------------------------------------------------------
# What the GPU test relies on, asserted from the float64 reference alone (the host test runs these
# on the CPU; the GPU test runs them again before it launches)
# ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def margin(c):
    return decision_margin(c)


def assert_guarded(c, ratio=None):
    """The margin guard and the bound on the spread."""
    ratio = margin(c) if ratio is None else ratio
    assert ratio >= MARGIN_BAR, ("input on a decision boundary", c.name, ratio)
    assert reference(c)["s"] < S_MAX, (c.name, reference(c)["s"])


def assert_path(c):
    path = c.path()
    assert path and all(path.values()), (c.name, path)
    assert c.Ns == (c.steps - 1) * c.stride + c.rows and c.lds <= LDS_DEVICE


def assert_clip_above(c):
    """At every step of every device: labelled predictions in (0.99, 0.999) and below 0.99, none
    within 1e-3 of the bound; and the gate's effect is far above the allowance."""
    sides = clip_sides(c)
    assert len(sides) == c.D * c.steps == 4
    for pred in sides:
        above = (pred > 0.99) & (pred < 0.999)
        assert above.sum() == 4 and (pred < 0.99).sum() == 4, pred
        assert np.abs(pred - 0.99).min() >= 1e-3, pred
    assert_guarded(c)
    effect = gate_effect(c)
    assert max(effect) > 100 * max(max(a) for a in reference(c)["allow"]), effect
    return effect


def assert_clip_below(c):
    """The scaled samples' labelled prediction is below 1e-16, the others' between 1e-3 and 0.99;
    the ordinary samples pass the margin guard (the blocked ones decide nothing)."""
    x, y, W = c.data
    assert c.steps == 1
    for d in range(c.D):
        logits, pred = forward(c, x[d], W[d])
        lab = pred[y[d] != 0]
        low = np.zeros(c.rows, bool)
        low[list(BELOW_ROWS)] = True
        assert np.all(lab[low] < 1e-16) and np.all((lab[~low] > 1e-3) & (lab[~low] < 0.98)), lab
        gap = logits.max(axis=1) - logits[y[d] != 0]
        assert np.all(gap[low] >= 40.0), gap
    assert_guarded(c, decision_margin(c, clip_below_keep(c)))
    # every blocked sample costs -log(1e-15): a third of the minibatch's cost and more
    assert np.all(reference(c)["c64"] > 2 * -np.log(1e-15) / c.rows)


def assert_one_class(c):
    """C = 1: the float64 epoch leaves the model as it is and costs -log(0.99)."""
    ref = reference(c)
    assert c.plan.SW == 1 and np.array_equal(ref["w64"], c.data[2].astype(np.float64))
    assert np.all(np.abs(ref["c64"] + np.log(0.99)) <= 1e-12)


def assert_tie(c, ties, zero):
    """Model 0 (device 0): two positions of a window tie at a positive value, the oracle takes the
    first, and the two positions' inputs differ, so the winner shows in W1's step."""
    x, y, W = c.data
    S, F = c.geom["stride"], c.geom["filter"]
    w4 = _split4(W[0].astype(np.float64), c.shapes, c.offs)
    _, pooled, arg, (xpad, _, _) = orc.tf1_cnn_forward(x[0], *w4, S)
    for b, q, ch, p1, p2 in ties:
        assert p1 < p2 and arg[b, q, ch] == p1 and pooled[b, q, ch] > 0
        w1, w2 = xpad[b, p1 * S:p1 * S + F], xpad[b, p2 * S:p2 * S + F]
        k = np.flatnonzero(w4[0][:, 0, ch])[0]
        assert w1[k] == w2[k] == pooled[b, q, ch] and not np.array_equal(w1, w2)
    assert pooled[zero] == 0.0
    assert np.array_equal(x, np.round(x)) and np.abs(x).max() <= 8  # small integers: exact in fp32
    assert reference(c)["s"] < S_MAX


def assert_dead(c):
    """Device 0: every pooled value of both minibatches is 0, at both steps; its float64 epoch
    leaves W1, b1 and W2 as they are and moves b2. Device 1 is ordinary."""
    x, y, W = c.data
    for i, w in enumerate(trajectory(c, 0)):
        lo = i * c.stride
        pooled = orc.tf1_cnn_forward(x[0, lo:lo + c.rows], *_split4(w, c.shapes, c.offs), c.geom["stride"])[1]
        assert not pooled.any()
    ref = reference(c)["w64"]
    w0 = W.astype(np.float64)
    assert np.array_equal(ref[0, :c.offs[3]], w0[0, :c.offs[3]])
    assert np.all(np.abs(ref[0, c.offs[3]:] - w0[0, c.offs[3]:]) > 1e-4)
    assert all(np.any(ref[1, c.offs[k]:c.offs[k + 1]] != w0[1, c.offs[k]:c.offs[k + 1]]) for k in range(4))
    assert_guarded(c, min(decision_margin(c, device_keep(c, d)) for d in range(c.D)))
