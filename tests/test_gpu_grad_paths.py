"""(f3) The CFA-GE gradient kernels (csrc/cfa_grad.hip) on the paths the two model shapes of
test_gpu_grad.py never take: the plain entry points, the LDS chunk loop past its first iteration,
chunking inside a batch split, the <16, 5> template away from L = 512 and without register taps,
the generic CNN kernel at its geometry edges, every softmax lane width, pooling ties, the 2NN
first layer from global weights, partial input slices, the scalar and the misaligned float4 gW1
paths, and both refusals.

Reference: the oracle's float64 tf1_cnn_grads / tf1_2nn_grads; tolerance: normwise_close(., 1e-5)
per tensor, as everywhere in the suite. No shape is larger than those test_gpu_grad.py already runs
(L <= 513, H <= 48, B <= 64), so the fp32 accumulation error is within what that bound already
accepts.

Paths are forced with the library's own measurement knobs (CFA_GRAD_LDS_CAP in bytes,
CFA_GRAD_SPLIT), which it reads with getenv on every call. The LDS plan is mirrored here
(cnn_plan / nn_plan) and every test asserts, before it launches, the condition that puts it on its
path, from that mirror alone: no test depends on the LDS size the device reports (every cap is at
most 64 KiB, the least the library assumes, and every uncapped launch fits in 64 KiB).

An fp32 kernel and an fp64 reference may disagree where an input sits on a decision (relu at 0,
pool winner against runner-up, the clip at 0.99 and 1e-15). Every randomised case asserts that
its smallest margin over those decisions (_decision_margin) is at least 1e-4 of the largest
pre-activation, about 100 times the fp32 error of these dot products; seeds are fixed so that it
holds. The pooling-tie cases are exempt by construction: their conv outputs are small integers,
exact in fp32, and the ties are the point."""
import functools
import types

import numpy as np
import pytest

from conftest import normwise_close
from oracle import cfa_oracle as orc

pytestmark = pytest.mark.gpu

# cfa_grad.hip: kGradBlock, kMaxTaps, kSpan
K_BLOCK, K_MAX_TAPS, K_SPAN = 512, 32, 32
LDS_FLOOR = 65536  # device_lds_max()'s fallback: the least LDS a launch plan assumes

STD_CNN = (512, 5, 16, 8, 8)  # (L, S, F, NC, C): federated_sample_CNN_CFA-GE.py:36-39
STD_2NN = (512, 32, 8)        # (L, H, C)


@pytest.fixture(autouse=True)
def _knobs_unset(monkeypatch):
    monkeypatch.delenv("CFA_GRAD_LDS_CAP", raising=False)
    monkeypatch.delenv("CFA_GRAD_SPLIT", raising=False)


def _ceil(a, b):
    return -(-a // b)


def cnn_plan(L, S, F, NC, C):
    """CnnDims as launch_grad_cnn fills it, with cnn_lds_fixed / cnn_lds_per_sample (floats)."""
    L1 = _ceil(L, S)
    L2 = _ceil(L1, S)
    LN = L2 * NC
    return types.SimpleNamespace(
        L1=L1, L2=L2, LN=LN, pl=orc._tf_same_left(L, F, S), ql=orc._tf_same_left(L1, S, S),
        P=F * NC + NC + LN * C + C, fixed=F * NC + NC + LN * C + C,
        per=L + 3 * LN + 2 * C + F * NC + NC,
        taps_in_regs=F <= K_MAX_TAPS and K_BLOCK % NC == 0, fast=(F, S) == (16, 5))


def nn_plan(L, H, C):
    """NnDims as launch_grad_2nn fills it, with nn_lds_fixed / nn_lds_per_sample (floats)."""
    G = _ceil(L, K_SPAN)
    return types.SimpleNamespace(G=G, P=L * H + H + H * C + C, fixed=H + H * C + C,
                                 per=L + 2 * H + 2 * C + G * H, w_in_regs=G * H <= K_BLOCK)


def _plan(ml, dims):
    return cnn_plan(*dims) if ml == 1 else nn_plan(*dims)


def lds_cap(plan, Bc):
    """A CFA_GRAD_LDS_CAP (bytes) under which plan_chunk fits exactly Bc samples."""
    cap = 4 * (plan.fixed + plan.per * Bc)
    assert cap <= LDS_FLOOR  # below anything the device can report, so the cap alone decides
    return cap


def planned_bc(plan, Bs, cap=LDS_FLOOR):
    """plan_chunk's samples per chunk for a workgroup of Bs samples (0: refused)."""
    return max(0, min(Bs, (cap // 4 - plan.fixed) // plan.per))


def nn_dz_aligned(dims, Bc):
    """Whether dz sits on a 16-byte boundary of the 2NN kernel's LDS (b1 W2 b2 xs act dz ...)."""
    L, H, C = dims
    return (H + H * C + C + Bc * L + Bc * H) % 4 == 0


# ------------------------------------------------------------------------------------------
# Cases: inputs, the float64 reference (computed once per evaluation and shared), the margin guard
# ------------------------------------------------------------------------------------------

def _softmax(logits):
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def _decision_margin(ml, x, y, model, stride=None):
    """(smallest margin, largest |pre-activation|) over the decisions of one evaluation, from the
    oracle's float64 forward pass: each pool winner's pre-activation (2NN: every hidden unit's)
    against 0, the top-two gap of each pooling window whose winner is positive, and
    |pred - 0.99|, |pred - 1e-15| for the classes with a non-zero label."""
    W1, b1, W2, b2 = [np.asarray(a, np.float64) for a in model]
    margins = []
    if ml == 1:
        S = int(stride)
        logits, _, _, (xpad, _, L1) = orc.tf1_cnn_forward(x, W1, b1, W2, b2, S)
        F = W1.shape[0]
        idx = np.arange(L1)[:, None] * S + np.arange(F)[None, :]
        pre = np.einsum("blf,fc->blc", xpad[:, idx], W1[:, 0, :]) + b1.reshape(-1)  # [B, L1, NC]
        L2, ql = _ceil(L1, S), orc._tf_same_left(L1, S, S)
        for q in range(L2):
            ps = [p for p in range(q * S - ql, q * S - ql + S) if 0 <= p < L1]
            top = -np.sort(-pre[:, ps, :], axis=1)
            margins.append(np.abs(top[:, 0, :]).min())
            if len(ps) > 1:
                h = np.maximum(top[:, :2, :], 0.0)
                gap = np.where(h[:, 0, :] > 0, h[:, 0, :] - h[:, 1, :], np.inf)
                margins.append(gap.min())
    else:
        pre = np.asarray(x, np.float64) @ W1 + b1.reshape(-1)
        margins.append(np.abs(pre).min())
        logits = np.maximum(pre, 0.0) @ W2 + b2.reshape(-1)
    pred = _softmax(logits)[np.asarray(y) != 0]
    margins += [np.abs(pred - 0.99).min(), np.abs(pred - 1e-15).min()]
    return float(min(margins)), float(np.abs(pre).max())


class Case:
    """Dx data sets of B samples, M models, and the evaluations (model_row[m], data_row[m])."""

    def __init__(self, ml, dims, B, M, Dx, seed, guard=True):
        rng = np.random.default_rng(seed)
        self.ml, self.dims, self.B, self.M, self.Dx, self.guard = ml, dims, B, M, Dx, guard
        self.plan = _plan(ml, dims)
        if ml == 1:
            L, S, F, NC, C = dims
            self.shapes = [(F, 1, NC), (NC,), (self.plan.LN, C), (C,)]
            scales = (0.3, 0.1, 0.1, 0.1)
            self.geom = {"filter": F, "number": NC, "stride": S}
        else:
            L, H, C = dims
            self.shapes = [(L, H), (H,), (H, C), (C,)]
            scales = (0.1, 0.1, 0.3, 0.1)
            self.geom = {"intermediate_nodes": H}
        self.L, self.C = L, C
        self.models = [[(rng.standard_normal(s) * k).astype(np.float32) for s, k in zip(self.shapes, scales)]
                       for _ in range(M)]
        self.x = rng.standard_normal((Dx, B, L)).astype(np.float32)
        self.y = np.eye(C, dtype=np.float32)[rng.integers(0, C, (Dx, B))]
        # scattered rows: every model used once, out of order; the data rows alternate from the last
        self.mrow = np.arange(M - 1, -1, -1, dtype=np.int32)
        self.drow = ((np.arange(M) + Dx - 1) % Dx).astype(np.int32)
        self.offs = np.concatenate([[0], np.cumsum([int(np.prod(s)) for s in self.shapes])])
        self.P = int(self.offs[-1])
        assert self.P == self.plan.P
        self._refs = {}

    @property
    def flat(self):
        return np.stack([np.concatenate([a.reshape(-1) for a in m]) for m in self.models])

    def ref(self, mi, di):
        """The oracle's four gradients of data set di at model mi (computed once, then shared)."""
        key = (int(mi), int(di))
        if key not in self._refs:
            x, y, m = self.x[di], self.y[di], self.models[mi]
            if self.guard:
                margin, scale = _decision_margin(self.ml, x, y, m, self.dims[1])
                assert margin >= 1e-4 * scale, ("input on a decision boundary", key, margin, scale)
            if self.ml == 1:
                g, _ = orc.tf1_cnn_grads(x, y, *m, stride=self.dims[1])
            else:
                g, _ = orc.tf1_2nn_grads(x, y, *m)
            for a in g:
                a.setflags(write=False)
            self._refs[key] = g
        return self._refs[key]


# Seeds chosen on the CPU so that every evaluation of the case passes the margin guard with a
# factor 2 to spare (the first such seed counting from 0); a case not listed takes seed 0. The
# standard shapes need a long search: of their thousands of windows or hidden units per case some
# pair is nearly always closer than the guard allows, and a random label often has pred < 1e-3.
# Key: (ml, dims, B, M, Dx).
SEEDS = {
    (1, STD_CNN, 6, 3, 1): 351, (1, STD_CNN, 7, 3, 2): 335, (1, STD_CNN, 9, 3, 2): 395, (1, STD_CNN, 6, 3, 3): 91,
    (2, STD_2NN, 6, 3, 1): 144, (2, STD_2NN, 7, 3, 2): 124, (2, STD_2NN, 9, 3, 2): 1, (2, STD_2NN, 6, 3, 3): 1800,
    (1, (513, 5, 16, 8, 8), 4, 3, 2): 1, (1, (127, 5, 16, 6, 8), 4, 3, 2): 2, (1, (513, 5, 16, 16, 8), 4, 3, 2): 5355,
    (1, (50, 3, 40, 4, 33), 5, 3, 2): 2, (2, (512, 48, 8), 5, 3, 2): 102,
}


@functools.lru_cache(maxsize=None)
def case(ml, dims, B, M, Dx=2):
    return Case(ml, dims, B, M, Dx, SEEDS.get((ml, dims, B, M, Dx), 0))


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_rows(gpu, c, split=False, mrow=None, drow=None):
    """grad_rows over the case's evaluations into a NaN-filled output; split: with a workspace."""
    import torch
    mrow = c.mrow if mrow is None else np.asarray(mrow, np.int32)
    drow = c.drow if drow is None else np.asarray(drow, np.int32)
    M = len(mrow)
    g = torch.full((M, c.P), float("nan"), device="cuda")
    ws = gpu.grad_workspace(M, c.B, c.P) if split else None
    gpu.grad_rows(c.ml, _t(c.x), _t(c.y), _t(c.flat), _t(mrow), _t(drow), g, c.geom, workspace=ws)
    torch.cuda.synchronize()
    return g.cpu().numpy()


def run_plain(gpu, c, di=0):
    """Engine.grad_cnn / grad_2nn: every model of the case on data set di."""
    import torch
    g = torch.full((c.M, c.P), float("nan"), device="cuda")
    if c.ml == 1:
        L, S, F, NC, C = c.dims
        gpu.grad_cnn(_t(c.x[di]), _t(c.y[di]), _t(c.flat), g, F, NC, S)
    else:
        gpu.grad_2nn(_t(c.x[di]), _t(c.y[di]), _t(c.flat), g, c.dims[1])
    torch.cuda.synchronize()
    return g.cpu().numpy()


def check(c, out, evals, family):
    """Row m of out against the oracle's evaluation evals[m] = (model, data set), per tensor."""
    assert out.dtype == np.float32 and out.shape == (len(evals), c.P)
    worst, bad = 0.0, []
    for m, (mi, di) in enumerate(evals):
        for k, r in enumerate(c.ref(mi, di)):
            a = out[m, c.offs[k]:c.offs[k + 1]].astype(np.float64)
            r = r.reshape(-1)
            scale = max(np.abs(r).max(), np.finfo(np.float32).tiny)
            err = np.abs(a - r).max() / scale if np.isfinite(a).all() else np.inf
            worst = max(worst, err)
            if not normwise_close(a, r, 1e-5):
                bad.append((m, "W1 b1 W2 b2".split()[k], err))
    print(f"{family}: worst normwise error {worst:.3e}")
    assert not bad, bad


def rows_evals(c):
    return list(zip(c.mrow, c.drow))


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_rows_both_ways(gpu, c, family):
    """The case's scattered evaluations, unsplit and with the default batch split."""
    check(c, run_rows(gpu, c), rows_evals(c), family + " unsplit")
    check(c, run_rows(gpu, c, split=True), rows_evals(c), family + " split")


# ------------------------------------------------------------------------------------------
# 1. The plain entry points (mrow == drow == nullptr)
# ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ml,dims", [(1, STD_CNN), (2, STD_2NN)])
def test_plain_entry_points(gpu, ml, dims):
    """cfa_ge_grad_cnn_f32 / cfa_ge_grad_2nn_f32 against the oracle, and bit for bit against the
    rows form with model_row = 0..M-1, data_row = 0 and no workspace: the same kernel, the same
    chains."""
    c = case(ml, dims, 6, 3, Dx=1)
    got = run_plain(gpu, c)
    check(c, got, [(m, 0) for m in range(c.M)], f"plain ml={ml}")
    rows = run_rows(gpu, c, mrow=np.arange(c.M), drow=np.zeros(c.M))
    assert same_bits(got, rows)


# ------------------------------------------------------------------------------------------
# 2. The chunk loop past its first iteration (the !first branches), one workgroup per evaluation
# ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ml,dims,Bc", [(1, STD_CNN, 3), (1, STD_CNN, 2), (1, STD_CNN, 1),
                                        (2, STD_2NN, 3), (2, STD_2NN, 1)])
def test_chunked_launch_equals_unchunked(gpu, monkeypatch, ml, dims, Bc):
    """B = 7 in chunks of Bc (ragged last chunk for 3 and 2) against the oracle, and bit for bit
    against the unchunked launch: every output's chain visits the samples in the same order
    whichever chunk holds them (the partial sum waits in the output bucket between chunks), and
    contraction is off."""
    c = case(ml, dims, 7, 3)
    assert planned_bc(c.plan, c.B) == c.B  # uncapped: the whole batch in one chunk
    whole = run_rows(gpu, c)
    cap = lds_cap(c.plan, Bc)
    assert planned_bc(c.plan, c.B, cap) == Bc < c.B  # capped: more than one chunk
    monkeypatch.setenv("CFA_GRAD_LDS_CAP", str(cap))
    got = run_rows(gpu, c)
    check(c, got, rows_evals(c), f"chunked ml={ml} Bc={Bc}")
    assert same_bits(got, whole)


# ------------------------------------------------------------------------------------------
# 3. Batch split and LDS chunking in one launch (!first accumulation into a workspace partial)
# ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ml,dims", [(1, STD_CNN), (2, STD_2NN)])
def test_split_and_chunked_launch(gpu, monkeypatch, ml, dims):
    """B = 9 over 2 workgroups (5 + 4 samples), each in chunks of 2: against the oracle, and four
    back-to-back launches into one NaN-filled output on one workspace give the same bits."""
    import torch
    c = case(ml, dims, 9, 3)
    cap = lds_cap(c.plan, 2)
    monkeypatch.setenv("CFA_GRAD_SPLIT", "2")
    monkeypatch.setenv("CFA_GRAD_LDS_CAP", str(cap))
    assert gpu.grad_splits(c.M, c.B, c.P) == 2
    Bs = _ceil(c.B, 2)
    assert planned_bc(c.plan, Bs, cap) == 2 < c.B - Bs < Bs  # both workgroups chunk
    ws = gpu.grad_workspace(c.M, c.B, c.P)  # sized under the knob
    assert ws.numel() >= c.M * 2 * c.P
    x, y, flat, mrow, drow = _t(c.x), _t(c.y), _t(c.flat), _t(c.mrow), _t(c.drow)
    g = torch.empty(c.M, c.P, device="cuda")
    outs = []
    for _ in range(4):
        g.fill_(float("nan"))
        gpu.grad_rows(ml, x, y, flat, mrow, drow, g, c.geom, workspace=ws)
        outs.append(g.clone())
    torch.cuda.synchronize()
    outs = [o.cpu().numpy() for o in outs]
    check(c, outs[0], rows_evals(c), f"split+chunked ml={ml}")
    for o in outs[1:]:
        assert same_bits(o, outs[0])


# ------------------------------------------------------------------------------------------
# 4, 5. The <16, 5> template at other lengths, and without register taps
# ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [3, 16, 26, 127, 513])
def test_fast_cnn_other_lengths(gpu, L):
    """The branch-free window path with other pads, a negative t0, positions outside [0, L1), a
    window that is all padding (L = 3 < filter) and L1 no multiple of 5."""
    c = case(1, (L, 5, 16, 8, 8), 4, 3)
    assert c.plan.fast and c.plan.taps_in_regs and L != 512
    if L == 3:
        assert L < 16 and c.plan.L1 == 1
    else:
        assert c.plan.L1 % 5 != 0  # the last pooling window is partly padding
    check_rows_both_ways(gpu, c, f"<16,5> L={L}")


@pytest.mark.parametrize("L,NC", [(127, 3), (127, 6), (513, 16)])
def test_fast_cnn_channel_counts(gpu, L, NC):
    """NC = 3, 6: the block is no multiple of NC, so the <16, 5> kernel reads its taps from LDS in
    the runtime loop; NC = 16: register taps with the channel tid % 16."""
    c = case(1, (L, 5, 16, NC, 8), 4, 3)
    assert c.plan.fast and c.plan.taps_in_regs == (K_BLOCK % NC == 0) == (NC == 16)
    check_rows_both_ways(gpu, c, f"<16,5> NC={NC}")


# ------------------------------------------------------------------------------------------
# 6. The generic CNN kernel at its geometry edges
# ------------------------------------------------------------------------------------------

GENERIC = {"F>kMaxTaps": (50, 3, 40, 4, 33), "S=1": (7, 1, 3, 5, 2), "S>=L": (9, 9, 2, 3, 4),
           "F=1": (40, 4, 1, 8, 8), "F<S": (33, 5, 2, 4, 8)}


@pytest.mark.parametrize("edge", list(GENERIC))
def test_generic_cnn_edges(gpu, edge):
    L, S, F, NC, C = dims = GENERIC[edge]
    assert {"F>kMaxTaps": F > K_MAX_TAPS, "S=1": S == 1, "S>=L": S >= L, "F=1": F == 1, "F<S": F < S}[edge]
    c = case(1, dims, 5, 3)
    assert not c.plan.fast
    check_rows_both_ways(gpu, c, f"generic {edge}")


# ------------------------------------------------------------------------------------------
# 7. Class counts: softmax lane widths 1, 2 and 64, and the refusal above 64
# ------------------------------------------------------------------------------------------

def _class_dims(ml, C):
    return (40, 5, 16, 8, C) if ml == 1 else (40, 8, C)


@pytest.mark.parametrize("ml", [1, 2])
@pytest.mark.parametrize("C", [1, 2, 33, 64])
def test_class_counts(gpu, ml, C):
    width = 1
    while width < C:
        width <<= 1
    assert width == {1: 1, 2: 2, 33: 64, 64: 64}[C]  # softmax_width
    c = case(ml, _class_dims(ml, C), 5, 2)
    plain, rows = run_plain(gpu, c), run_rows(gpu, c)
    check(c, plain, [(m, 0) for m in range(c.M)], f"classes ml={ml} C={C} plain")
    check(c, rows, rows_evals(c), f"classes ml={ml} C={C} rows")
    if C == 1:  # pred = 1 > 0.99: the clip blocks every gradient, as in the oracle
        assert all(not g.any() for m in range(c.M) for g in c.ref(m, 0))
        assert not plain.any() and not rows.any()


@pytest.mark.parametrize("ml", [1, 2])
def test_clip_blocks_predictions_above_its_bound(gpu, ml):
    """Labelled predictions on both sides of 0.99, close enough to it that a gradient let through
    above the bound would show (test_saturated_softmax has pred = 1 - 4e-18 there, where the
    softmax gradient vanishes whether the clip blocks it or not)."""
    c = Case(ml, _class_dims(ml, 4), 8, 2, 1, 0)
    for m in c.models:
        m[2] *= np.float32(0.1)
        m[3][:] = [6.5, 0, 0, 0]  # pred_0 = e^6.5 / (e^6.5 + 3) = 0.9955 before the small W2 term
    c.y = np.eye(4, dtype=np.float32)[[[0, 1, 0, 1, 0, 2, 0, 3]]]
    for m in c.models:
        W1, b1, W2, b2 = [a.astype(np.float64) for a in m]
        if ml == 1:
            logits = orc.tf1_cnn_forward(c.x[0], W1, b1, W2, b2, 5)[0]
        else:
            logits = np.maximum(c.x[0].astype(np.float64) @ W1 + b1, 0.0) @ W2 + b2
        pred = _softmax(logits)[c.y[0] != 0]
        assert ((pred > 0.99) & (pred < 0.999)).sum() == 4 and (pred < 0.99).sum() == 4
    check(c, run_plain(gpu, c), [(0, 0), (1, 0)], f"clip ml={ml}")


@pytest.mark.parametrize("ml", [1, 2])
def test_more_than_64_classes_is_refused(gpu, ml):
    import torch
    from federated_amd._lib import CFAError
    c = case(ml, _class_dims(ml, 65), 2, 2)
    g = torch.full((c.M, c.P), -7.0, device="cuda")
    with pytest.raises(CFAError, match="more than 64 classes"):
        if ml == 1:
            gpu.grad_cnn(_t(c.x[0]), _t(c.y[0]), _t(c.flat), g, 16, 8, 5)
        else:
            gpu.grad_2nn(_t(c.x[0]), _t(c.y[0]), _t(c.flat), g, 8)
    with pytest.raises(CFAError, match="more than 64 classes"):
        gpu.grad_rows(ml, _t(c.x), _t(c.y), _t(c.flat), _t(c.mrow), _t(c.drow), g, c.geom)
    torch.cuda.synchronize()
    assert bool((g == -7.0).all())


# ------------------------------------------------------------------------------------------
# 8. Pooling ties and a maximum of exactly 0, on inputs that are exact in fp32
# ------------------------------------------------------------------------------------------

def _tie_case(fast):
    """Small-integer x, W1 with one tap equal to 1 per channel and b1 = 0: every conv output is a
    copy of an x entry. Exempt from the margin guard: the ties are the point, and nothing before
    the pooling rounds. Returns the case and its [(sample, window, channel, first, second)] ties
    of model 0."""
    rng = np.random.default_rng(77)
    if fast:
        # L1 = 12, L2 = 3, pl = 5, ql = 1: windows p in {0..3}, {4..8} (interior), {9..11} (padded)
        dims, B, taps = (60, 5, 16, 2, 3), 3, [(5, 8), (6, 9)]  # model 0: h0[p] = x[5p], h1[p] = x[5p + 3]
    else:
        # L1 = 4, L2 = 2, pl = ql = 0: windows p in {0, 1}, {2, 3}
        dims, B, taps = (8, 2, 3, 1, 3), 2, [(1,), (0,)]        # model 0: h[p] = x[2p + 1]
    c = Case(1, dims, B, 2, 1, 77, guard=False)
    x = rng.integers(-2, 3, (1, B, dims[0])).astype(np.float32)
    if fast:
        x[0, 0, [25, 35]] = 7       # sample 0: p = 5 and 7 of the interior window
        x[0, 1, [50, 55]] = 6       # sample 1: p = 10 and 11 of the last window, whose p = 12, 13 are padding
        x[0, 2, [0, 5, 10, 15]] = [0, -1, 0, -2]  # sample 2: the first window's maximum is exactly 0
        ties = [(0, 1, 0, 5, 7), (1, 2, 0, 10, 11)]
        zero = (2, 0, 0)
    else:
        x[0, 0] = [3, 1, 3, 2, 1, 5, 1, 5]   # h = 1 2 5 5: window 1 ties at p = 2 and 3
        x[0, 1] = [2, 0, 1, -1, 1, 4, 2, 3]  # h = 0 0 4 3: window 0 has maximum exactly 0
        ties = [(0, 1, 0, 2, 3)]
        zero = (1, 0, 0)
    c.x = x
    for m, ks in enumerate(taps):
        c.models[m][0][:] = 0
        c.models[m][1][:] = 0
        for ch, k in enumerate(ks):
            c.models[m][0][k, 0, ch] = 1
    return c, ties, zero


@pytest.mark.parametrize("fast", [False, True], ids=["generic", "fast"])
def test_pooling_ties_go_to_the_first_maximum(gpu, fast):
    c, ties, zero = _tie_case(fast)
    L, S, F, NC, C = c.dims
    assert c.plan.fast == fast and (c.plan.taps_in_regs or not fast)
    # the inputs do what they were built for (float64 forward pass of model 0)
    _, pooled, arg, (xpad, _, _) = orc.tf1_cnn_forward(c.x[0], *c.models[0], S)
    for b, q, ch, p1, p2 in ties:
        assert arg[b, q, ch] == p1 and pooled[b, q, ch] > 0
        w1, w2 = xpad[b, p1 * S:p1 * S + F], xpad[b, p2 * S:p2 * S + F]
        k = np.flatnonzero(c.models[0][0][:, 0, ch])[0]
        assert w1[k] == w2[k] == pooled[b, q, ch]  # two equal maxima ...
        assert not np.array_equal(w1, w2)          # ... whose neighbours differ: the winner shows in gW1
    assert pooled[zero] == 0.0
    evals = [(0, 0), (1, 0)]
    check(c, run_plain(gpu, c), evals, f"ties fast={fast}")
    check(c, run_rows(gpu, c, split=True, mrow=[0, 1], drow=[0, 0]), evals, f"ties fast={fast} split")


@pytest.mark.parametrize("fast", [False, True], ids=["generic", "fast"])
def test_zero_maximum_gives_no_gradient(gpu, fast):
    """Every window's maximum is exactly 0 (x <= 0 through a unit tap): the relu passes nothing, so
    the gradients of W1, b1 and W2 are exactly 0 and only b2's is not."""
    c, _, _ = _tie_case(fast)
    c.x = -np.abs(c.x)
    got = run_plain(gpu, c)
    check(c, got, [(0, 0), (1, 0)], f"zero maximum fast={fast}")
    assert not got[:, :c.offs[3]].any() and got[:, c.offs[3]:].all()


# ------------------------------------------------------------------------------------------
# 9. 2NN layouts
# ------------------------------------------------------------------------------------------

NN_LAYOUTS = {"W1 from global": (512, 48, 8, 5), "partial slice, scalar gW1": (70, 7, 5, 5),
              "dz misaligned": (33, 4, 3, 4), "one input": (1, 1, 2, 3), "one short slice": (31, 16, 8, 4)}


@pytest.mark.parametrize("layout", list(NN_LAYOUTS))
def test_2nn_layouts(gpu, layout):
    L, H, C, B = NN_LAYOUTS[layout]
    dims = (L, H, C)
    c = case(2, dims, B, 3)
    assert planned_bc(c.plan, B) == B
    if layout == "W1 from global":
        assert not c.plan.w_in_regs and c.plan.G * H > K_BLOCK
    else:
        assert c.plan.w_in_regs and L % K_SPAN != 0  # a partial last slice
    if layout == "partial slice, scalar gW1":
        assert L > K_SPAN and H % 4 != 0
    if layout == "dz misaligned":
        assert H % 4 == 0 and not nn_dz_aligned(dims, B)  # H4 == 0 although H % 4 == 0
    if layout == "one short slice":
        assert L < K_SPAN and H % 4 == 0 and nn_dz_aligned(dims, B) and c.P % 4 == 0  # aligned float4
    check_rows_both_ways(gpu, c, f"2NN {layout}")


@pytest.mark.parametrize("B,Bc", [(2, 2), (4, 2)], ids=["one chunk", "two chunks"])
def test_2nn_float4_on_a_misaligned_row(gpu, monkeypatch, B, Bc):
    """H % 4 == 0 and dz aligned in LDS, but P % 4 != 0: the odd gradient rows are not 16-byte
    aligned, so the float4 path stores (and, in the second chunk, reloads) them as scalars."""
    dims = (5, 4, 2)
    c = case(2, dims, B, 3)
    assert c.P == 34 and c.P % 4 != 0 and dims[1] % 4 == 0
    assert (dims[2] + Bc * dims[0]) % 4 == 0 and nn_dz_aligned(dims, Bc)
    if Bc < B:
        cap = lds_cap(c.plan, Bc)
        assert planned_bc(c.plan, B, cap) == Bc < B
        monkeypatch.setenv("CFA_GRAD_LDS_CAP", str(cap))
    else:
        assert planned_bc(c.plan, B) == Bc
    # unsplit: row m of the output starts at m * P floats, so row 1 is misaligned
    check(c, run_rows(gpu, c), rows_evals(c), f"2NN float4 misaligned B={B}")
    check(c, run_plain(gpu, c, 1), [(m, 1) for m in range(c.M)], f"2NN float4 misaligned plain B={B}")


# ------------------------------------------------------------------------------------------
# 10. One sample does not fit the workgroup's LDS
# ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ml,dims", [(1, STD_CNN), (2, STD_2NN)])
def test_sample_that_does_not_fit_is_refused(gpu, monkeypatch, ml, dims):
    import torch
    from federated_amd._lib import CFAError
    c = case(ml, dims, 6, 3, Dx=1)
    cap = lds_cap(c.plan, 1) - 4
    assert planned_bc(c.plan, c.B, cap) == 0
    monkeypatch.setenv("CFA_GRAD_LDS_CAP", str(cap))
    g = torch.full((c.M, c.P), -7.0, device="cuda")
    with pytest.raises(CFAError, match="does not fit"):
        if ml == 1:
            gpu.grad_cnn(_t(c.x[0]), _t(c.y[0]), _t(c.flat), g, 16, 8, 5)
        else:
            gpu.grad_2nn(_t(c.x[0]), _t(c.y[0]), _t(c.flat), g, 32)
    with pytest.raises(CFAError, match="does not fit"):
        gpu.grad_rows(ml, _t(c.x), _t(c.y), _t(c.flat), _t(c.mrow), _t(c.drow), g, c.geom,
                      workspace=gpu.grad_workspace(c.M, c.B, c.P))
    torch.cuda.synchronize()
    assert bool((g == -7.0).all())  # nothing was launched


# ------------------------------------------------------------------------------------------
# 11. Batch invariance
# ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ml,dims", [(1, STD_CNN), (2, STD_2NN)])
def test_evaluation_does_not_depend_on_its_launch(gpu, ml, dims):
    """An evaluation inside an M = 5 launch with scattered rows over 3 data sets has the bits of
    the same evaluation launched alone (M = 1), both unsplit."""
    c = case(ml, dims, 6, 3, Dx=3)
    mrow, drow = [2, 0, 1, 0, 2], [1, 2, 0, 0, 2]
    many = run_rows(gpu, c, mrow=mrow, drow=drow)
    check(c, many, list(zip(mrow, drow)), f"batch invariance ml={ml}")
    for m in range(5):
        alone = run_rows(gpu, c, mrow=[mrow[m]], drow=[drow[m]])
        assert same_bits(alone[0], many[m]), m
