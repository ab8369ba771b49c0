"""The cases of tests/test_lenet_huber_host.py and tests/test_gpu_lenet_huber.py: the Huber drivers'
objective on the LeNet-1 family, restated in numpy fp64 on top of the forward and backward
restatements of tests/lenet_cases.py and tests/lenet_grad_cases.py (no torch here).

The objective (federated_learning_keras_consensus_FL_MNIST.py:369-377): keras.losses.Huber(),
delta = 1, between the integer label ITSELF, cast to float, and the softmax probability of the true
class. Per sample with label l and logits z: p = softmax(z)[l], e = p - l, h = 0.5 e^2 where
|e| <= 1, else |e| - 0.5; the batch loss is the mean of h. At the logits
dz[c] = g p ((c == l) - softmax(z)[c]) with g = e on the quadratic branch and sign(e) on the linear
one; `grads` differs from lenet_grad_cases.grads in these lines alone.

With 0 < p < 1 the label alone picks the branch: 0 the quadratic one on p, 1 the quadratic one on
1 - p, 2 and above the linear one. lenet_cases.make draws labels at random, so a case here has a
label vector of its own (`labels_of`): position i holds kind i % 3 (kind 0: label 0; kind 1: label
1; kind 2: the labels 2 .. C - 1 in turn; with two classes i % 2), and the last position holds
C - 1. Then every batch of `batches_used`, which lists every batch the host and GPU tests evaluate,
holds a label 0, a label 1 and, where C > 2, a label >= 2, and every case holds its label C - 1
(lenet1: 9). Not every start of a batch of 3 in a set of 7 can do that (the kinds would have to
have period 3 around a ring of 7), so the tests take their starts from the table below. The
images and models are lenet_cases.make's for the case's seed.

The seed rule is lenet_grad_cases' with this gradient: the relu-gate margin over every model and
sample of the set, and no tensor's gradient all zero for any model on any batch of the set (every
start, wrapping); a case's seed is the smallest that meets it, and the host test derives it again."""
import numpy as np

import lenet_cases as lc
import lenet_grad_cases as gc

D = gc.D
# name: (geometry, batch, Nt, seed): shapes from lenet_grad_cases.CASES, the seed this module's own
CASES = {
    "lenet1": (lc.LENET1, 6, 13, 3),             # the K = 5 kernels, a full group and a partial one, labels up to 9
    "pool2_drops": ((12, 3, 2, 3, 4), 3, 7, 0),  # the runtime-k kernels, a partial chunk
    "lanes_64": ((10, 3, 1, 1, 2), 3, 7, 34),    # two classes: the linear branch is never taken
    "classes_64": ((12, 3, 2, 3, 64), 3, 7, 0),  # four logit passes
    "finish_256": ((14, 3, 4, 4, 4), 3, 7, 2),   # the loss in a second finish block
}
VAL_BATCHES = 2  # the validation tests' batches: samples [0, batch) and [batch, 2 batch) of a set
CAPTURED = ("lenet1", 4)  # the captured chain: two epochs of two batches, the cursor moving on by a batch each


def shifts(name):
    """The per-device sets: device d's is the shared one rolled by 3 d samples (a roll by a
    multiple of 3 keeps the kinds of the positions)."""
    return [3 * d % CASES[name][2] for d in range(D)]


def firsts(name):
    """The `first` of the batch-position tests: the last one's batch wraps after one sample, the
    second lies a whole set further."""
    Nt = CASES[name][2]
    return [3, Nt + 1, Nt - 1]


def batches_used(name):
    """(shift, first) of every batch a test evaluates: the gradient on the shared set and on the
    per-device sets, the batch positions, the validation batches on either kind of set, and the
    batches the captured chain's cursor reaches."""
    _, batch, Nt, _ = CASES[name]
    out = [(s, b * batch) for s in shifts(name) for b in range(VAL_BATCHES)]
    out += [(0, f) for f in firsts(name)]
    if name == CAPTURED[0]:
        out += [(0, b * batch % Nt) for b in range(CAPTURED[1])]
    return out


def labels_of(name):
    geom, _, Nt, _ = CASES[name]
    C = geom[4]
    if C == 2:
        lab = np.arange(Nt) % 2
    else:
        lab = np.arange(Nt) % 3
        high = np.flatnonzero(lab == 2)
        lab[high] = 2 + np.arange(len(high)) % (C - 2)
    lab[Nt - 1] = C - 1
    return lab.astype(np.int32)


def batch_index(name, first=0, shift=0):
    _, batch, Nt, _ = CASES[name]
    return (np.arange(batch) + first + shift) % Nt


def huber(p, labels):
    """(h, g) per sample: Keras Huber(delta = 1) of e = p - label and its derivative in e."""
    e = p - labels.astype(np.float64)
    quad = np.abs(e) <= 1.0
    return np.where(quad, 0.5 * e * e, np.abs(e) - 0.5), np.where(quad, e, np.sign(e))


def loss_of(x, labels, row, geom):
    """fp64 batch-mean Huber loss of the model `row` on x [n, side, side] / labels [n]."""
    n = len(labels)
    p = np.exp(lc.log_probs(x, row, geom))[np.arange(n), labels]
    return float(huber(p, labels)[0].mean())


def grads(x, labels, row, geom):
    """lenet_grad_cases.grads with the Huber objective: fp64 (gradient [P], batch-mean loss)."""
    K1, b1, K2, b2, Wd, bd = (t.astype(np.float64) for t in lc.split(row, geom))
    h0, z1, a1, z2, a2 = gc._forward(x, row, geom)
    n = h0.shape[0]
    flat = a2.reshape(n, -1)
    z = flat @ Wd + bd
    z = z - z.max(axis=1, keepdims=True)
    sm = np.exp(z - np.log(np.exp(z).sum(axis=1, keepdims=True)))
    p = sm[np.arange(n), labels]
    h, g = huber(p, labels)
    onehot = np.zeros_like(sm)
    onehot[np.arange(n), labels] = 1.0
    dz = (g * p)[:, None] * (onehot - sm)
    dWd, dbd, dflat = flat.T @ dz, dz.sum(axis=0), dz @ Wd.T
    dz2 = gc._unpool(dflat.reshape(a2.shape), z2.shape) * (z2 > 0)
    dK2, db2, da1 = gc._conv_backward(a1, K2, dz2, True)
    dz1 = gc._unpool(da1, z1.shape) * (z1 > 0)
    dK1, db1, _ = gc._conv_backward(h0, K1, dz1, False)
    out = np.concatenate([t.reshape(-1) for t in (dK1, db1, dK2, db2, dWd, dbd)]) / n
    return out, float(h.mean())


def meets_the_seed_rule(name, seed):
    """lenet_grad_cases.meets_the_seed_rule with this module's labels and gradient."""
    geom, batch, Nt, _ = CASES[name]
    x, _, models = lc.make(geom, D, Nt, seed)
    labels = labels_of(name)
    for row in models:
        lo, hi = gc.margin(x, row, geom)
        if not (lo >= gc.GUARD * hi and gc.preactivation_shift(x, row, geom) <= 0.1 * lo):
            return False
        for first in range(Nt):
            idx = batch_index(name, first)
            if not all(np.abs(t).max() > 0 for t in gc.tensors(grads(x[idx], labels[idx], row, geom)[0], geom)):
                return False
    return True


_DATA, _REF, _COST = {}, {}, {}


def data(name):
    """(x [Nt, side, side] fp32, labels [Nt] int32, models [D, P] fp32) of a case: read only."""
    if name not in _DATA:
        geom, _, Nt, seed = CASES[name]
        x, _, models = lc.make(geom, D, Nt, seed)
        _DATA[name] = (x, labels_of(name), models)
        for a in _DATA[name]:
            a.setflags(write=False)
    return _DATA[name]


def per_device(name):
    """(x [D, Nt, side, side], labels [D, Nt]): device d's set is the shared one rolled by shifts[d]."""
    x, labels, _ = data(name)
    s = shifts(name)
    return np.stack([np.roll(x, -k, axis=0) for k in s]), np.stack([np.roll(labels, -k) for k in s])


def reference(name, model, first=0, shift=0):
    """fp64 (gradient, loss) of model row `model` on the case's batch that starts at sample `first`
    (wrapping) of the shared set rolled by `shift`; computed once per key and shared."""
    key = (name, model, first, shift)
    if key not in _REF:
        x, labels, models = data(name)
        idx = batch_index(name, first, shift)
        g, loss = grads(x[idx], labels[idx], models[model], CASES[name][0])
        g.setflags(write=False)
        _REF[key] = (g, loss)
    return _REF[key]


def costs(name, per_device_sets=False):
    """fp64 validation cost [D] over VAL_BATCHES batches: the mean of the batch losses, each the
    mean of its samples' Huber losses; shared set, or the per-device ones. Computed once."""
    key = (name, per_device_sets)
    if key not in _COST:
        geom, batch, _, _ = CASES[name]
        x, labels, models = data(name)
        out = np.zeros(D)
        for d in range(D):
            shift = shifts(name)[d] if per_device_sets else 0
            per = []
            for b in range(VAL_BATCHES):
                idx = batch_index(name, b * batch, shift)
                per.append(loss_of(x[idx], labels[idx], models[d], geom))
            out[d] = np.mean(per)
        out.setflags(write=False)
        _COST[key] = out
    return _COST[key]
