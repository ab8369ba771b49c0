"""The cases of tests/test_lenet_max_host.py and tests/test_gpu_lenet_max.py: the TF2 drivers'
max-pool CNNs (create_q_model, -modelselection 1 and "any other value") restated in numpy fp64 from
the layer definitions, forward and backward, on the geometry, row layout, convolution and data of
tests/lenet_cases.py and tests/lenet_grad_cases.py (no torch here).

The family: Conv2D(c1, k x k, valid, relu) -> MaxPooling2D(2 x 2, stride 2, valid) -> Conv2D(c2) ->
MaxPooling2D -> Flatten (NHWC) -> Dense(classes, softmax). The pool takes the largest relu(z) of a
window and drops an odd last row and column. Backward, the whole of d(pooled) goes to the FIRST
largest relu(z) in window order (0,0), (0,1), (1,0), (1,1) (TF's MaxPoolGrad; numpy's argmax also
returns the first) and then through that position's relu gate z > 0, so a window without a positive
z passes nothing; a dropped row or column receives 0. Everything else is lenet_grad_cases'.

An fp32 and this fp64 evaluation must take the same discrete decisions, or a gradient moves by a
whole term. So a case's seed is the smallest for which, over EVERY model and EVERY sample of its
set, (1) the smallest |pre-activation| of both convolutions stays above GUARD (lenet_grad_cases',
1e-5) of the largest, (2) in every window whose maximum is positive the two largest relu(z) lie
further apart than GUARD of the largest pre-activation, (3) a numpy fp32 evaluation moves no
pre-activation by more than a tenth of the smaller of those two distances, and (4) no model has a
tensor whose gradient is all zero on any batch of the set, for either objective.
test_lenet_max_host.py derives every seed again. The drivers' geometries have 29 376
pre-activations and 7 008 windows a sample: with three models and three samples (28, 3, 14, 64, 10)
first meets the rule at seed 682 and (28, 3, 32, 64, 10) not below 1 500, so their sets are shrunk
to one model and two samples (one batch), where seeds 4 and 11 meet it; the search is bounded by
SEED_BOUND and the guard is never shrunk.

PLAN restates the launch plan of cfa_lenet_max.hip from the geometry, the batch and the LDS limit
alone, and `path` names the arithmetic that puts a case on the loop, tail or branch it exists for."""
import numpy as np

import lenet_cases as lc
import lenet_grad_cases as gc
import lenet_huber_cases as hc

MNIST_CNN32 = (28, 3, 32, 64, 10)
MNIST_CNN14 = (28, 3, 14, 64, 10)
GUARD = gc.GUARD
SEED_BOUND = 4000  # seeds tried before a case's set would have to shrink further
LOSSES = ("xent", "huber")

# name: (geometry, batch, Nt, D, seed)
CASES = {
    "pool2_drops": ((12, 3, 2, 3, 4), 3, 7, 3, 0),   # conv2 output 3: the second pool drops; chunks of 2 and 1
    "pool1_drops": ((14, 4, 3, 5, 3), 3, 7, 3, 0),   # conv1 output 11: the first pool drops; the runtime-k kernels
    "map_1x1": ((13, 4, 3, 5, 3), 3, 7, 3, 0),       # a 1 x 1 final map
    "generic_k": ((20, 4, 3, 4, 5), 5, 11, 3, 0),    # runtime k, both pools drop; validation chunks of 4 and 1
    "two_groups": ((12, 3, 2, 3, 4), 9, 10, 3, 2),   # a full group of 8 samples (four chunks) and a group of 1
    "finish_256": ((14, 3, 4, 4, 4), 3, 7, 3, 2),    # P + 1 = 257: a second finish block of one live thread
    "cnn14": (MNIST_CNN14, 2, 2, 1, 4),              # 2 samples a gradient chunk, 3 a validation chunk
    "cnn32": (MNIST_CNN32, 2, 2, 1, 11),             # 1 sample a gradient chunk (two passes), 2 a validation chunk
}
SMALL = tuple(n for n in CASES if not n.startswith("cnn"))
# validation only (costs take no discrete decision that a 1e-5 comparison could see): name: (geometry,
# batch, batches, Nt, D)
EVAL_CASES = {
    "cnn32_tail": (MNIST_CNN32, 3, 1, 4, 3),           # validation chunks of 2 and 1 samples
    "cnn14_tail": (MNIST_CNN14, 4, 1, 5, 3),           # validation chunks of 3 and 1 samples
    "chunk_tail_2": ((12, 3, 2, 3, 4), 6, 2, 13, 3),   # chunks of 4 and 2 samples, two batches
    "raised_lds": ((90, 3, 4, 2, 3), 2, 1, 3, 3),      # one sample's activations above 64 KiB
}

# cfa_lenet_global.h: kGlobalBlock, kGlobalEvalChunk, kGlobalGradChunk, kGlobalGroup
BLOCK, EVAL_CHUNK, GRAD_CHUNK, GROUP = 512, 4, 2, 8
LDS_LIMIT = 160 * 1024


def sample_floats(geom):
    """lenet_sample_floats: image, two pooled maps, logits."""
    side, k, c1, c2, classes = geom
    _, p1, _, p2 = lc.stages(geom)
    return side * side + p1 * p1 * c1 + p2 * p2 * c2 + classes


def eval_lds_bytes(geom, n, batch):
    return 4 * (n * sample_floats(geom) + batch)


def eval_chunk(geom, batch, lds_limit=LDS_LIMIT):
    """lenet_global_eval_chunk: the most samples (up to 4) within 64 KiB, else 1 under the limit, else 0."""
    for n in range(EVAL_CHUNK, 0, -1):
        if eval_lds_bytes(geom, n, batch) <= lc.LDS_DEFAULT:
            return n
    return 1 if eval_lds_bytes(geom, 1, batch) <= lds_limit else 0


def grad_lds_bytes(geom, n):
    """lenet_global_grad_lds: n samples' activations and gradients, the weight tile, a group's losses,
    the chunk's labels, the decision bytes."""
    side, k, c1, c2, classes = geom
    _, p1, _, p2 = lc.stages(geom)
    n1, flat = p1 * p1 * c1, p2 * p2 * c2
    sample = side * side + 2 * n1 + 2 * flat + 2 * classes + 4 * flat
    return 4 * (n * sample + c1 * (c2 + 1) + GROUP + n + (n * (n1 + flat) + 3) // 4)


def grad_chunk(geom, lds_limit=LDS_LIMIT):
    for n in range(GRAD_CHUNK, 0, -1):
        if grad_lds_bytes(geom, n) <= lds_limit:
            return n
    return 0


def grad_workspace_bytes(geom, batch, D):
    return 4 * D * ((batch + GROUP - 1) // GROUP) * (lc.size(geom) + GROUP)


def plan(geom, batch, lds_limit=LDS_LIMIT):
    """The launch plan of a geometry and a batch: kernel, chunks and their tails, groups, LDS, the
    weight-gradient items against the workgroup, the tile copy's passes, the finish blocks."""
    side, k, c1, c2, classes = geom
    ec, gcn = eval_chunk(geom, batch, lds_limit), grad_chunk(geom, lds_limit)
    groups = (batch + GROUP - 1) // GROUP
    last = batch - GROUP * (groups - 1)
    return {"fast": k == 3, "s": lc.stages(geom), "eval_chunk": ec, "eval_tail": batch % ec if ec else None,
            "eval_lds": eval_lds_bytes(geom, ec, batch) if ec else None,
            "grad_chunk": gcn, "grad_lds": grad_lds_bytes(geom, gcn) if gcn else None,
            "groups": groups, "last": last, "last_tail": last % gcn if gcn else None,
            "items": (k * c1, k * c1 * c2), "L": (gc.lanes(k * c1, BLOCK), gc.lanes(k * c1 * c2, BLOCK)),
            "tile_passes": -(-c1 * c2 // BLOCK), "finish_blocks": -(-(lc.size(geom) + 1) // 256)}


def path(name, lds_limit=LDS_LIMIT):
    """The conditions that put the case `name` on the path it exists for, {text: bool}."""
    if name in CASES:
        geom, batch = CASES[name][:2]
    else:
        geom, batch = EVAL_CASES[name][:2]
    p, P = plan(geom, batch, lds_limit), lc.size(geom)
    s1, p1, s2, p2 = p["s"]
    if name == "pool2_drops":
        return {"the k = 3 kernels": p["fast"], "the second pool drops": s2 % 2 == 1 and s1 % 2 == 0,
                "gradient chunks of 2 and 1": p["grad_chunk"] == 2 and batch == 3,
                "one partial validation chunk": batch < p["eval_chunk"] == 4}
    if name == "pool1_drops":
        return {"the runtime-k kernels": not p["fast"], "the first pool drops": s1 % 2 == 1}
    if name == "map_1x1":
        return {"a 1 x 1 final map": p2 == 1}
    if name == "generic_k":
        return {"the runtime-k kernels": not p["fast"], "both pools drop": s1 % 2 == 1 and s2 % 2 == 1,
                "validation chunks of 4 and 1": p["eval_chunk"] == 4 and p["eval_tail"] == 1,
                "gradient chunks of 2, 2 and 1 in one group": (p["grad_chunk"], p["groups"], batch) == (2, 1, 5)}
    if name == "two_groups":
        return {"a full group of four chunks, then a group of one sample":
                    (p["groups"], p["last"], p["grad_chunk"]) == (2, 1, 2) and batch > GROUP,
                "validation chunks of 4, 4 and 1": p["eval_chunk"] == 4 and batch == 9}
    if name == "finish_256":
        return {"P + 1 = 257: 2 finish blocks": (P + 1, p["finish_blocks"]) == (257, 2)}
    if name == "cnn14":
        return {"P = 24 278": P == 24278, "28 -> 26 -> 13 -> 11 -> 5": p["s"] == (26, 13, 11, 5),
                "2 samples a gradient chunk: 132 700 bytes of LDS, above the default":
                    (p["grad_chunk"], p["grad_lds"]) == (2, 132700) and p["grad_lds"] > lc.LDS_DEFAULT,
                "3 * 14 * 64 = 2 688 items > 512: one lane each, six passes": p["items"][1] == 2688 and p["L"][1] == 1,
                "the tile copy's second pass: 14 * 64 > 512": p["tile_passes"] == 2}
    if name == "cnn32":
        return {"P = 34 826": P == 34826, "28 -> 26 -> 13 -> 11 -> 5": p["s"] == (26, 13, 11, 5),
                "1 sample a gradient chunk (two would need 192 136 bytes): 100 244 bytes of LDS":
                    (p["grad_chunk"], p["grad_lds"], grad_lds_bytes(geom, 2)) == (1, 100244, 192136)
                    and grad_lds_bytes(geom, 2) > lds_limit,
                "two passes of one sample": batch == 2,
                "2 samples a validation chunk": p["eval_chunk"] == 2}
    if name == "cnn32_tail":
        return {"validation chunks of 2 and 1: 62 428 bytes of LDS": (p["eval_chunk"], p["eval_tail"], p["eval_lds"])
                == (2, 1, 62428)}
    if name == "cnn14_tail":
        return {"validation chunks of 3 and 1": (p["eval_chunk"], p["eval_tail"]) == (3, 1)}
    if name == "chunk_tail_2":
        return {"validation chunks of 4 and 2": (p["eval_chunk"], p["eval_tail"]) == (4, 2)}
    if name == "raised_lds":
        return {"one sample: 66 924 bytes of LDS": (p["eval_chunk"], p["eval_lds"]) == (1, 66924),
                "above the default limit": p["eval_lds"] > lc.LDS_DEFAULT, "within the device's": p["eval_lds"] <= lds_limit}
    raise KeyError(name)


# ---- the restatement ------------------------------------------------------------------------

def _windows(h):
    """The 2 x 2 windows of an NHWC map, [n, p, p, c, 4] in window order (0,0), (0,1), (1,0), (1,1);
    an odd last row and column are dropped."""
    p = h.shape[1] // 2
    h = h[:, :2 * p, :2 * p, :]
    return np.stack([h[:, 0::2, 0::2], h[:, 0::2, 1::2], h[:, 1::2, 0::2], h[:, 1::2, 1::2]], axis=-1)


def max_pool(h):
    """MaxPooling2D(2 x 2, stride 2, valid), NHWC."""
    return _windows(h).max(axis=-1)


def _forward(x, row, geom, dtype=np.float64):
    conv = lc.conv_valid if dtype == np.float64 else gc._conv32
    K1, b1, K2, b2, Wd, bd = (t.astype(dtype) for t in lc.split(row, geom))
    h0 = np.asarray(x, dtype=dtype)[..., None]
    z1 = conv(h0, K1, b1)
    a1 = max_pool(np.maximum(z1, 0)).astype(dtype)
    z2 = conv(a1, K2, b2)
    a2 = max_pool(np.maximum(z2, 0)).astype(dtype)
    return h0, z1, a1, z2, a2


def log_probs(x, row, geom):
    """fp64 log softmax of the model `row` on images x [n, side, side]: [n, classes]."""
    _, _, _, _, a2 = _forward(x, row, geom)
    _, _, _, _, Wd, bd = (t.astype(np.float64) for t in lc.split(row, geom))
    z = a2.reshape(a2.shape[0], -1) @ Wd + bd
    z = z - z.max(axis=1, keepdims=True)
    return z - np.log(np.exp(z).sum(axis=1, keepdims=True))


def sample_losses(x, labels, row, geom, loss="xent"):
    lp = log_probs(x, row, geom)
    n = len(labels)
    if loss == "huber":
        return hc.huber(np.exp(lp)[np.arange(n), labels], labels)[0]
    return -lp[np.arange(n), labels]


def loss_of(x, labels, row, geom, loss="xent"):
    """fp64 batch-mean loss of the model `row` on x [n, side, side] / labels [n]."""
    return float(sample_losses(x, labels, row, geom, loss).mean())


def _unpool(d, z):
    """The max pool's backward and the relu gate behind it: d [n, p, p, c] to the first largest
    relu(z) of each window of z [n, s, s, c], where that z > 0; 0 everywhere else."""
    w = _windows(np.maximum(z, 0))
    at = w.argmax(axis=-1)  # the first maximum
    p = d.shape[1]
    out = np.zeros(z.shape)
    for j, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        out[:, dy:2 * p:2, dx:2 * p:2, :] = d * (at == j)
    return out * (z > 0)


def grads(x, labels, row, geom, loss="xent"):
    """fp64 (gradient [P], the six tensors flattened in row order; batch-mean loss) of the model
    `row` on the batch x [n, side, side] / labels [n], for the objective `loss`."""
    K1, b1, K2, b2, Wd, bd = (t.astype(np.float64) for t in lc.split(row, geom))
    h0, z1, a1, z2, a2 = _forward(x, row, geom)
    n = h0.shape[0]
    flat = a2.reshape(n, -1)
    z = flat @ Wd + bd
    z = z - z.max(axis=1, keepdims=True)
    lp = z - np.log(np.exp(z).sum(axis=1, keepdims=True))
    sm = np.exp(lp)
    onehot = np.zeros_like(sm)
    onehot[np.arange(n), labels] = 1.0
    if loss == "huber":
        p = sm[np.arange(n), labels]
        h, g = hc.huber(p, labels)
        dz, value = (g * p)[:, None] * (onehot - sm), float(h.mean())
    else:
        dz, value = sm - onehot, float(-lp[np.arange(n), labels].mean())
    dWd, dbd, dflat = flat.T @ dz, dz.sum(axis=0), dz @ Wd.T
    dz2 = _unpool(dflat.reshape(a2.shape), z2)
    dK2, db2, da1 = gc._conv_backward(a1, K2, dz2, True)
    dz1 = _unpool(da1, z1)
    dK1, db1, _ = gc._conv_backward(h0, K1, dz1, False)
    out = np.concatenate([t.reshape(-1) for t in (dK1, db1, dK2, db2, dWd, dbd)]) / n
    return out, value


# ---- the seed rule --------------------------------------------------------------------------

def _gap(z):
    """The smallest distance between the two largest relu(z) over the windows whose maximum is positive."""
    w = np.sort(_windows(np.maximum(z, 0)), axis=-1)
    live = w[..., 3] > 0
    return float((w[..., 3] - w[..., 2])[live].min()) if live.any() else np.inf


def decisions(x, row, geom):
    """(smallest |pre-activation|, smallest window gap, largest |pre-activation|, largest |fp32 - fp64|
    pre-activation) over both convolutions and every sample of x."""
    _, z1, _, z2, _ = _forward(x, row, geom)
    _, y1, _, y2, _ = _forward(x, row, geom, np.float32)
    a = np.concatenate([np.abs(z1).reshape(-1), np.abs(z2).reshape(-1)])
    shift = max(np.abs(z1 - y1).max(), np.abs(z2 - y2).max())
    return float(a.min()), min(_gap(z1), _gap(z2)), float(a.max()), float(shift)


def _stage1_clear(x, row, geom):
    """The rule's first half on the first convolution alone (a cheap early exit of the search: the
    largest pre-activation of both stages is at least this stage's)."""
    K1, b1 = (t.astype(np.float64) for t in lc.split(row, geom)[:2])
    z1 = lc.conv_valid(np.asarray(x, dtype=np.float64)[..., None], K1, b1)
    return np.abs(z1).min() >= GUARD * np.abs(z1).max() and _gap(z1) >= GUARD * np.abs(z1).max()


def meets_the_seed_rule(geom, batch, Nt, D, seed):
    x, labels, models = lc.make(geom, D, Nt, seed)
    for row in models:
        if not _stage1_clear(x, row, geom):
            return False
        lo, gap, hi, shift = decisions(x, row, geom)
        if not (lo >= GUARD * hi and gap >= GUARD * hi and shift <= 0.1 * min(lo, gap)):
            return False
        for first in range(Nt if Nt > batch else 1):
            idx = (np.arange(batch) + first) % Nt
            for loss in LOSSES:
                if not all(np.abs(t).max() > 0 for t in gc.tensors(grads(x[idx], labels[idx], row, geom, loss)[0], geom)):
                    return False
    return True


def smallest_seed(name):
    geom, batch, Nt, D, _ = CASES[name]
    for seed in range(SEED_BOUND):
        if meets_the_seed_rule(geom, batch, Nt, D, seed):
            return seed
    return None


# ---- data and references, computed once and shared: read only --------------------------------

_DATA, _REF, _COST = {}, {}, {}


def data(name):
    """(x [Nt, side, side] fp32, labels [Nt] int32, models [D, P] fp32) of a case."""
    if name not in _DATA:
        if name in CASES:
            geom, _, Nt, D, seed = CASES[name]
        else:
            (geom, _, _, Nt, D), seed = EVAL_CASES[name], 0
        _DATA[name] = lc.make(geom, D, Nt, seed)
        for a in _DATA[name]:
            a.setflags(write=False)
    return _DATA[name]


def per_device(name):
    """One set per device from the case's own samples: device d's set is the shared one rolled by d."""
    x, labels, _ = data(name)
    D = CASES[name][3]
    return np.stack([np.roll(x, -d, axis=0) for d in range(D)]), np.stack([np.roll(labels, -d) for d in range(D)])


def reference(name, model, first=0, shift=0, loss="xent"):
    """fp64 (gradient, loss) of model row `model` on the case's batch that starts at sample `first`
    (wrapping) of the shared set rolled by `shift`."""
    key = (name, model, first, shift, loss)
    if key not in _REF:
        geom, batch, Nt = CASES[name][:3]
        x, labels, models = data(name)
        idx = (np.arange(batch) + first + shift) % Nt
        g, value = grads(x[idx], labels[idx], models[model], geom, loss)
        g.setflags(write=False)
        _REF[key] = (g, value)
    return _REF[key]


def costs(name, batch, batches, loss="xent"):
    """fp64 validation cost [D] of the case's models on the first batch * batches samples of the
    shared set: the mean of the batch losses, each the mean of its samples' losses."""
    key = (name, batch, batches, loss)
    if key not in _COST:
        geom = (CASES.get(name) or EVAL_CASES[name])[0]
        x, labels, models = data(name)
        n = batch * batches
        out = np.array([sample_losses(x[:n], labels[:n], row, geom, loss).reshape(batches, batch).mean(axis=1).mean()
                        for row in models])
        out.setflags(write=False)
        _COST[key] = out
    return _COST[key]
