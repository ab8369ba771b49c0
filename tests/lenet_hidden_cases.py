"""The cases of tests/test_lenet_hidden_host.py and tests/test_gpu_lenet_hidden.py: the CIFAR
drivers' hidden-layer LeNet (federated_learning_keras_consensus_FL_threads_CIFAR_crossentropy.py:179-186,
-modelselection 1) restated in numpy fp64 from the layer definitions, forward and backward, with the
convolution, pool, unpool and Huber helpers of tests/lenet_cases.py, lenet_grad_cases.py and
lenet_huber_cases.py, which already take any number of input channels (no torch here).

The family, seven numbers (side, channels, kernel, c1, c2, hidden, classes): x [side, side, channels]
-> Conv2D(c1, k x k, valid, relu) -> AveragePooling2D(2 x 2, stride 2, valid) -> Conv2D(c2) ->
AveragePooling2D -> Flatten (NHWC) -> Dense(hidden, relu) -> Dense(classes, softmax). A model row
is get_weights() order, C-order: K1 (k, k, channels, c1) b1 K2 (k, k, c1, c2) b2 Wh (flat, hidden) bh
Wd (hidden, classes) bd. Backward through the hidden layer: dh = (dz Wd^T) where its pre-activation
is > 0 (TF's ReluGrad), dWh = flat^T dh, dbh = sum dh, dflat = dh Wh^T; the rest is lenet_grad_cases'.

A relu gate that differs between an fp32 and this fp64 evaluation moves a gradient by a whole term,
so a case's seed is the smallest for which, over EVERY model and EVERY sample of its set, (1) the
smallest |pre-activation| of both convolutions AND the hidden layer stays above GUARD
(lenet_grad_cases', 1e-5) of the largest, (2) a numpy fp32 evaluation moves no pre-activation by
more than a tenth of that distance, (3) no model has a tensor whose gradient is all zero on
any batch of the set, for either objective, and (4) no tensor's gradient is so ill-conditioned that
numpy's own fp32 evaluation of the restatement (`grads(..., dtype=np.float32)`) misses the fp64 one
by more than CONDITION = 1e-5 normwise, the tolerance the device is held to: a bias gradient is a sum
of terms of both signs, and where they cancel to a thousandth of their size (the second bias of
(10, 2, 3, 3, 3, 16, 3) at seed 1: one live channel, 1.6e-5) no fp32 sum in any order is good to 1e-5.
A case on which a plain fp32 evaluation of the reference's own formulas misses the tolerance says
nothing about a kernel. The clause only rejects seeds; no tolerance is widened by it. The search is bounded by SEED_BOUND; a set that meets
no seed is shrunk, never the guard (no case needed it: `cifar`, with 4 064 pre-activations a sample,
three models and one batch of three samples, meets the rule at seed 1). test_lenet_hidden_host.py
derives every seed again.

`plan` restates the launch plan of cfa_lenet_global.h for this family from the geometry, the batch and the LDS
limit alone, and `path` names the arithmetic that puts a case on the loop, tail or branch it exists for."""
import numpy as np

import lenet_cases as lc
import lenet_grad_cases as gc
import lenet_huber_cases as hc

CIFAR_LENET = (32, 3, 5, 4, 8, 128, 10)
GUARD = gc.GUARD
CONDITION = 1e-5  # the tests' own tolerance: numpy's fp32 evaluation of the restatement has to meet it too
SEED_BOUND = 400  # seeds tried before a case's set would have to shrink
LOSSES = ("xent", "huber")

# name: (geometry, batch, Nt, D, seed)
CASES = {
    "cin3_map1": ((12, 3, 3, 2, 3, 5, 4), 3, 7, 3, 2),      # three channels, a 1 x 1 final map, hidden 5; chunks of 2 and 1
    "cin1_hidden": ((12, 1, 3, 2, 3, 6, 4), 3, 7, 3, 1),    # one channel, with its axis present in x
    "pool1_drops": ((14, 2, 4, 3, 5, 4, 3), 3, 7, 3, 1),    # conv1 output 11: the first pool drops; runtime k
    "pool2_drops": ((12, 2, 3, 2, 3, 4, 4), 3, 7, 3, 0),    # conv2 output 3: the second pool drops
    "generic_k": ((20, 2, 4, 3, 4, 6, 5), 5, 11, 3, 6),     # k = 4, both pools drop, a 2 x 2 final map
    "k5": ((16, 3, 5, 2, 3, 7, 3), 3, 7, 3, 2),             # the compile-time k = 5 kernels
    "hidden_1": ((12, 3, 3, 2, 3, 1, 4), 3, 7, 3, 36),       # one hidden unit: 16 slices of one column, one dflat lane
    "hidden_wide": ((12, 3, 3, 2, 3, 520, 4), 3, 7, 3, 1),  # hidden above the 512 threads: a second column pass
    "two_groups": ((12, 3, 3, 2, 3, 5, 4), 9, 10, 3, 0),    # a full group of 8 samples (four chunks) and a group of 1
    "finish_256": ((10, 2, 3, 3, 3, 16, 3), 3, 7, 3, 2),    # P + 1 = 257: a second finish block of one live thread
    "odd_side": ((13, 3, 3, 2, 3, 5, 4), 3, 7, 3, 1),       # an image of 507 floats: odd offsets of samples and LDS arrays
    "cifar": (CIFAR_LENET, 3, 3, 3, 1),                     # the driver geometry: chunks of 2 and 1 samples
}
SMALL = tuple(n for n in CASES if n != "cifar")
# validation only (costs take no discrete decision that a 1e-5 comparison could see): name: (geometry,
# batch, batches, Nt, D)
EVAL_CASES = {
    "chunk_tail_2": ((12, 3, 3, 2, 3, 5, 4), 6, 2, 13, 3),   # chunks of 4 and 2 samples, two batches
    "cifar_tail": (CIFAR_LENET, 4, 1, 5, 2),                 # the driver geometry: chunks of 3 and 1
    "raised_lds": ((76, 3, 3, 1, 1, 2, 3), 2, 1, 3, 2),      # one sample's state above 64 KiB
}

# cfa_lenet_global.h: kGlobalBlock, kGlobalEvalChunk, kGlobalGradChunk, kGlobalGroup
BLOCK, EVAL_CHUNK, GRAD_CHUNK, GROUP = 512, 4, 2, 8
LDS_LIMIT = 160 * 1024
# a geometry whose ONE-sample gradient state is beyond the device's LDS (from grad_lds_bytes, not by
# trial): the image alone is 120 * 120 * 3 floats = 172 800 bytes
TOO_LARGE = (120, 3, 3, 1, 1, 2, 3)


def stages(geom):
    side, cin, k, c1, c2, hidden, classes = geom
    return lc.stages((side, k, c1, c2, classes))


def layer_shapes(geom):
    side, cin, k, c1, c2, hidden, classes = geom
    p2 = stages(geom)[3]
    return [(k, k, cin, c1), (c1,), (k, k, c1, c2), (c2,), (p2 * p2 * c2, hidden), (hidden,), (hidden, classes),
            (classes,)]


def size(geom):
    return sum(int(np.prod(s)) for s in layer_shapes(geom))


def split(row, geom):
    """The eight tensors of a model row."""
    out, o = [], 0
    for s in layer_shapes(geom):
        n = int(np.prod(s))
        out.append(np.asarray(row[o:o + n]).reshape(s))
        o += n
    assert o == len(row)
    return out


def tensors(vec, geom):
    """The eight tensors of a gradient row, flat, for a per-tensor comparison."""
    return [np.asarray(t).reshape(-1) for t in split(vec, geom)]


# ---- the launch plan ------------------------------------------------------------------------

def hidden_cols(H, T=BLOCK):
    return min(H, T)


def hidden_slices(H, T=BLOCK):
    """lenet_hidden_slices: the slices that share a column's sum over i."""
    S = 1
    while S < 16 and 2 * S * hidden_cols(H, T) <= T:
        S *= 2
    return S


def hidden_lanes(H):
    """lenet_hidden_lanes: the lanes that share one dflat sum over j."""
    L = 1
    while L < 64 and L < H:
        L *= 2
    return L


def part_floats(H, n):
    return hidden_slices(H) * n * hidden_cols(H)


def sample_floats(geom):
    side, cin, k, c1, c2, hidden, classes = geom
    _, p1, _, p2 = stages(geom)
    return side * side * cin + p1 * p1 * c1 + p2 * p2 * c2 + hidden + classes


def eval_lds_bytes(geom, n, batch):
    return 4 * (n * sample_floats(geom) + part_floats(geom[5], n) + batch)


def eval_chunk(geom, batch, lds_limit=LDS_LIMIT):
    for n in range(EVAL_CHUNK, 0, -1):
        if eval_lds_bytes(geom, n, batch) <= lc.LDS_DEFAULT:
            return n
    return 1 if eval_lds_bytes(geom, 1, batch) <= lds_limit else 0


def grad_lds_bytes(geom, n):
    side, cin, k, c1, c2, hidden, classes = geom
    _, p1, _, p2 = stages(geom)
    n1, flat = p1 * p1 * c1, p2 * p2 * c2
    sample = side * side * cin + 2 * n1 + 2 * flat + 2 * hidden + 2 * classes + 4 * flat
    return 4 * (n * sample + part_floats(hidden, n) + c1 * (c2 + 1) + GROUP + n + (n * (n1 + flat) + 3) // 4)


def grad_chunk(geom, lds_limit=LDS_LIMIT):
    for n in range(GRAD_CHUNK, 0, -1):
        if grad_lds_bytes(geom, n) <= lc.LDS_DEFAULT:
            return n
    return 1 if grad_lds_bytes(geom, 1) <= lds_limit else 0


def grad_workspace_bytes(geom, batch, D):
    return 4 * D * ((batch + GROUP - 1) // GROUP) * (size(geom) + GROUP)


def plan(geom, batch, lds_limit=LDS_LIMIT):
    side, cin, k, c1, c2, hidden, classes = geom
    ec, gcn = eval_chunk(geom, batch, lds_limit), grad_chunk(geom, lds_limit)
    groups = (batch + GROUP - 1) // GROUP
    last = batch - GROUP * (groups - 1)
    return {"fast": k == 5, "s": stages(geom), "eval_chunk": ec, "eval_tail": batch % ec if ec else None,
            "eval_lds": eval_lds_bytes(geom, ec, batch) if ec else None,
            "grad_chunk": gcn, "grad_lds": grad_lds_bytes(geom, gcn) if gcn else None,
            "groups": groups, "last": last, "cols": hidden_cols(hidden), "slices": hidden_slices(hidden),
            "col_passes": -(-hidden // hidden_cols(hidden)), "lanes": hidden_lanes(hidden),
            "finish_blocks": -(-(size(geom) + 1) // 256)}


def path(name, lds_limit=LDS_LIMIT):
    """The conditions that put the case `name` on the path it exists for, {text: bool}."""
    geom, batch = (CASES.get(name) or EVAL_CASES[name])[:2]
    side, cin, k, c1, c2, hidden, classes = geom
    p, P = plan(geom, batch, lds_limit), size(geom)
    s1, p1, s2, p2 = p["s"]
    if name == "cin3_map1":
        return {"three input channels": cin == 3, "a 1 x 1 final map, flat = 3": p2 == 1 and p2 * p2 * c2 == 3,
                "hidden 5: 16 slices of 5 columns, 8 dflat lanes of which 3 have no j":
                    (p["slices"], p["cols"], p["lanes"]) == (16, 5, 8),
                "gradient chunks of 2 and 1": p["grad_chunk"] == 2 and batch == 3,
                "the runtime-k kernels": not p["fast"]}
    if name == "cin1_hidden":
        return {"one channel": cin == 1}
    if name == "pool1_drops":
        return {"the first pool drops": s1 % 2 == 1, "the runtime-k kernels at k = 4": k == 4 and not p["fast"],
                "two channels": cin == 2}
    if name == "pool2_drops":
        return {"the second pool drops": s2 % 2 == 1 and s1 % 2 == 0, "two channels": cin == 2}
    if name == "generic_k":
        return {"k = 4": k == 4 and not p["fast"], "both pools drop": s1 % 2 == 1 and s2 % 2 == 1,
                "a 2 x 2 final map": p2 == 2, "two channels": cin == 2,
                "validation chunks of 4 and 1": p["eval_chunk"] == 4 and p["eval_tail"] == 1,
                "gradient chunks of 2, 2 and 1 in one group": (p["grad_chunk"], p["groups"], batch) == (2, 1, 5)}
    if name == "k5":
        return {"the k = 5 kernels": p["fast"], "three channels": cin == 3, "16 -> 12 -> 6 -> 2 -> 1": p["s"] == (12, 6, 2, 1)}
    if name == "hidden_1":
        return {"one column, 16 slices, one dflat lane": (p["cols"], p["slices"], p["lanes"]) == (1, 16, 1)}
    if name == "hidden_wide":
        return {"hidden 520 above the workgroup's 512 threads: one slice, a second column pass of 8":
                    hidden > BLOCK and (p["cols"], p["slices"], p["col_passes"]) == (BLOCK, 1, 2)
                    and hidden - BLOCK == 8,
                "64 dflat lanes, each more than 8 columns": p["lanes"] == 64}
    if name == "two_groups":
        return {"a full group of four chunks, then a group of one sample":
                    (p["groups"], p["last"], p["grad_chunk"]) == (2, 1, 2) and batch == GROUP + 1,
                "validation chunks of 4, 4 and 1": p["eval_chunk"] == 4 and batch == 9}
    if name == "finish_256":
        return {"P + 1 = 257: 2 finish blocks": (P + 1, p["finish_blocks"]) == (257, 2)}
    if name == "odd_side":
        nx, n1 = side * side * cin, p1 * p1 * c1
        return {"an odd side with three channels: an image of 507 floats": (side % 2, cin, nx) == (1, 3, 507),
                "the second sample of a chunk and the first pooled map start at odd float offsets":
                    nx % 2 == 1 and (p["grad_chunk"] * nx) % 4 != 0,
                "the first pool drops": s1 % 2 == 1}
    if name == "cifar":
        return {"P = 28 130": P == 28130, "32 -> 28 -> 14 -> 10 -> 5": p["s"] == (28, 14, 10, 5),
                "the k = 5 kernels": p["fast"],
                "128 columns in 4 slices, 64 dflat lanes": (p["cols"], p["slices"], p["lanes"]) == (128, 4, 64),
                "2 samples a gradient chunk: 55 176 bytes of LDS, within the default":
                    (p["grad_chunk"], p["grad_lds"]) == (2, 55176) and p["grad_lds"] <= lc.LDS_DEFAULT}
    if name == "chunk_tail_2":
        return {"validation chunks of 4 and 2": (p["eval_chunk"], p["eval_tail"]) == (4, 2)}
    if name == "cifar_tail":
        return {"validation chunks of 3 and 1": (p["eval_chunk"], p["eval_tail"]) == (3, 1),
                "56 872 bytes at the driver's batch of 100": eval_lds_bytes(geom, 3, 100) == 56872
                and eval_lds_bytes(geom, 4, 100) > lc.LDS_DEFAULT}
    if name == "raised_lds":
        return {"one sample a chunk": p["eval_chunk"] == 1, "above the default limit": p["eval_lds"] > lc.LDS_DEFAULT,
                "within the device's": p["eval_lds"] <= lds_limit}
    raise KeyError(name)


# ---- the restatement ------------------------------------------------------------------------

def _forward(x, row, geom, dtype=np.float64):
    """x [n, side, side, channels] -> (h0, z1, a1, z2, a2, zh): inputs, both convolutions' and the
    hidden layer's pre-activations, both pooled maps."""
    conv = lc.conv_valid if dtype == np.float64 else gc._conv32
    K1, b1, K2, b2, Wh, bh, Wd, bd = (t.astype(dtype) for t in split(row, geom))
    h0 = np.asarray(x, dtype=dtype)
    z1 = conv(h0, K1, b1)
    a1 = lc.avg_pool(np.maximum(z1, 0)).astype(dtype)
    z2 = conv(a1, K2, b2)
    a2 = lc.avg_pool(np.maximum(z2, 0)).astype(dtype)
    zh = a2.reshape(a2.shape[0], -1) @ Wh + bh
    return h0, z1, a1, z2, a2, zh


def log_probs(x, row, geom):
    """fp64 log softmax of the model `row` on images x [n, side, side, channels]: [n, classes]."""
    zh = _forward(x, row, geom)[5]
    Wd, bd = (t.astype(np.float64) for t in split(row, geom)[6:])
    z = np.maximum(zh, 0) @ Wd + bd
    z = z - z.max(axis=1, keepdims=True)
    return z - np.log(np.exp(z).sum(axis=1, keepdims=True))


def sample_losses(x, labels, row, geom, loss="xent"):
    lp = log_probs(x, row, geom)
    n = len(labels)
    if loss == "huber":
        return hc.huber(np.exp(lp)[np.arange(n), labels], labels)[0]
    return -lp[np.arange(n), labels]


def loss_of(x, labels, row, geom, loss="xent"):
    return float(sample_losses(x, labels, row, geom, loss).mean())


def grads(x, labels, row, geom, loss="xent", dtype=np.float64):
    """fp64 (gradient [P], the eight tensors flattened in row order; batch-mean loss) of the model
    `row` on the batch x [n, side, side, channels] / labels [n], for the objective `loss`. With
    dtype = np.float32 the forward pass and every product of the backward pass are numpy fp32 (the
    seed rule's measure of how well a tensor's sums are conditioned; not a reference)."""
    K1, b1, K2, b2, Wh, bh, Wd, bd = (t.astype(dtype) for t in split(row, geom))
    h0, z1, a1, z2, a2, zh = _forward(x, row, geom, dtype)
    n = h0.shape[0]
    flat, h = a2.reshape(n, -1), np.maximum(zh, 0)
    z = h @ Wd + bd
    z = z - z.max(axis=1, keepdims=True)
    lp = z - np.log(np.exp(z).sum(axis=1, keepdims=True))
    sm = np.exp(lp)
    onehot = np.zeros_like(sm)
    onehot[np.arange(n), labels] = 1.0
    if loss == "huber":
        p = sm[np.arange(n), labels]
        hub, g = hc.huber(p, labels)
        dz, value = ((g * p)[:, None] * (onehot - sm)).astype(dtype), float(hub.mean())
    else:
        dz, value = sm - onehot, float(-lp[np.arange(n), labels].mean())
    dWd, dbd = h.T @ dz, dz.sum(axis=0)
    dh = (dz @ Wd.T) * (zh > 0)
    dWh, dbh, dflat = flat.T @ dh, dh.sum(axis=0), dh @ Wh.T
    dz2 = (gc._unpool(dflat.reshape(a2.shape), z2.shape) * (z2 > 0)).astype(dtype)
    dK2, db2, da1 = gc._conv_backward(a1, K2, dz2, True)
    dz1 = (gc._unpool(da1.astype(dtype), z1.shape) * (z1 > 0)).astype(dtype)
    dK1, db1, _ = gc._conv_backward(h0, K1, dz1, False)
    out = np.concatenate([t.reshape(-1) for t in (dK1, db1, dK2, db2, dWh, dbh, dWd, dbd)]) / n
    return out, value


# ---- the seed rule --------------------------------------------------------------------------

def make(geom, D, Nt, seed=0):
    """(x [Nt, side, side, channels] fp32, labels [Nt] int32, models [D, P] fp32), seeded: images
    rng.random in [0, 1), weights 0.1 * standard_normal, labels uniform, as lenet_cases.make."""
    rng = np.random.default_rng(seed)
    x = rng.random((Nt, geom[0], geom[0], geom[1])).astype(np.float32)
    labels = rng.integers(0, geom[6], Nt).astype(np.int32)
    models = (0.1 * rng.standard_normal((D, size(geom)))).astype(np.float32)
    return x, labels, models


def decisions(x, row, geom):
    """(smallest |pre-activation|, largest, largest |fp32 - fp64| pre-activation) over both
    convolutions and the hidden layer, every sample of x."""
    f64, f32 = _forward(x, row, geom), _forward(x, row, geom, np.float32)
    a = np.concatenate([np.abs(f64[i]).reshape(-1) for i in (1, 3, 5)])
    shift = max(np.abs(f64[i] - f32[i]).max() for i in (1, 3, 5))
    return float(a.min()), float(a.max()), float(shift)


def meets_the_seed_rule(geom, batch, Nt, D, seed):
    x, labels, models = make(geom, D, Nt, seed)
    for row in models:
        lo, hi, shift = decisions(x, row, geom)
        if not (lo >= GUARD * hi and shift <= 0.1 * lo):
            return False
        for first in range(Nt if Nt > batch else 1):
            idx = (np.arange(batch) + first) % Nt
            for loss in LOSSES:
                g64 = tensors(grads(x[idx], labels[idx], row, geom, loss)[0], geom)
                if not all(np.abs(t).max() > 0 for t in g64):
                    return False
                g32 = tensors(grads(x[idx], labels[idx], row, geom, loss, np.float32)[0], geom)
                if not all(np.abs(a - b).max() <= CONDITION * np.abs(b).max() for a, b in zip(g32, g64)):
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
    """(x [Nt, side, side, channels] fp32, labels [Nt] int32, models [D, P] fp32) of a case."""
    if name not in _DATA:
        if name in CASES:
            geom, _, Nt, D, seed = CASES[name]
        else:
            (geom, _, _, Nt, D), seed = EVAL_CASES[name], 0
        _DATA[name] = make(geom, D, Nt, seed)
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


# ---- the drivers' epoch, restated: validate, local Adam updates, an ended-aware round --------------

# lr 3e-2: with 7 samples and two batches an epoch the costs have to fall between epochs, or no target
# lets the first epoch pass without a flag and the second raise one. margin: every cost the run compares
# with the target lies at least this far from it, relatively: ten times the 1e-5 the costs are held to.
EPOCHS = {"case": "cin3_map1", "epochs": 3, "val_batches": 2, "steps": 2, "lr": 3e-2, "clipnorm": 1.0,
          "margin": 1e-4}


def adam_clipnorm(w, g, m, v, t, geom, lr, clip, b1=0.9, b2=0.999, eps=1e-7):
    """One Keras Adam step in fp64 after tf.clip_by_norm per layer: (w, m, v) after step t (1-based)."""
    g, o = g.copy(), 0
    for shape in layer_shapes(geom):
        n = int(np.prod(shape))
        norm = np.sqrt((g[o:o + n] ** 2).sum())
        g[o:o + n] *= clip / max(norm, clip)
        o += n
    m = m + (g - m) * (1 - b1)
    v = v + (g * g - v) * (1 - b2)
    lr_t = lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)
    return w - lr_t * m / (np.sqrt(v) + eps), m, v


def tf2_round(rows, flags, lists):
    """One consensus round of the TF2 drivers with the training_end rule "copy" (consensus_v3.py:144-159),
    every device on the previous rows and flags: an ended device keeps its row; a device that meets an
    ended neighbour takes that neighbour's row (its list is read up to the first one); every other
    device runs w <- w + eps (x_q - w) over its neighbours in order, eps = 1 / (neighbours + 1)."""
    out = rows.copy()
    for d, nbr in enumerate(lists):
        if flags[d]:
            continue
        first = next((j for j in nbr if flags[j]), None)
        if first is not None:
            out[d] = rows[first]
            continue
        w, eps = rows[d].copy(), 1.0 / (len(nbr) + 1)
        for j in nbr:
            w = w + eps * (rows[j] - w)
        out[d] = w
    return out


def drivers_epochs(loss, target):
    """EPOCHS restated in fp64 on the case's per-device sets (device d: the shared set rolled by d), a
    ring, no device ended at the start. An epoch: the validation cost of every live device over the
    first val_batches batches of its set and ended |= cost < target; `steps` local batches (gradient
    at the device's cursor, Adam with clipnorm, cursor + batch mod Nt) for every device still live;
    one tf2_round. Returns (models, cost, ended, history), history[e] = (costs validated in epoch e
    with NaN for a skipped device, flags after that validation, steps taken so far)."""
    name = EPOCHS["case"]
    geom, batch, Nt, D, _ = CASES[name]
    xs, ls = per_device(name)
    w = data(name)[2].astype(np.float64)
    m, v = np.zeros_like(w), np.zeros_like(w)
    t, cursor = np.zeros(D, dtype=np.int64), np.zeros(D, dtype=np.int64)
    ended, cost = np.zeros(D, dtype=np.int32), np.zeros(D)
    lists = [[(d - 1) % D, (d + 1) % D] for d in range(D)]
    n, history = batch * EPOCHS["val_batches"], []
    for _ in range(EPOCHS["epochs"]):
        seen = np.full(D, np.nan)
        for d in range(D):
            if not ended[d]:
                per = sample_losses(xs[d][:n], ls[d][:n], w[d], geom, loss)
                seen[d] = cost[d] = per.reshape(EPOCHS["val_batches"], batch).mean(axis=1).mean()
        ended = ended | (np.nan_to_num(seen, nan=np.inf) < target).astype(np.int32)
        for _ in range(EPOCHS["steps"]):
            for d in range(D):
                if ended[d]:
                    continue
                idx = (np.arange(batch) + cursor[d]) % Nt
                g = grads(xs[d][idx], ls[d][idx], w[d], geom, loss)[0]
                t[d] += 1
                w[d], m[d], v[d] = adam_clipnorm(w[d], g, m[d], v[d], t[d], geom, EPOCHS["lr"], EPOCHS["clipnorm"])
                cursor[d] = (cursor[d] + batch) % Nt
        history.append((seen, ended.copy(), t.copy()))
        w = tf2_round(w, ended, lists)
    return w, cost, ended, history


def epochs_target(loss):
    """The target of the EPOCHS run, from the restatement alone, in a run that never ends (target
    -inf): halfway between the smallest cost the SECOND epoch's validation sees and the smaller of that
    epoch's second smallest and the first epoch's smallest. So the first epoch (local updates and an
    eps-mix of all three rows) raises no flag and the second raises exactly one, in the middle of the
    sequence: its neighbours copy its row in that epoch's round and validate the copy in the third."""
    history = drivers_epochs(loss, -np.inf)[3]
    first, second = np.sort(history[0][0]), np.sort(history[1][0])
    return float(0.5 * (second[0] + min(second[1], first[0])))
