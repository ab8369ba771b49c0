"""The cases of tests/test_lenet_training_host.py and tests/test_gpu_lenet_training.py: the LeNet-1
family's backward pass restated in numpy fp64 from the layer definitions, on top of the forward
restatement of tests/lenet_cases.py (no torch here), the case table and the seeded data.

Per sample with label l: dz = softmax(z) - onehot(l); dWd = flat (x) dz, dbd = dz, dflat = Wd dz;
the average pool hands 0.25 of a pooled element's gradient to each of its four positions and 0 to
a row or column it dropped; relu passes where its input is > 0; a convolution (cross-correlation,
kernel (kh, kw, in, out), NHWC) has dK[i, j] = sum_{y,x} in[y+i, x+j] (x) dzc[y, x],
db = sum_{y,x} dzc[y, x] and din[y+i, x+j] += K[i, j] dzc[y, x]. The batch's gradient is the mean.

A relu gate that differs between an fp32 and this fp64 evaluation moves a bias gradient by a whole
term, far above the 1e-5 tolerance, so a case's seed is chosen (here, from the restatement alone)
such that over EVERY model and EVERY sample of its set the smallest |pre-activation| of both
convolutions stays above 1e-5 of the largest (`margin`); an fp32 evaluation moves a
pre-activation by about 3e-7 of the largest (test_lenet_training_host.py holds it to a tenth of
the margin). Whatever batch, `first`, `src` or per-device set a test picks stays inside that.

PATHS names the cases that exist for a loop, a lane plan or a branch of cfa_lenet_grad.hip and
cfa_lenet_graph.h the others never take. `plan` restates the launch plan from the geometry and the
batch alone, and `path` gives the arithmetic that puts a case on its path as named conditions that
the tests assert. A PATHS case's seed is the smallest that meets the margin rule and under which no
model has a tensor whose gradient is all zero on any batch of the set (with one or two channels a
model's relus are often all shut, and a comparison relative to a zero tensor says nothing);
test_lenet_training_host.py derives it again."""
import numpy as np

import lenet_cases as lc

D = 3
# name: (geometry, batch, Nt, seed). The library cuts a batch into groups of 4 samples (one
# workgroup each) and a group into chunks of 2.
CASES = {
    "lenet1": (lc.LENET1, 6, 13, 3),               # a full group and a second of one chunk; the K = 5 kernel
    "pool2_drops": ((12, 3, 2, 3, 4), 3, 7, 0),    # the second pool drops a row and column; a partial chunk
    "pool1_drops": ((14, 4, 3, 5, 3), 3, 7, 0),    # the first pool drops a row and column
    "map_1x1": ((13, 4, 3, 5, 3), 3, 7, 0),        # a 1 x 1 final map
    "generic_k": ((16, 3, 3, 4, 5), 5, 11, 1),     # the runtime-k kernel, two groups, the second a partial chunk
    # the paths no case above takes (PATHS, path()); a seed is the smallest that meets the margin rule and
    # leaves no tensor's gradient all zero (a model whose relus are all shut: seeds 0 to 33 of lanes_64)
    "k5_drops": ((23, 5, 4, 13, 17), 9, 13, 1),       # 23 -> 19 -> 9 -> 5 -> 2: the K = 5 kernel where both pools
                                                      # drop, 260 items, 272 logit lanes, groups of 4, 4 and 1
    "generic_items": ((12, 3, 8, 11, 4), 3, 7, 1),    # the runtime-k kernel with 264 items
    "lanes_64": ((10, 3, 1, 1, 2), 3, 7, 34),         # 3 items, 1 channel: 64 lanes a sum, fewer rows than lanes
    "classes_64": ((12, 3, 2, 3, 64), 3, 7, 0),       # the entry's most classes: 1 024 logit lanes
    "classes_33": ((12, 3, 2, 3, 33), 3, 7, 1),       # 528 logit lanes: a third pass of 16
    "finish_255": ((10, 3, 4, 5, 5), 3, 7, 0),        # P + 1 = 256: the loss is the finish block's last thread
    "finish_256": ((14, 3, 4, 4, 4), 3, 7, 2),        # P + 1 = 257: a second finish block of one live thread
    "raised_lds": ((20, 3, 8, 32, 40), 3, 4, 1),      # P = 13 976: 141 736 bytes of LDS, above the default 64 KiB
}
PATHS = ("k5_drops", "generic_items", "lanes_64", "classes_64", "classes_33", "finish_255", "finish_256",
         "raised_lds")
GUARD = 1e-5
# cfa_lenet_grad.hip: kGradBlockL, kGradChunk, kGradGroup
BLOCK, CHUNK, GROUP = 256, 2, 4


def lanes(items, T=BLOCK):
    """lenet_lanes: the lanes that share one of `items` sums."""
    L = 1
    while L < 64 and 2 * L * items <= T:
        L *= 2
    return L


def grad_lds_bytes(geom):
    """lenet_grad_lds: model and gradient sums, a chunk's activations and their gradients, a group's
    losses, a chunk's labels, the gate bytes."""
    side, k, c1, c2, classes = geom
    _, p1, _, p2 = lc.stages(geom)
    n1, flat = p1 * p1 * c1, p2 * p2 * c2
    sample = side * side + 2 * n1 + 2 * flat + 2 * classes + 4 * flat
    return 4 * (2 * lc.size(geom) + CHUNK * sample + GROUP + CHUNK + (CHUNK * (n1 + flat) + 3) // 4)


def plan(name):
    """What the launch of a case looks like from the geometry and the batch alone: the kernel, the
    items, lanes and rows (of a one-sample chunk) of both weight gradients, the lanes of both bias
    gradients, the lanes of lenet_logits for a full chunk, the groups and the LDS."""
    geom, batch, _, _ = CASES[name]
    side, k, c1, c2, classes = geom
    s1, p1, s2, p2 = lc.stages(geom)
    groups = (batch + GROUP - 1) // GROUP
    return {"fast": k == 5, "s": (s1, p1, s2, p2), "items": (k * c1, k * c1 * c2),
            "L": (lanes(k * c1), lanes(k * c1 * c2)), "rows": (2 * p1, 2 * p2), "Lb": (lanes(c1), lanes(c2)),
            "logit_lanes": min(CHUNK, batch) * classes * 8, "groups": groups, "last": batch - GROUP * (groups - 1),
            "lds": grad_lds_bytes(geom), "finish_blocks": (lc.size(geom) + 1 + BLOCK - 1) // BLOCK}


def path(name, lds_limit=160 * 1024):
    """The conditions that put the PATHS case `name` on its path, {text: bool}; `lds_limit` is the
    device's LDS per workgroup."""
    p, P = plan(name), lc.size(CASES[name][0])
    if name == "k5_drops":
        return {"the K = 5 kernel": p["fast"],
                "both pools drop a row and column": p["s"][0] % 2 == 1 and p["s"][2] % 2 == 1,
                "stage 2: 5 * 4 * 13 = 260 items > 256, one lane each, a second pass of `idx += T`":
                    p["items"][1] == 260 > BLOCK and p["L"][1] == 1,
                "lenet_logits: 2 * 17 * 8 = 272 lanes > 256, a second pass of 16": p["logit_lanes"] == 272,
                "three groups, the last of one sample": (p["groups"], p["last"]) == (3, 1), "P = 2 318": P == 2318}
    if name == "generic_items":
        return {"the runtime-k kernel": not p["fast"],
                "stage 2: 3 * 8 * 11 = 264 items > 256, one lane each, a second pass":
                    p["items"][1] == 264 > BLOCK and p["L"][1] == 1}
    if name == "lanes_64":
        return {"3 items per stage: 64 lanes a sum": p["items"] == (3, 3) and p["L"] == (64, 64),
                "one channel per stage: 64 lanes a bias sum": p["Lb"] == (64, 64),
                "a one-sample chunk has 8 and 2 rows, a full one 16 and 4: lanes without a row": p["rows"] == (8, 2),
                "a one-sample chunk occurs": CASES[name][1] % CHUNK == 1}
    if name in ("classes_64", "classes_33"):
        C = CASES[name][0][4]
        last = 16 * C % BLOCK or BLOCK
        return {"lenet_logits: 2 * C * 8 = %d lanes, passes of 256 and a last one of %d" % (16 * C, last):
                    p["logit_lanes"] == 16 * C > BLOCK,
                "the entry's most classes, or a last pass below a wave": C == 64 or last < 64}
    if name in ("finish_255", "finish_256"):
        return {"P + 1 = %d: %d finish blocks" % (P + 1, p["finish_blocks"]):
                    (P + 1, p["finish_blocks"]) == ((256, 1) if name == "finish_255" else (257, 2))}
    if name == "raised_lds":
        return {"141 736 bytes of LDS": p["lds"] == 141736, "above the default limit": p["lds"] > lc.LDS_DEFAULT,
                "within the device's": p["lds"] <= lds_limit}
    raise KeyError(name)


def _conv32(h, K, b):
    """lc.conv_valid with every product and sum in fp32."""
    k, so = K.shape[0], h.shape[1] - K.shape[0] + 1
    out = np.zeros((h.shape[0], so, so, K.shape[3]), dtype=np.float32)
    for i in range(k):
        for j in range(k):
            out += np.einsum("nyxc,co->nyxo", h[:, i:i + so, j:j + so, :], K[i, j])
    return out + b


def _forward(x, row, geom, dtype=np.float64):
    conv = lc.conv_valid if dtype == np.float64 else _conv32
    K1, b1, K2, b2, Wd, bd = (t.astype(dtype) for t in lc.split(row, geom))
    h0 = np.asarray(x, dtype=dtype)[..., None]
    z1 = conv(h0, K1, b1)
    a1 = lc.avg_pool(np.maximum(z1, 0)).astype(dtype)
    z2 = conv(a1, K2, b2)
    a2 = lc.avg_pool(np.maximum(z2, 0)).astype(dtype)
    return h0, z1, a1, z2, a2


def _unpool(d, shape):
    """The average pool's backward: 0.25 d to each window position, 0 where the pool dropped."""
    out = np.zeros(shape)
    p = d.shape[1]
    out[:, :2 * p, :2 * p, :] = 0.25 * np.repeat(np.repeat(d, 2, axis=1), 2, axis=2)
    return out


def _conv_backward(h, K, dz, want_input):
    k, so = K.shape[0], dz.shape[1]
    dK, dh = np.zeros(K.shape), np.zeros(h.shape) if want_input else None
    for i in range(k):
        for j in range(k):
            dK[i, j] = np.einsum("nyxc,nyxo->co", h[:, i:i + so, j:j + so, :], dz)
            if want_input:
                dh[:, i:i + so, j:j + so, :] += np.einsum("nyxo,co->nyxc", dz, K[i, j])
    return dK, dz.sum(axis=(0, 1, 2)), dh


def grads(x, labels, row, geom):
    """fp64 (gradient [P], the six tensors flattened in row order; batch-mean loss) of the model
    `row` on the batch x [n, side, side] / labels [n]."""
    K1, b1, K2, b2, Wd, bd = (t.astype(np.float64) for t in lc.split(row, geom))
    h0, z1, a1, z2, a2 = _forward(x, row, geom)
    n = h0.shape[0]
    flat = a2.reshape(n, -1)
    z = flat @ Wd + bd
    z = z - z.max(axis=1, keepdims=True)
    lp = z - np.log(np.exp(z).sum(axis=1, keepdims=True))
    dz = np.exp(lp)
    dz[np.arange(n), labels] -= 1.0
    dWd, dbd, dflat = flat.T @ dz, dz.sum(axis=0), dz @ Wd.T
    dz2 = _unpool(dflat.reshape(a2.shape), z2.shape) * (z2 > 0)
    dK2, db2, da1 = _conv_backward(a1, K2, dz2, True)
    dz1 = _unpool(da1, z1.shape) * (z1 > 0)
    dK1, db1, _ = _conv_backward(h0, K1, dz1, False)
    g = np.concatenate([t.reshape(-1) for t in (dK1, db1, dK2, db2, dWd, dbd)]) / n
    return g, float(-lp[np.arange(n), labels].mean())


def margin(x, row, geom):
    """(smallest, largest) |pre-activation| over both convolutions, fp64."""
    _, z1, _, z2, _ = _forward(x, row, geom)
    a = np.concatenate([np.abs(z1).reshape(-1), np.abs(z2).reshape(-1)])
    return float(a.min()), float(a.max())


def preactivation_shift(x, row, geom):
    """Largest |fp32 - fp64| pre-activation of both convolutions (a numpy fp32 evaluation)."""
    _, a1, _, a2, _ = _forward(x, row, geom)
    _, b1, _, b2, _ = _forward(x, row, geom, np.float32)
    return float(max(np.abs(a1 - b1).max(), np.abs(a2 - b2).max()))


def meets_the_seed_rule(geom, batch, Nt, seed):
    """A PATHS case's rule for a seed: the margin rule over every model and sample of the set, and no
    tensor's gradient all zero for any model on any batch of the set."""
    x, labels, models = lc.make(geom, D, Nt, seed)
    for row in models:
        lo, hi = margin(x, row, geom)
        if not (lo >= GUARD * hi and preactivation_shift(x, row, geom) <= 0.1 * lo):
            return False
        for first in range(Nt):
            idx = (np.arange(batch) + first) % Nt
            if not all(np.abs(t).max() > 0 for t in tensors(grads(x[idx], labels[idx], row, geom)[0], geom)):
                return False
    return True


def tensors(vec, geom):
    """The six tensors of a gradient row, flat, for a per-tensor comparison."""
    return [np.asarray(t).reshape(-1) for t in lc.split(vec, geom)]


_DATA, _REF = {}, {}


def data(name):
    """(x [Nt, side, side] fp32, labels [Nt] int32, models [D, P] fp32) of a case: read only."""
    if name not in _DATA:
        geom, _, Nt, seed = CASES[name]
        _DATA[name] = lc.make(geom, D, Nt, seed)
        for a in _DATA[name]:
            a.setflags(write=False)
    return _DATA[name]


def per_device(name):
    """One set per device from the case's own samples: device d's set is the shared one rolled by
    d samples, (x [D, Nt, side, side], labels [D, Nt])."""
    x, labels, _ = data(name)
    return np.stack([np.roll(x, -d, axis=0) for d in range(D)]), np.stack([np.roll(labels, -d) for d in range(D)])


def reference(name, model, first=0, shift=0):
    """fp64 (gradient, loss) of model row `model` on the case's batch that starts at sample
    `first` (wrapping) of the shared set rolled by `shift`; computed once per key and shared."""
    key = (name, model, first, shift)
    if key not in _REF:
        geom, batch, Nt, _ = CASES[name]
        x, labels, models = data(name)
        idx = (np.arange(batch) + first + shift) % Nt
        g, loss = grads(x[idx], labels[idx], models[model], geom)
        g.setflags(write=False)
        _REF[key] = (g, loss)
    return _REF[key]
