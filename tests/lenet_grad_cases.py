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
the margin). Whatever batch, `first`, `src` or per-device set a test picks stays inside that."""
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
}
GUARD = 1e-5


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
