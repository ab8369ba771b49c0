"""The cases of tests/test_lenet_validation_host.py and tests/test_gpu_lenet_validation.py: the
LeNet-1 family's forward pass, validation cost and flag rule restated in numpy fp64 from the layer
definitions (no torch here), the geometry table and the seeded data.

The family, geometry (side, kernel, c1, c2, classes), Keras semantics: input [side, side, 1];
Conv2D(c1, k x k, valid, relu), a cross-correlation with the kernel tensor (kh, kw, in, out);
AveragePooling2D(2 x 2, stride 2, valid), which drops an odd last row and column; Conv2D(c2);
AveragePooling2D; Flatten in NHWC order; Dense(classes, softmax). A model row is get_weights()
order, C-order: K1 b1 K2 b2 Wd bd.

Data: images rng.random in [0, 1), weights 0.1 * standard_normal, labels uniform. With it every
class probability stays above 0.07 and the costs lie between 1 and 2.4, far from the region where
a probability underflows in fp32 (there the library's log-softmax and the reference's log of the
softmax differ by design), and an fp32 evaluation differs from this fp64 one by about 6e-8
normwise: conftest.normwise_close at 1e-5 has more than 100x of margin."""
import numpy as np

LENET1 = (28, 5, 4, 8, 10)
# (geometry, batch, batches, Nt): LeNet-1 at the driver's batch; then the smallest geometries that
# reach each path, with one unused tail sample
CASES = {
    "lenet1": (LENET1, 100, 2, 200),
    "pool2_drops": ((12, 3, 2, 3, 4), 3, 2, 7),   # conv2 output 3: the second pool drops a row and column; P = 93
    "pool1_drops": ((14, 4, 3, 5, 3), 3, 2, 7),   # conv1 output 11: the first pool drops a row and column
    "map_1x1": ((13, 4, 3, 5, 3), 3, 2, 7),       # flat = 5: a 1 x 1 map
}
UNSUPPORTED = (28, 3, 32, 64, 10)  # P = 34 826: beyond one workgroup's LDS


def stages(geom):
    side, k, c1, c2, classes = geom
    s1 = side - k + 1
    p1 = s1 // 2
    s2 = p1 - k + 1
    p2 = s2 // 2
    return s1, p1, s2, p2


def layer_shapes(geom):
    side, k, c1, c2, classes = geom
    p2 = stages(geom)[3]
    return [(k, k, 1, c1), (c1,), (k, k, c1, c2), (c2,), (p2 * p2 * c2, classes), (classes,)]


def size(geom):
    return sum(int(np.prod(s)) for s in layer_shapes(geom))


def split(row, geom):
    """The six tensors of a model row."""
    out, o = [], 0
    for s in layer_shapes(geom):
        n = int(np.prod(s))
        out.append(np.asarray(row[o:o + n]).reshape(s))
        o += n
    assert o == len(row)
    return out


def conv_valid(h, K, b):
    """Conv2D, valid, stride 1, NHWC: out[n, y, x, o] = sum_{i,j,c} h[n, y+i, x+j, c] K[i, j, c, o] + b[o]."""
    k = K.shape[0]
    so = h.shape[1] - k + 1
    out = np.zeros((h.shape[0], so, so, K.shape[3]))
    for i in range(k):
        for j in range(k):
            out += np.einsum("nyxc,co->nyxo", h[:, i:i + so, j:j + so, :], K[i, j])
    return out + b


def avg_pool(h):
    """AveragePooling2D(2 x 2, stride 2, valid), NHWC."""
    p = h.shape[1] // 2
    h = h[:, :2 * p, :2 * p, :]
    return (h[:, 0::2, 0::2] + h[:, 0::2, 1::2] + h[:, 1::2, 0::2] + h[:, 1::2, 1::2]) / 4.0


def log_probs(x, row, geom):
    """fp64 log softmax of the model `row` on images x [n, side, side]: [n, classes]."""
    K1, b1, K2, b2, Wd, bd = (t.astype(np.float64) for t in split(row, geom))
    h = np.asarray(x, dtype=np.float64)[..., None]
    h = avg_pool(np.maximum(conv_valid(h, K1, b1), 0.0))
    h = avg_pool(np.maximum(conv_valid(h, K2, b2), 0.0))
    z = h.reshape(h.shape[0], -1) @ Wd + bd
    z = z - z.max(axis=1, keepdims=True)
    return z - np.log(np.exp(z).sum(axis=1, keepdims=True))


def costs(x, labels, models, geom, batch, batches):
    """cost[d] = mean over the batches of the mean over a batch of -log softmax(z)[label]; x
    [Nt, side, side] / labels [Nt] shared, or [D, Nt, ...] per device."""
    out = np.zeros(len(models))
    n = batch * batches
    for d, row in enumerate(models):
        xd, ld = (x, labels) if x.ndim == 3 else (x[d], labels[d])
        lp = log_probs(xd[:n], row, geom)
        loss = -lp[np.arange(n), ld[:n]]
        out[d] = loss.reshape(batches, batch).mean(axis=1).mean()
    return out


def flags(cost, target, before=None, skip=None):
    """ended[d] = ended[d] | (cost[d] < target) for every device not skipped."""
    out = np.zeros(len(cost), dtype=np.int32) if before is None else np.array(before, dtype=np.int32)
    for d in range(len(cost)):
        if skip is None or not skip[d]:
            out[d] |= int(cost[d] < target)
    return out


def make(geom, D, Nt, seed=0):
    """(x [Nt, side, side] fp32, labels [Nt] int32, models [D, P] fp32), seeded."""
    rng = np.random.default_rng(seed)
    x = rng.random((Nt, geom[0], geom[0])).astype(np.float32)
    labels = rng.integers(0, geom[4], Nt).astype(np.int32)
    models = (0.1 * rng.standard_normal((D, size(geom)))).astype(np.float32)
    return x, labels, models


_REF = {}


def reference(name, D, seed=0):
    """The case's data and its fp64 costs, computed once per (case, D, seed) and shared: read only."""
    key = (name, D, seed)
    if key not in _REF:
        geom, batch, batches, Nt = CASES[name]
        x, labels, models = make(geom, D, Nt, seed)
        ref = costs(x, labels, models, geom, batch, batches)
        for a in (x, labels, models, ref):
            a.setflags(write=False)
        _REF[key] = (x, labels, models, ref)
    return _REF[key]
