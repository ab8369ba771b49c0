"""The cases of tests/test_lenet_validation_host.py and tests/test_gpu_lenet_validation.py: the
LeNet-1 family's forward pass, validation cost and flag rule restated in numpy fp64 from the layer
definitions (no torch here), the geometry table and the seeded data.

The family, geometry (side, kernel, c1, c2, classes), Keras semantics: input [side, side, 1];
Conv2D(c1, k x k, valid, relu), a cross-correlation with the kernel tensor (kh, kw, in, out);
AveragePooling2D(2 x 2, stride 2, valid), which drops an odd last row and column; Conv2D(c2);
AveragePooling2D; Flatten in NHWC order; Dense(classes, softmax). A model row is get_weights()
order, C-order: K1 b1 K2 b2 Wd bd.

Data: images rng.random in [0, 1), weights 0.1 * standard_normal, labels uniform. With it every
class probability stays above 0.07 (above 0.014 in the PATHS cases, which have up to 40 classes)
and the costs lie between 1 and 2.4 (up to 3.9 there), far from the region where a probability
underflows in fp32 (there the library's log-softmax and the reference's log of the softmax differ
by design; tests/test_gpu_lenet_paths.py goes there on purpose, with a model of its own), and an
fp32 evaluation differs from this fp64 one by about 6e-8 normwise: conftest.normwise_close at 1e-5
has more than 100x of margin.

PATHS names the cases that exist for a loop or branch of cfa_lenet.hip the others never take;
`path(name, ...)` restates the launch plan (cfa_lenet.hip, cfa_internal.h: shared_grid_x) and
gives the arithmetic that puts the case there, as named conditions that the tests assert."""
import numpy as np

LENET1 = (28, 5, 4, 8, 10)
# (geometry, batch, batches, Nt): LeNet-1 at the driver's batch; then the smallest geometries that
# reach each path, with one unused tail sample
CASES = {
    "lenet1": (LENET1, 100, 2, 200),
    "pool2_drops": ((12, 3, 2, 3, 4), 3, 2, 7),   # conv2 output 3: the second pool drops a row and column; P = 93
    "pool1_drops": ((14, 4, 3, 5, 3), 3, 2, 7),   # conv1 output 11: the first pool drops a row and column
    "map_1x1": ((13, 4, 3, 5, 3), 3, 2, 7),       # flat = 5: a 1 x 1 map
    # the paths no case above takes (PATHS, path()), each again with one unused tail sample
    "many_batches": ((12, 3, 2, 3, 4), 3, 5, 16),    # at D = 600: 2 workgroups own a device's 5 batches, D > 256
    "chunk_tail_1": ((12, 3, 2, 3, 4), 5, 2, 11),    # chunks of 4 and 1 samples
    "chunk_tail_2": ((12, 3, 2, 3, 4), 6, 2, 13),    # chunks of 4 and 2 samples
    "k5_drops": ((23, 5, 4, 13, 17), 5, 2, 11),      # 23 -> 19 -> 9 -> 5 -> 2: the K = 5 kernel, both pools drop
    "raised_lds": ((20, 3, 8, 32, 40), 3, 1, 4),     # P = 13 976: 77 932 bytes of LDS, above the default 64 KiB
}
PATHS = ("many_batches", "chunk_tail_1", "chunk_tail_2", "k5_drops", "raised_lds")
MANY_D = 600  # the population of "many_batches"
UNSUPPORTED = (28, 3, 32, 64, 10)  # P = 34 826: beyond one workgroup's LDS


# cfa_lenet.hip: kLenetBlock, kLenetChunk, the workgroups per CU of the launch; the dynamic LDS of a
# launch before the kernel's limit is raised
BLOCK, CHUNK, WG_PER_CU, LDS_DEFAULT = 256, 4, 4, 65536


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


def eval_lds_bytes(geom, batch):
    """lenet_eval_lds: the model, a chunk's activations (image, two pooled maps, logits), a batch's losses."""
    side, k, c1, c2, classes = geom
    _, p1, _, p2 = stages(geom)
    sample = side * side + p1 * p1 * c1 + p2 * p2 * c2 + classes
    return 4 * (size(geom) + CHUNK * sample + batch)


def eval_grid_x(batches, D, cus):
    """grid.x of lenet_eval_kernel: shared_grid_x(batches, 4, D) workgroups per device, evened out."""
    gx = max(1, min(batches, (cus * WG_PER_CU + D - 1) // D))
    per = (batches + gx - 1) // gx
    return (batches + per - 1) // per


def path(name, D=1, cus=256, lds_limit=160 * 1024):
    """The conditions that put the PATHS case `name` on its path, {text: bool}, for a population of
    D on a device of `cus` compute units and `lds_limit` bytes of LDS per workgroup."""
    geom, batch, batches, Nt = CASES[name]
    side, k, c1, c2, classes = geom
    s1, p1, s2, p2 = stages(geom)
    tail = batch % CHUNK
    if name == "many_batches":
        gx = eval_grid_x(batches, D, cus)
        return {"fewer workgroups than batches: ceil(4 CUs / D) < batches": (WG_PER_CU * cus + D - 1) // D < batches,
                "a workgroup's batch loop runs again": 1 <= gx < batches,
                "the finish kernel's device loop runs again": D > BLOCK}
    if name in ("chunk_tail_1", "chunk_tail_2"):
        return {"a full chunk, then one of %d" % tail: batch > CHUNK and tail == int(name[-1])}
    if name == "k5_drops":
        return {"the K = 5 kernel": k == 5, "both pools drop a row and column": s1 % 2 == 1 and s2 % 2 == 1,
                "a third, partial-wave pass of lenet_logits: 4 * 17 * 8 = 544 = 2 * 256 + 32":
                    CHUNK * classes * 8 == 544 and 0 < CHUNK * classes * 8 % BLOCK < 64,
                "a chunk of one sample": tail == 1}
    if name == "raised_lds":
        need = eval_lds_bytes(geom, batch)
        return {"77 932 bytes of LDS": need == 77932, "above the default limit": need > LDS_DEFAULT,
                "within the device's": need <= lds_limit}
    raise KeyError(name)


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
