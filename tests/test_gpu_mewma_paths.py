"""The CFA-GE gradient step (cfa_mewma_update_f32 in csrc/cfa_mewma.hip, cfa_mewma_tf1_f64 in
csrc/cfa_tf1.hip) on the paths that test_gpu_kernels.py, test_gpu_entry_fuzz.py and the HostMixer
tests never take: element-strided gradients (the reference's `[..., devices]` slices held on the
device), passes chained above CFA_MAX_FANIN, every dtype mask of the fp64 entry on the scalar
kernel, on the vector kernel's grid-stride loop and across two passes, and refusals that must
leave W and the states as they were.

Reference: the oracle's tf1_mewma (cfa_ge_2stage.py:593-621: neighbour j in order, s_j = g_j at
init, else rho*g_j + (1-rho)*s_j stored in the state array's dtype, W = W - lr*(s_j if filtered
else g_j)) on host arrays of the reference's own dtypes, with rho, 1-rho, lr1 and lr2 Python
floats (weak scalars under numpy 2). A flat bucket is handed to it as four pieces cut at the
learning-rate split, so lr1 and lr2 apply to [0, split) and [split, P) separately. Bar: bit for
bit, W and every s_j; for the fp64 entry the value widened to fp64, and where the reference result
is fp32 also its round trip through fp32 (as test_mewma_tf1_f64_identical).

Knobs (init, filtered): (False, True), (False, False), (True, False). At init every state bucket
holds NaN beforehand: the kernels must not read it.

Sizes, in elements (W = 4 for the fp32 entry's float4, 2 for the fp64 entry's double2):
  scalar only      P = 1, 3 (fp32), 1 (fp64);
  body + tail      W*(3*256 + 100) + (W-1): a partial last block and a ragged scalar tail;
  grid-stride      W*((cus + 3)*256 + 77) + (W-1): both vector kernels launch one workgroup per CU,
                   so this is the first size at which their loop iterates;
  chained/strided  5 003.
The dispatch rule of both entries is mirrored in _vector_body, and every test asserts from it the
path it means to take before it launches."""
import functools
import types

import numpy as np
import pytest
import torch

from oracle import cfa_oracle as O

pytestmark = pytest.mark.gpu

BLOCK = 256     # kBlock
MAX_FANIN = 16  # CFA_MAX_FANIN
RHO = 0.99
LRS = {"f32": (0.1, 0.05), "f64": (0.025, 0.001)}
KNOBS = [(False, True), (False, False), (True, False)]  # (init, filtered)
KNOB_IDS = ["mewma_filtered", "mewma_raw", "init"]
F64 = "s64_g64_w64"
MASKS = [F64, "s32_g64_w64", "s64_g32_w64", "s32_g32_w32", "s32_g32_w64",
         "s64_g64_w32", "s32_g64_w32", "s64_g32_w32"]
P_CHAIN = 5_003


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _width(entry):
    return 4 if entry == "f32" else 2


def body_tail(entry):
    w = _width(entry)
    return w * (3 * BLOCK + 100) + (w - 1)


def grid_stride(entry, cus):
    w = _width(entry)
    return w * ((cus + 3) * BLOCK + 77) + (w - 1)


def inner_split(P):
    """No multiple of 4 and strictly inside the vector body (for P >= 8); P // 2 below that."""
    return (P // 2) | 1 if P >= 8 else P // 2


# ------------------------------------------------------------------------------------------
# Cases: host arrays in the reference's dtypes and the oracle's result (computed once, shared)
# ------------------------------------------------------------------------------------------

def _np_dtypes(entry, dtypes):
    if entry == "f32":
        return np.float32, np.float32, np.float32
    dt = {"32": np.float32, "64": np.float64}
    return dt[dtypes[1:3]], dt[dtypes[5:7]], dt[dtypes[9:11]]


def _mask(entry, dtypes):
    from federated_amd.engine import TF1_GRAD_F32, TF1_STATE_F32, TF1_W_F32
    sd, gd, wd = _np_dtypes(entry, dtypes)
    return (TF1_STATE_F32 if sd == np.float32 else 0) | (TF1_GRAD_F32 if gd == np.float32 else 0) | \
        (TF1_W_F32 if wd == np.float32 else 0)


@functools.lru_cache(maxsize=6)
def case(entry, P, n, knob, split, dtypes=F64):
    init, filtered = KNOBS[knob]
    sd, gd, wd = _np_dtypes(entry, dtypes)
    rng = np.random.default_rng([1700, int(entry == "f64"), P, n, knob, split, MASKS.index(dtypes)])
    W = rng.standard_normal(P).astype(wd)
    g = [rng.standard_normal(P).astype(gd) for _ in range(n)]
    s = [np.full(P, np.nan, sd) if init else rng.standard_normal(P).astype(sd) for _ in range(n)]
    lr1, lr2 = LRS[entry]
    # the flat bucket as the oracle's four tensors: two under lr1, two under lr2 (some may be empty)
    cuts = [0, split // 2, split, split + (P - split + 1) // 2, P]
    pieces = list(zip(cuts, cuts[1:]))
    st4 = [np.stack([x[a:b] for x in s], axis=-1) for a, b in pieces]  # [..., n] saved states
    W4 = O.tf1_mewma([W[a:b] for a, b in pieces], st4, [[x[a:b] for a, b in pieces] for x in g],
                     RHO, lr1, lr2, filtered, init)
    Wref = np.concatenate(W4)
    sref = [np.concatenate([st[:, j] for st in st4]) for j in range(n)]
    u32 = (sd if filtered else gd) == np.float32
    assert Wref.dtype == (np.float32 if wd == np.float32 and u32 else np.float64)  # numpy 2 promotion
    assert all(x.dtype == sd for x in sref) and np.isfinite(Wref).all() and all(np.isfinite(x).all() for x in sref)
    for a in [W, Wref] + g + s + sref:
        a.setflags(write=False)
    return types.SimpleNamespace(entry=entry, P=P, n=n, init=init, filtered=filtered, split=split, lr1=lr1,
                                 lr2=lr2, mask=_mask(entry, dtypes), W=W, s=s, g=g, Wref=Wref, sref=sref)


def _torch_dtype(entry):
    return torch.float32 if entry == "f32" else torch.float64


def _view(host, off, entry):
    """A device view of ``host`` (widened to the entry's dtype) ``off`` elements into an allocation."""
    tdt = _torch_dtype(entry)
    base = torch.zeros(host.size + 4, dtype=tdt, device="cuda")
    v = base[off:off + host.size]
    v.copy_(torch.tensor(host).to(tdt))
    assert v.data_ptr() % 16 == (off * v.element_size()) % 16
    return v


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def place(c, off=0, cols=None, D=0):
    """The case's buckets on the device: W and the states at element offset ``off``; gradient j
    contiguous and 16-byte aligned, or, for j in ``cols``, column cols[j] of one [P, D] stack whose
    other columns hold NaN. Returns (W, s, g, stack)."""
    dW = _view(c.W, off, c.entry)
    ds = [_view(x, off, c.entry) for x in c.s]
    cols = cols or {}
    stack = None
    if cols:
        assert len(set(cols.values())) == len(cols) < D  # at least one column is not passed
        stack = torch.full((c.P, D), float("nan"), dtype=_torch_dtype(c.entry), device="cuda")
        for j, col in cols.items():
            stack[:, col].copy_(torch.tensor(c.g[j]).to(stack.dtype))
    dg = [stack[:, cols[j]] if j in cols else _view(c.g[j], 0, c.entry) for j in range(c.n)]
    for j in cols:
        assert dg[j].stride(0) == D and dg[j].numel() == c.P
    return dW, ds, dg, stack


def _vector_body(c, dW, ds, dg):
    """Elements each pass hands to its vector kernel, as both entries decide it: all of W, s_j and
    g_j of the pass 16-byte aligned and every g_j of unit stride, then P rounded down to a vector."""
    w = _width(c.entry)
    out = []
    for done in range(0, c.n, MAX_FANIN):
        js = range(done, min(done + MAX_FANIN, c.n))
        vec = dW.data_ptr() % 16 == 0 and all(
            ds[j].data_ptr() % 16 == 0 and dg[j].data_ptr() % 16 == 0 and dg[j].stride(0) == 1 for j in js)
        out.append(c.P // w * w if vec else 0)
    return out


def _same(got, ref, what):
    wide = ref.astype(got.dtype)
    if not np.array_equal(got, wide):
        i = int(np.flatnonzero(~(got == wide))[0])
        raise AssertionError(f"{what}: first difference at element {i}: got {got[i]!r}, reference {wide[i]!r}")
    if ref.dtype != got.dtype:  # the reference result is fp32: the fp64 bucket holds exactly that value
        assert np.array_equal(got.astype(ref.dtype), ref), what


def run(gpu, c, placed):
    dW, ds, dg, stack = placed
    before = _bits(stack).clone() if stack is not None else None
    if c.entry == "f32":
        gpu.mewma(dW, ds, dg, RHO, c.lr1, c.lr2, c.split, c.init, c.filtered)
    else:
        gpu.mewma_tf1_f64(dW, ds, dg, RHO, c.lr1, c.lr2, c.split, c.init, c.filtered, c.mask)
    torch.cuda.synchronize()
    _same(dW.cpu().numpy(), c.Wref, "W")
    for j in range(c.n):
        _same(ds[j].cpu().numpy(), c.sref[j], f"s[{j}]")
    if stack is not None:
        assert torch.equal(_bits(stack), before), "the gradient stack was written"


# ------------------------------------------------------------------------------------------
# (a) Strided gradients
# ------------------------------------------------------------------------------------------

STACKS = {2: {0: 1}, 3: {0: 0, 1: 2}, 8: {j: j for j in range(5)}}  # D: {gradient j: column}
ENTRIES = [("f32", F64), ("f64", F64), ("f64", "s32_g64_w32"), ("f64", "s32_g32_w32")]
ENTRY_IDS = ["f32", "f64", "f64-s32_g64_w32", "f64-all32"]


@pytest.mark.parametrize("entry,dtypes", ENTRIES, ids=ENTRY_IDS)
@pytest.mark.parametrize("knob", range(3), ids=KNOB_IDS)
@pytest.mark.parametrize("D", list(STACKS))
@pytest.mark.parametrize("off", [0, 1])
def test_every_gradient_strided(gpu, entry, dtypes, knob, D, off):
    """g[j] = stack[:, col] of a [P, D] device stack: the scalar kernels' g[i * stride], with W
    and the states aligned (off 0) or views at element offset 1."""
    cols = STACKS[D]
    c = case(entry, P_CHAIN, len(cols), knob, inner_split(P_CHAIN), dtypes)
    placed = place(c, off, cols, D)
    assert _vector_body(c, *placed[:3]) == [0]
    run(gpu, c, placed)


@pytest.mark.parametrize("entry,dtypes", ENTRIES, ids=ENTRY_IDS)
@pytest.mark.parametrize("knob", range(3), ids=KNOB_IDS)
@pytest.mark.parametrize("which", [0, 1, 2])
def test_one_strided_gradient_sends_the_pass_to_the_scalar_kernel(gpu, entry, dtypes, knob, which):
    """One of three gradients strided, everything else contiguous and 16-byte aligned."""
    c = case(entry, P_CHAIN, 3, knob, inner_split(P_CHAIN), dtypes)
    placed = place(c, 0, {which: 1}, 3)
    dW, ds, dg, _ = placed
    assert all(t.data_ptr() % 16 == 0 for t in [dW] + ds + [dg[j] for j in range(3) if j != which])
    assert [dg[j].stride(0) for j in range(3)] == [3 if j == which else 1 for j in range(3)]
    assert _vector_body(c, dW, ds, dg) == [0]
    run(gpu, c, placed)


# ------------------------------------------------------------------------------------------
# (b) Passes chained above CFA_MAX_FANIN
# ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("entry,dtypes", ENTRIES[:2], ids=ENTRY_IDS[:2])
@pytest.mark.parametrize("knob", range(3), ids=KNOB_IDS)
@pytest.mark.parametrize("n", [16, 17, 33])
def test_chained_passes(gpu, entry, dtypes, knob, n):
    """One full pass; a full pass and a pass of one; two full passes and a pass of one: W carried
    in place, s and g indexed past the first pass. Aligned buckets: every pass on the vector kernel
    with the odd tail on the scalar one."""
    c = case(entry, P_CHAIN, n, knob, inner_split(P_CHAIN), dtypes)
    placed = place(c)
    w = _width(entry)
    assert _vector_body(c, *placed[:3]) == [P_CHAIN // w * w] * -(-n // MAX_FANIN) and P_CHAIN % w
    run(gpu, c, placed)


@pytest.mark.parametrize("entry,dtypes", ENTRIES[:2], ids=ENTRY_IDS[:2])
@pytest.mark.parametrize("knob", range(3), ids=KNOB_IDS)
def test_second_pass_on_the_scalar_kernel(gpu, entry, dtypes, knob):
    """n = 17 with only g[16] strided: the first pass takes the vector kernel, the second the
    scalar kernel, on the same W."""
    c = case(entry, P_CHAIN, 17, knob, inner_split(P_CHAIN), dtypes)
    placed = place(c, 0, {16: 1}, 2)
    w = _width(entry)
    assert _vector_body(c, *placed[:3]) == [P_CHAIN // w * w, 0]
    run(gpu, c, placed)


# ------------------------------------------------------------------------------------------
# (c) The fp64 entry's dtype masks
# ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtypes", MASKS)
@pytest.mark.parametrize("knob", range(3), ids=KNOB_IDS)
def test_masks_on_the_grid_stride_loop(gpu, cus, dtypes, knob):
    P = grid_stride("f64", cus)
    assert P // 2 > cus * BLOCK  # more double2 than one workgroup per CU holds: the loop iterates
    c = case("f64", P, 3, knob, inner_split(P), dtypes)
    placed = place(c)
    assert _vector_body(c, *placed[:3]) == [P - 1]
    run(gpu, c, placed)


@pytest.mark.parametrize("dtypes", MASKS)
@pytest.mark.parametrize("knob", range(3), ids=KNOB_IDS)
@pytest.mark.parametrize("n", [1, 16])
def test_masks_on_the_scalar_kernel(gpu, dtypes, knob, n):
    """W and the states at element offset 1 (8-byte aligned only): the whole bucket on the scalar
    kernel, with a mask."""
    P = body_tail("f64")
    c = case("f64", P, n, knob, inner_split(P), dtypes)
    placed = place(c, 1)
    assert _vector_body(c, *placed[:3]) == [0]
    run(gpu, c, placed)


@pytest.mark.parametrize("dtypes", MASKS)
@pytest.mark.parametrize("knob", range(3), ids=KNOB_IDS)
@pytest.mark.parametrize("n", [1, 3, 16])
def test_masks_on_body_and_odd_last_element(gpu, dtypes, knob, n):
    """An odd P on aligned buckets: the body on the vector kernel (N = 1, 3, 16 of both
    templates, a partial last block), the last element on the scalar one."""
    P = body_tail("f64")
    c = case("f64", P, n, knob, inner_split(P), dtypes)
    placed = place(c)
    assert P % 2 == 1 and _vector_body(c, *placed[:3]) == [P - 1]
    run(gpu, c, placed)


@pytest.mark.parametrize("dtypes", MASKS)
@pytest.mark.parametrize("knob", range(3), ids=KNOB_IDS)
def test_masks_across_two_passes(gpu, dtypes, knob):
    """n = 17: the second pass starts from the mask again, W fp32 bit included, on a W that the
    first pass may have promoted to fp64."""
    c = case("f64", P_CHAIN, 17, knob, inner_split(P_CHAIN), dtypes)
    placed = place(c)
    assert _vector_body(c, *placed[:3]) == [P_CHAIN - 1] * 2
    run(gpu, c, placed)


def test_scalar_only_f64(gpu):
    for knob in range(3):
        for dtypes in MASKS:
            for split in (0, 1):
                c = case("f64", 1, 3, knob, split, dtypes)
                placed = place(c)
                assert _vector_body(c, *placed[:3]) == [0]
                run(gpu, c, placed)


# ------------------------------------------------------------------------------------------
# (d) The fp32 entry at the same shapes
# ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("knob", range(3), ids=KNOB_IDS)
@pytest.mark.parametrize("n", [1, 5, 16])
@pytest.mark.parametrize("size", ["P=1", "P=3", "body+tail", "grid-stride"])
def test_f32_sizes(gpu, cus, knob, n, size):
    P = {"P=1": 1, "P=3": 3, "body+tail": body_tail("f32"), "grid-stride": grid_stride("f32", cus)}[size]
    c = case("f32", P, n, knob, inner_split(P))
    placed = place(c)
    assert _vector_body(c, *placed[:3]) == [P // 4 * 4] and P % 4 == (P if P < 4 else 3)
    if size == "grid-stride":
        assert P // 4 > cus * BLOCK  # more float4 than one workgroup per CU holds: the loop iterates
    run(gpu, c, placed)


@pytest.mark.parametrize("knob", range(3), ids=KNOB_IDS)
def test_f32_misaligned_w(gpu, knob):
    """W and the states at element offset 1: everything on the scalar kernel."""
    P = body_tail("f32")
    c = case("f32", P, 5, knob, inner_split(P))
    placed = place(c, 1)
    assert _vector_body(c, *placed[:3]) == [0]
    run(gpu, c, placed)


@pytest.mark.parametrize("entry,dtypes", ENTRIES, ids=ENTRY_IDS)
@pytest.mark.parametrize("knob", range(3), ids=KNOB_IDS)
@pytest.mark.parametrize("where", ["split=0", "split=P"])
def test_split_at_the_ends(gpu, entry, dtypes, knob, where):
    """One learning rate over the whole bucket: lr2 (split = 0) or lr1 (split = P)."""
    P = body_tail(entry)
    c = case(entry, P, 3, knob, 0 if where == "split=0" else P, dtypes)
    run(gpu, c, place(c))


# ------------------------------------------------------------------------------------------
# (e) A refused call launches nothing
# ------------------------------------------------------------------------------------------

def _raw_call(gpu, entry, dW, ds, g_ptrs, strides, mask=0):
    from federated_amd import _lib
    n, P = len(ds), dW.numel()
    lr1, lr2 = LRS[entry]
    head = (dW.data_ptr(), _lib.ptr_table([x.data_ptr() for x in ds]), _lib.ptr_table(g_ptrs),
            _lib.int64_array(strides), n, RHO, lr1, lr2, inner_split(P), 0, 1)
    if entry == "f32":
        _lib.call("cfa_mewma_update_f32", *head, P, gpu.stream_handle())
    else:
        _lib.call("cfa_mewma_tf1_f64", *head, mask, P, gpu.stream_handle())


def _refused(fn):
    from federated_amd._lib import CFA_E_INVALID, CFAError
    with pytest.raises(CFAError) as e:
        fn()
    assert e.value.code == CFA_E_INVALID
    torch.cuda.synchronize()


@pytest.mark.parametrize("entry", ["f32", "f64"])
@pytest.mark.parametrize("bad", ["expand view", "stride -1", "null gradient", "null state"])
def test_refusal_at_neighbour_16_leaves_buckets_unchanged(gpu, entry, bad):
    """n = 17 with valid buckets 0..15 and a bad one at index 16, in the second pass: the call is
    refused before the first pass is launched, so W and all 17 states keep their bits."""
    P, n = 64, 17
    c = case(entry, P, n, 0, inner_split(P))  # MEWMA, filtered: a launched pass rewrites W and s
    dW, ds, dg, _ = place(c)
    W0, s0 = _bits(dW).clone(), [_bits(x).clone() for x in ds]
    ptrs, strides = [x.data_ptr() for x in dg], [1] * n
    if bad == "expand view":
        dg[16] = torch.zeros(1, dtype=dW.dtype, device="cuda").expand(P)
        assert dg[16].dim() == 1 and dg[16].numel() == P and dg[16].stride(0) == 0
        if entry == "f32":
            _refused(lambda: gpu.mewma(dW, ds, dg, RHO, c.lr1, c.lr2, c.split, False, True))
        else:
            _refused(lambda: gpu.mewma_tf1_f64(dW, ds, dg, RHO, c.lr1, c.lr2, c.split, False, True, 0))
    elif bad == "stride -1":
        strides[16] = -1
        _refused(lambda: _raw_call(gpu, entry, dW, ds, ptrs, strides))
    elif bad == "null gradient":
        ptrs[16] = None
        _refused(lambda: _raw_call(gpu, entry, dW, ds, ptrs, strides))
    else:
        from federated_amd import _lib
        lr1, lr2 = LRS[entry]
        s_ptrs = [x.data_ptr() for x in ds[:16]] + [None]
        args = (dW.data_ptr(), _lib.ptr_table(s_ptrs), _lib.ptr_table(ptrs), _lib.int64_array(strides), n, RHO,
                lr1, lr2, c.split, 0, 1)
        if entry == "f32":
            _refused(lambda: _lib.call("cfa_mewma_update_f32", *args, P, gpu.stream_handle()))
        else:
            _refused(lambda: _lib.call("cfa_mewma_tf1_f64", *args, 0, P, gpu.stream_handle()))
    assert torch.equal(_bits(dW), W0), "W was rewritten by a refused call"
    for j in range(n):
        assert torch.equal(_bits(ds[j]), s0[j]), f"s[{j}] was rewritten by a refused call"


@pytest.mark.parametrize("entry", ["f32", "f64"])
def test_refusals_at_one_neighbour(gpu, entry):
    P = 64
    c = case(entry, P, 1, 0, inner_split(P))
    dW, ds, dg, _ = place(c)
    W0, s0 = _bits(dW).clone(), _bits(ds[0]).clone()
    ptrs = [dg[0].data_ptr()]
    _refused(lambda: _raw_call(gpu, entry, dW, ds, ptrs, [0]))
    _refused(lambda: _raw_call(gpu, entry, dW, ds, ptrs, [-1]))
    zero = [torch.zeros(1, dtype=dW.dtype, device="cuda").expand(P)]
    if entry == "f32":
        _refused(lambda: gpu.mewma(dW, ds, zero, RHO, c.lr1, c.lr2, c.split, False, True))
    else:
        _refused(lambda: gpu.mewma_tf1_f64(dW, ds, zero, RHO, c.lr1, c.lr2, c.split, False, True, 0))
        _refused(lambda: _raw_call(gpu, entry, dW, ds, ptrs, [1], mask=0x8))  # an unknown dtype bit
        _refused(lambda: gpu.mewma_tf1_f64(dW, ds, dg, RHO, c.lr1, c.lr2, c.split, False, True, 0x8))
    assert torch.equal(_bits(dW), W0) and torch.equal(_bits(ds[0]), s0)
