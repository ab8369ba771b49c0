"""The LeNet-family kernels (csrc/cfa_lenet.hip, cfa_lenet_grad.hip, on the phases of
cfa_lenet_graph.h) on the loops, lane plans and branches that test_gpu_lenet_validation.py and
test_gpu_lenet_training.py never take:

gradient  a K = 5 geometry whose pools both drop a row and column; more weight-gradient items than
          threads (`idx += T` runs again, one lane a sum) in both kernel forms; 64 lanes a sum with
          fewer rows than lanes; second and third passes of lenet_logits, lenet_xent and
          lenet_dense_backward at 17, 33 and 64 classes; three groups, the last of one sample; the
          finish grid where P + 1 fills a block exactly and where it spills one thread into a second;
          a launch above 64 KiB of LDS; a negative `first`; a `src` entry outside [0, D) at the
          kernel; relu at exactly z == 0; a softmax whose probabilities underflow in fp32.
validation  a workgroup that owns several batches and a population above 256 devices (the batch loop
          of lenet_eval_kernel, the device loop of lenet_finish_kernel), with skip, flags and a
          saturated log there; partial chunks of 1 and 2 samples; the K = 5 geometry with dropped
          rows and a partial-wave pass of lenet_logits; a launch above 64 KiB of LDS; the saturated
          softmax.

The table cases live in lenet_cases.py and lenet_grad_cases.py (PATHS), so the host tests pin their
references by torch's CPU fp64 and hold their seeds to the margin rule; `path()` there gives the
arithmetic that puts a case on its path, and every test here asserts it first, with the device's own
CU count and LDS limit where it depends on them. The comparison is the two files' own: the fp64
restatement, `normwise_close(., 1e-5)` per tensor, 1e-5 on the loss; every measured error is
printed."""
import numpy as np
import pytest
import torch

import lenet_cases as lc
import lenet_grad_cases as gc
import test_gpu_lenet_training as gt
import test_gpu_lenet_validation as vt
from conftest import normwise_close

pytestmark = pytest.mark.gpu

D = gc.D
SENTINEL = gt.SENTINEL
SMALL = "pool2_drops"  # (12, 3, 2, 3, 4), P = 93: the edges run on it


def _device():
    """(compute units, LDS bytes a workgroup may take) as the device reports them."""
    p = torch.cuda.get_device_properties(torch.cuda.current_device())
    return int(p.multi_processor_count), int(p.shared_memory_per_block)


def _assert_path(conditions):
    assert conditions and all(conditions.values()), [k for k, v in conditions.items() if not v]


def _skip_below(need):
    limit = _device()[1]
    if limit < need:
        pytest.skip(f"the device reports {limit} bytes of LDS per workgroup, the launch needs {need}")
    return limit


def _assert_tensors(tag, got, ref, geom):
    """Every tensor of the gradient row `got` within 1e-5 normwise of `ref`; the worst error."""
    worst = 0.0
    for i, (a, b) in enumerate(zip(gc.tensors(got, geom), gc.tensors(ref, geom))):
        err = np.max(np.abs(a.astype(np.float64) - b)) / np.max(np.abs(b))
        worst = max(worst, err)
        print(tag, "tensor", i, "normwise error", err)
        assert normwise_close(a, b, rtol=1e-5), (tag, i, err)
    return worst


# ------------------------------------------------------------------------------------------
# Gradient: the table's PATHS cases
# ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", gc.PATHS)
def test_gradient_path_parity(gpu, name):
    """Gradient and loss of every PATHS case against the fp64 restatement, the padding untouched,
    the same bits twice and for a row alone. What each case reaches (gc.path asserts the numbers):

    k5_drops       lenet_conv_pool<5> and lenet_conv_wgrad<5> (w[] slides through registers) at
                   23 -> 19 -> 9 -> 5 -> 2, where both pools drop a row and column; stage 2 has
                   5 * 4 * 13 = 260 items > 256 threads, so L = 1 and `idx += T` runs a second pass;
                   lenet_logits has 2 * 17 * 8 = 272 lanes > 256, a second pass of 16 lanes; a batch
                   of 9 is three groups of 4, 4 and 1 samples.
    generic_items  the runtime-k lenet_conv_wgrad<0> with 3 * 8 * 11 = 264 items > 256.
    lanes_64       3 items and one channel per stage: L = 64 for both weight and both bias gradients;
                   a one-sample chunk has 8 (stage 1) and 2 (stage 2) rows, so most lanes sum nothing.
    classes_64     2 * 64 * 8 = 1 024 logit lanes: four full passes; lenet_xent and
                   lenet_dense_backward at the entry's most classes.
    classes_33     2 * 33 * 8 = 528 lanes: two passes and a third of 16 lanes.
    finish_255     P + 1 = 256: the loss is the last thread of the one finish block.
    finish_256     P + 1 = 257: the loss is the only live thread of a second finish block.
    raised_lds     141 736 bytes of dynamic LDS > 65 536: the launch goes through raise_lds_limit."""
    limit = _skip_below(gc.plan(name)["lds"]) if name == "raised_lds" else _device()[1]
    _assert_path(gc.path(name, limit))
    _, _, models = gc.data(name)
    P = models.shape[1]
    out, loss = gt._grad(gpu, name, models)
    g, l = out.cpu().numpy(), loss.cpu().numpy()
    worst = max(gt._assert_parity(name, g[d, :P], l[d], d) for d in range(D))
    print("case", name, "worst normwise error", worst)
    assert (g[:, P:] == SENTINEL).all()
    wide, wloss = gt._grad(gpu, name, models, pad=7)
    assert (gt._bits(wide[:, :P]) == gt._bits(out[:, :P])).all() and (gt._bits(wloss) == gt._bits(loss)).all()
    assert (wide[:, P:].cpu().numpy() == SENTINEL).all()
    one, oloss = gt._grad(gpu, name, models[1:2])
    assert (gt._bits(one[0, :P]) == gt._bits(out[1, :P])).all() and gt._bits(oloss)[0] == gt._bits(loss)[1]


@pytest.mark.parametrize("name", ["k5_drops", "lanes_64"])
def test_gradient_path_with_first_and_a_wrap(gpu, name):
    """The same cases on another batch of the set, one that wraps: the last group of k5_drops (one
    sample) and the one-sample chunk of lanes_64 then hold other samples."""
    _, _, Nt, _ = gc.CASES[name]
    _, _, models = gc.data(name)
    P = models.shape[1]
    first = [Nt - 1, 1, Nt - 2]
    out, loss = gt._grad(gpu, name, models, first=gt._cuda(np.array(first, dtype=np.int64)))
    g, l = out.cpu().numpy(), loss.cpu().numpy()
    for d in range(D):
        gt._assert_parity(name, g[d, :P], l[d], d, first=first[d], what="first")


@pytest.mark.parametrize("name", ["finish_255", "finish_256"])
def test_finish_grid_edge_writes_the_loss_and_nothing_beyond(gpu, name):
    """lenet_grad_finish_kernel's grid is ceil((P + 1) / 256) blocks: at P = 255 the loss is thread
    255 of the only block, at P = 256 thread 0 of a second one whose other 255 threads own nothing.
    The loss is written (parity), and the row padding and a sentinel behind loss[D - 1] are not."""
    geom, batch, _, _ = gc.CASES[name]
    _assert_path(gc.path(name))
    x, labels, models = gc.data(name)
    P = models.shape[1]
    assert P == (255 if name == "finish_255" else 256)
    W = gt._stack(models)
    out = torch.full((D, P + 5), SENTINEL, dtype=torch.float32, device="cuda")
    loss = torch.full((D + 1,), SENTINEL, dtype=torch.float32, device="cuda")
    ws = gpu.lenet_grad_workspace(D, batch, geom)
    gpu.lenet_grad(geom, gt._cuda(x), gt._cuda(labels), W, batch, out[:, :P], ws, loss[:D])
    torch.cuda.synchronize()
    g, l = out.cpu().numpy(), loss.cpu().numpy()
    for d in range(D):
        gt._assert_parity(name, g[d, :P], l[d], d, what="edge")
    assert (g[:, P:] == SENTINEL).all() and l[D] == SENTINEL and (l[:D] != SENTINEL).all()


# ------------------------------------------------------------------------------------------
# Gradient: edges, on the small cases
# ------------------------------------------------------------------------------------------

def test_a_negative_first_counts_from_the_sets_end(gpu):
    """The `f0 < 0` branch after C's `%` in lenet_grad_kernel: first = -1 is the set's last sample
    and first = -Nt - 2 the one before (-13 % 11 == -2 in C, + Nt), with the bits of the
    non-negative form and the fp64 reference's parity for those batches."""
    name = "generic_k"
    _, _, Nt, _ = gc.CASES[name]
    _, _, models = gc.data(name)
    P = models.shape[1]
    same = [Nt - 1, Nt - 2, 0]
    neg, nloss = gt._grad(gpu, name, models, first=gt._cuda(np.array([-1, -Nt - 2, 0], dtype=np.int64)))
    pos, ploss = gt._grad(gpu, name, models, first=gt._cuda(np.array(same, dtype=np.int64)))
    assert (gt._bits(neg) == gt._bits(pos)).all() and (gt._bits(nloss) == gt._bits(ploss)).all()
    g, l = neg.cpu().numpy(), nloss.cpu().numpy()
    for d in range(D):
        gt._assert_parity(name, g[d, :P], l[d], d, first=same[d], what="negative first")


def test_a_src_out_of_range_gives_that_row_nan_at_the_kernel(gpu):
    """The kernel's own early exit for a `src` entry outside [0, D) (a device tensor goes through
    Engine.lenet_grad unchecked): nothing is read, rows 1 and 2 and their losses become NaN, row 0
    has the bits it has with a valid `src`, and the padding is untouched."""
    name = SMALL
    _, _, models = gc.data(name)
    P = models.shape[1]
    out, loss = gt._grad(gpu, name, models, pad=2, src=gt._cuda(np.array([1, D, -1], dtype=np.int32)))
    good, gloss = gt._grad(gpu, name, models, pad=2, src=gt._cuda(np.array([1, 1, 1], dtype=np.int32)))
    g, l = out.cpu().numpy(), loss.cpu().numpy()
    assert np.isnan(g[1:, :P]).all() and np.isnan(l[1:]).all()
    assert (gt._bits(out[0]) == gt._bits(good[0])).all() and gt._bits(loss)[0] == gt._bits(gloss)[0]
    assert np.isfinite(g[0, :P]).all() and (g[:, P:] == SENTINEL).all()
    gt._assert_parity(name, g[0, :P], l[0], 1, what="src")


def _zero_convolutions():
    """Models of SMALL's geometry whose K1, b1, K2, b2 are zero, every third entry -0.0, with Wd and
    bd random: every pre-activation of both convolutions is exactly 0."""
    geom = gc.CASES[SMALL][0]
    P, flat, C = lc.size(geom), lc.stages(geom)[3] ** 2 * geom[3], geom[4]
    models = (0.1 * np.random.default_rng(5).standard_normal((D, P))).astype(np.float32)
    models[:, :P - flat * C - C] = 0.0
    models[:, 0:P - flat * C - C:3] = -0.0
    return models, P - flat * C - C, P - C


def test_relu_at_exactly_zero_passes_nothing(gpu):
    """The relu test is `z > 0`, forward and backward (TF's ReluGrad): with K1, b1, K2, b2 all zero
    (some -0.0) every pre-activation is exactly 0, so every gate is shut. dK1, db1, dK2, db2 and
    dWd (flat = 0) must be exactly 0.0 (bits, modulo sign), and dbd and the loss the fp64
    reference's, whose loss is that of logits = bd. dK1, db1 and dK2 are zero whatever the gate is
    (K2 = 0 and a1 = 0); db2 is what tells: a kernel that gated on `z >= 0` would give
    db2[c] = mean_s sum_{py,px} dflat[s, py, px, c], which the test shows is not zero for this
    model. The case is outside the margin rule on purpose: its expectation is exact."""
    name = SMALL
    geom, batch, _, _ = gc.CASES[name]
    x, labels, _ = gc.data(name)
    models, oWd, obd = _zero_convolutions()
    out, loss = gt._grad(gpu, name, models)
    g, l = out.cpu().numpy(), loss.cpu().numpy()
    p2, c2 = lc.stages(geom)[3], geom[3]
    for d in range(D):
        ref, ref_loss = gc.grads(x[:batch], labels[:batch], models[d], geom)
        bd = models[d, obd:].astype(np.float64)
        lse = bd.max() + np.log(np.exp(bd - bd.max()).sum())
        assert abs(ref_loss - np.mean(lse - bd[labels[:batch]])) <= 1e-12 and (ref[:obd] == 0).all()
        # what `z >= 0` would have passed to db2
        dz = np.tile(np.exp(bd - lse), (batch, 1))
        dz[np.arange(batch), labels[:batch]] -= 1.0
        open_gate = (dz @ models[d, oWd:obd].astype(np.float64).reshape(-1, geom[4]).T).reshape(batch, p2 * p2, c2)
        assert np.abs(open_gate.sum(axis=1).mean(axis=0)).max() > 1e-3
        assert (out[d, :obd].cpu().numpy().view(np.uint32) & 0x7fffffff == 0).all()
        err = np.max(np.abs(g[d, obd:len(ref)] - ref[obd:])) / np.max(np.abs(ref[obd:]))
        print("relu at zero, model", d, "dbd normwise error", err, "loss error", abs(l[d] - ref_loss))
        assert normwise_close(g[d, obd:len(ref)], ref[obd:], 1e-5) and abs(float(l[d]) - ref_loss) <= 1e-5


def _saturated():
    """SMALL's models with the Wd block times 1e4 (in fp32): the logits are hundreds apart."""
    geom = gc.CASES[SMALL][0]
    P, flat, C = lc.size(geom), lc.stages(geom)[3] ** 2 * geom[3], geom[4]
    models = gc.data(SMALL)[2].copy()
    models[:, P - flat * C - C:P - C] *= np.float32(1e4)
    return models


def test_a_softmax_that_underflows_in_fp32_gives_a_finite_cost_and_gradient(gpu):
    """The log-softmax form -(z_l - max - log(sum exp(z - max))) where class probabilities
    underflow in fp32 (the reference's log of the softmax output gives inf there; the library a
    finite cost, by design): Wd times 1e4 gives fp64 costs of 24 to 277, and for two of the three
    models every labelled probability of the gradient's batch lies below fp32's smallest subnormal
    (asserted; the third model stays representable, at costs near 24). The convolutions are untouched, so the
    relu margins are the case's own. Every loss and cost is finite; the validation cost and the
    gradient meet the fp64 restatement (which uses the max-shifted form) at 1e-5 normwise, the loss
    at 1e-5 relative to the reference loss."""
    name = SMALL
    geom, batch, Nt, _ = gc.CASES[name]
    assert lc.CASES[name] == (geom, batch, 2, Nt)  # the validation case of the same name: two batches
    x, labels, _ = gc.data(name)
    models = _saturated()
    lp = np.stack([lc.log_probs(x[:2 * batch], row, geom)[np.arange(2 * batch), labels[:2 * batch]] for row in models])
    gone = np.log(2.0 ** -149)  # below it a probability is 0 in fp32, and its log -inf
    assert ((lp[:, :batch] < gone).all(axis=1).sum(), (lp[:, batch:] < gone).any(axis=1).sum()) == (2, 2)
    ref_cost = lc.costs(x, labels, models, geom, batch, 2)
    assert ref_cost.min() > 20 and ref_cost.max() > 270
    val = vt._validation(gpu, name, x, labels)
    cost = val.validate(vt._stack(models, 3)).cpu().numpy()
    print("saturated validation cost", cost, "normwise error", np.max(np.abs(cost - ref_cost)) / np.max(ref_cost))
    assert np.isfinite(cost).all() and normwise_close(cost, ref_cost, 1e-5)
    out, loss = gt._grad(gpu, name, models)
    g, l = out.cpu().numpy(), loss.cpu().numpy()
    P = models.shape[1]
    assert np.isfinite(g[:, :P]).all() and np.isfinite(l).all()
    for d in range(D):
        ref, ref_loss = gc.grads(x[:batch], labels[:batch], models[d], geom)
        worst = _assert_tensors(f"saturated model {d}", g[d, :P], ref, geom)
        print("saturated model", d, "loss", l[d], "reference", ref_loss, "worst tensor", worst)
        assert abs(float(l[d]) - ref_loss) <= 1e-5 * abs(ref_loss)


# ------------------------------------------------------------------------------------------
# Validation
# ------------------------------------------------------------------------------------------

def _many(gpu):
    """The "many_batches" case at D = 600 on this device: its conditions asserted with the device's
    CU count, and (x, labels, models, fp64 costs)."""
    cus, _ = _device()
    _, _, batches, _ = lc.CASES["many_batches"]
    assert (4 * cus + lc.MANY_D - 1) // lc.MANY_D < batches  # fewer workgroups per device than batches
    _assert_path(lc.path("many_batches", lc.MANY_D, cus))
    return lc.reference("many_batches", lc.MANY_D)


def test_a_workgroup_that_owns_several_batches_and_more_devices_than_a_block(gpu):
    """lenet_eval_kernel's `for (b = blockIdx.x; b < batches; b += gridDim.x)` and
    lenet_finish_kernel's `d += blockDim.x`: 600 devices and 5 batches of 3. The launcher gives
    about 4 workgroups per CU over all devices, ceil(4 * CUs / 600) per device, which is below 5
    batches for any device of up to 300 CUs (asserted from the device's count; 2 workgroups on the
    MI355X, owning batches 0, 2, 4 and 1, 3), so the loss array and the chunk buffers in LDS are
    reused across batches. Cost parity for all 600; and the bits of devices 0, 255, 256 and 599 are
    those of the same model validated alone, where every batch has a workgroup of its own (asserted):
    a batch loss does not depend on the grid."""
    x, labels, models, ref = _many(gpu)
    cus, _ = _device()
    _, _, batches, _ = lc.CASES["many_batches"]
    val = vt._validation(gpu, "many_batches", x, labels)
    cost = val.validate(vt._stack(models, 3)).clone()
    got = cost.cpu().numpy()
    print("many_batches D", lc.MANY_D, "max rel err", np.max(np.abs(got - ref)) / np.max(np.abs(ref)))
    assert normwise_close(got, ref, 1e-5)
    assert lc.eval_grid_x(batches, 1, cus) == batches
    for d in (0, 255, 256, 599):
        alone = vt._validation(gpu, "many_batches", x, labels).validate(vt._stack(models[d:d + 1]))
        assert vt._bits(alone)[0] == vt._bits(cost)[d], d


def test_skip_flags_and_a_saturated_log_above_256_devices(gpu):
    """The finish kernel's second and third trips (devices 256 to 599) with everything it does:
    skipped devices on both sides of 256 keep cost and flag and log their untouched cost, the others
    raise their flags by the restatement's rule, and with log_cap = 2 three calls leave the first
    call in row 0 and the third in row 1, as test_log has it at D = 5."""
    x, labels, models, ref = _many(gpu)
    n = lc.MANY_D
    target = vt._gap_target(ref)
    W = vt._stack(models)
    val = vt._validation(gpu, "many_batches", x, labels, target=target, log_cap=2)
    plain = val.validate(W).clone()
    skipped = [3, 255, 256, 599]
    flags = np.zeros(n, dtype=np.int32)
    flags[skipped] = 1
    skip = vt._cuda(flags)
    ended = torch.zeros(n, dtype=torch.int32, device="cuda")
    val.val_cost.fill_(SENTINEL)
    val.validate(W, skip=skip, ended=ended)
    cost = val.val_cost.cpu().numpy()
    others = np.setdiff1d(np.arange(n), skipped)
    assert (cost[skipped] == SENTINEL).all() and (vt._bits(val.val_cost)[others] == vt._bits(plain)[others]).all()
    want = lc.flags(ref, target, skip=flags)
    assert 0 < want.sum() < n and ended.cpu().numpy().tolist() == want.tolist()
    assert (vt._bits(val.val_log[1]) == vt._bits(val.val_cost)).all()  # the second call's row, the skipped ones' too
    assert (vt._bits(val.val_log[0]) == vt._bits(plain)).all()
    # a third call, another population: row 1 is overwritten, row 0 stays
    other = lc.make(lc.CASES["many_batches"][0], n, 16, seed=12)[2]
    third = val.validate(vt._stack(other)).clone()
    assert val.epochs_done == 3
    assert (vt._bits(val.val_log[0]) == vt._bits(plain)).all() and (vt._bits(val.val_log[1]) == vt._bits(third)).all()
    assert not (vt._bits(third) == vt._bits(plain)).any()


@pytest.mark.parametrize("name,n,pad", [(name, n, pad) for name in ("chunk_tail_1", "chunk_tail_2", "k5_drops")
                                        for n, pad in ((1, 0), (5, 3))])
def test_validation_path_parity(gpu, name, n, pad):
    """chunk_tail_1, chunk_tail_2: batches of 5 and 6 samples are a chunk of 4 and a partial one of 1
    and of 2 (the earlier cases have only 3). k5_drops: lenet_conv_pool<5> where both pools drop a
    row and column (23 -> 19 -> 9 -> 5 -> 2), and lenet_logits with 4 * 17 * 8 = 544 lanes: two full
    passes and a third of 32 lanes, half a wave (136 lanes for the one-sample chunk)."""
    _assert_path(lc.path(name, n, _device()[0]))
    x, labels, models, ref = lc.reference(name, n)
    val = vt._validation(gpu, name, x, labels)
    cost = val.validate(vt._stack(models, pad)).cpu().numpy()
    print(name, n, pad, "cost", cost, "max rel err", np.max(np.abs(cost - ref)) / np.max(np.abs(ref)))
    assert normwise_close(cost, ref, 1e-5)


def test_launches_above_64_kib_of_lds(gpu):
    """Both entries through raise_lds_limit: (20, 3, 8, 32, 40), P = 13 976. By the documented
    formulas the gradient kernel needs 4 * (2 P + 2 * 3 504 + 4 + 2 + 468) = 141 736 bytes and the
    validation kernel 4 * (P + 4 * 1 376 + 3) = 77 932, both in (65 536, the device's limit]
    (asserted from the device; skipped, with that reason, on a device that reports less).
    Validation parity, and the gradient's loss has the bits of the validation kernel's batch loss
    (gradient parity: test_gradient_path_parity[raised_lds])."""
    name = "raised_lds"
    geom, batch, Nt, _ = gc.CASES[name]
    need_grad, need_eval = gc.grad_lds_bytes(geom), lc.eval_lds_bytes(geom, batch)
    assert (need_grad, need_eval) == (4 * (2 * 13976 + 2 * 3504 + 4 + 2 + 468), 4 * (13976 + 4 * 1376 + 3))
    limit = _skip_below(max(need_grad, need_eval))
    assert 65536 < need_eval <= limit and 65536 < need_grad <= limit
    _assert_path(gc.path(name, limit))
    _assert_path(lc.path(name, D, _device()[0], limit))
    assert lc.CASES[name] == (geom, batch, 1, Nt)
    x, labels, models, ref = lc.reference(name, D)
    cost = vt._validation(gpu, name, x, labels).validate(vt._stack(models, 1)).cpu().numpy()
    print(name, "validation cost", cost, "max rel err", np.max(np.abs(cost - ref)) / np.max(np.abs(ref)))
    assert normwise_close(cost, ref, 1e-5)
    # the shared forward, on the gradient case's own data (another seed)
    x, labels, models = gc.data(name)
    _, loss = gt._grad(gpu, name, models)
    one = vt._validation(gpu, name, x, labels).validate(gt._stack(models)).cpu().numpy()
    assert (one.astype(np.float32).view(np.uint32) == gt._bits(loss)).all()
    assert (one.astype(np.float32).astype(np.float64) == one).all()
