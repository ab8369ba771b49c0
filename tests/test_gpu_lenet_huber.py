"""The Huber drivers' objective on the device (cfa_lenet_eval_loss_f32, cfa_lenet_grad_loss_f32 with
CFA_LENET_LOSS_HUBER; `loss="huber"` of LenetValidation and LenetTraining) against the fp64
restatement of tests/lenet_huber_cases.py (its docstring has the objective, the labels that put
every Huber branch into every batch, and the seed rule; test_lenet_huber_host.py pins the
restatement by torch's autograd and checks the labels and seeds).

Every case has D = 3 devices. The bounds are those of the kernel family's cross-entropy tests
(test_gpu_lenet_training.py, test_gpu_lenet_validation.py): normwise 1e-5 per tensor and on the
validation costs, 1e-5 on a batch loss."""
import numpy as np
import pytest
import torch

import lenet_grad_cases as gc
import lenet_huber_cases as hc
from conftest import normwise_close

pytestmark = pytest.mark.gpu

D = hc.D
SENTINEL = -7.25
NAMES = sorted(hc.CASES)


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()  # a copy: the shared reference data is read only


def _stack(models):
    """The models as a [D, P] CUDA view of a stack whose rows are pitched to 16 bytes; NaN padding."""
    n, P = models.shape
    full = torch.full((n, (P + 3) // 4 * 4), float("nan"), dtype=torch.float32, device="cuda")
    full[:, :P] = _cuda(models)
    return full[:, :P]


def _bits(t):
    a = t.detach().cpu().contiguous().numpy()
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _grad(gpu, name, models, x=None, labels=None, loss_kind="huber", **kw):
    """One Engine.lenet_grad call on the case's set (or x / labels): (grads [n, P] view, loss [n])."""
    geom, batch, _, _ = hc.CASES[name]
    x0, l0, _ = hc.data(name)
    xs, ls = _cuda(x0 if x is None else x), _cuda(l0 if labels is None else labels)
    W = _stack(models)
    n, P = W.shape
    out = torch.full((n, (P + 3) // 4 * 4), SENTINEL, dtype=torch.float32, device="cuda")
    loss = torch.full((n,), SENTINEL, dtype=torch.float32, device="cuda")
    ws = gpu.lenet_grad_workspace(n, batch, geom)
    gpu.lenet_grad(geom, xs, ls, W, batch, out[:, :P], ws, loss, loss_kind=loss_kind, **kw)
    torch.cuda.synchronize()
    return out[:, :P], loss


def _sets(name, per_device):
    return hc.per_device(name) if per_device else hc.data(name)[:2]


def _training(gpu, name, per_device=False, **kw):
    from federated_amd.tf2_training import LenetTraining
    geom, batch, _, _ = hc.CASES[name]
    x, labels = _sets(name, per_device)
    return LenetTraining(gpu, geom, _cuda(x), _cuda(labels), batch, **kw)


def _validation(gpu, name, per_device=False, batches=hc.VAL_BATCHES, **kw):
    from federated_amd.tf2_validation import LenetValidation
    geom, batch, _, _ = hc.CASES[name]
    x, labels = _sets(name, per_device)
    return LenetValidation(gpu, geom, _cuda(x), _cuda(labels), batch, batches, **kw)


def _assert_parity(name, got_row, got_loss, model, first=0, shift=0, what=""):
    geom = hc.CASES[name][0]
    ref, ref_loss = hc.reference(name, model, first, shift)
    worst = 0.0
    for i, (a, b) in enumerate(zip(gc.tensors(got_row, geom), gc.tensors(ref, geom))):
        err = np.max(np.abs(a.astype(np.float64) - b)) / np.max(np.abs(b))
        worst = max(worst, err)
        assert normwise_close(a, b, rtol=1e-5), (name, what, model, i, err)
    print(name, what, "model", model, "first", first, "shift", shift, "loss", got_loss, "loss error",
          abs(float(got_loss) - ref_loss), "worst tensor", worst)
    assert abs(float(got_loss) - ref_loss) <= 1e-5
    return worst


def _gap_target(ref):
    """The midpoint of the widest gap between two devices' reference costs. The gap must exceed
    1e-4 of the larger cost: a device cost within the parity bound (1e-5) of its reference then
    stays on its side of the midpoint."""
    s = np.sort(ref)
    i = int(np.argmax(np.diff(s)))
    assert s[i + 1] - s[i] > 1e-4 * s[i + 1]
    return 0.5 * (s[i] + s[i + 1])


def _flags(ref, target):
    return [int(c < target) for c in ref]


@pytest.mark.parametrize("name", NAMES)
def test_gradient_and_loss_parity(gpu, name):
    _, _, models = hc.data(name)
    out, loss = _grad(gpu, name, models)
    g, l = out.cpu().numpy(), loss.cpu().numpy()
    worst = max(_assert_parity(name, g[d], l[d], d) for d in range(D))
    print(name, "worst normwise error over devices and tensors", worst)
    # and it is not the cross-entropy gradient
    xent, xloss = _grad(gpu, name, models, loss_kind="xent")
    assert not (_bits(xent) == _bits(out)).all(axis=1).any() and not (_bits(xloss) == _bits(loss)).any()


@pytest.mark.parametrize("per_device", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_validation_cost_flags_and_skip(gpu, name, per_device):
    _, _, models = hc.data(name)
    ref = hc.costs(name, per_device)
    target = _gap_target(ref)
    want = _flags(ref, target)
    assert 0 < sum(want) < D
    W = _stack(models)
    val = _validation(gpu, name, per_device, target=target, loss="huber")
    ended = torch.zeros(D, dtype=torch.int32, device="cuda")
    cost = val.validate(W, ended=ended).clone()
    got = cost.cpu().numpy()
    print(name, per_device, "cost", got, "max rel err", np.max(np.abs(got - ref)) / np.max(np.abs(ref)))
    assert normwise_close(got, ref, 1e-5)
    assert ended.cpu().numpy().tolist() == want
    # skip: a flagged device's cost and flag stay; skip and ended are one tensor, as a population's
    below = want.index(1)
    flagged = (below + 1) % D
    flags = np.zeros(D, dtype=np.int32)
    flags[flagged] = 1
    both = _cuda(flags)
    val.val_cost.fill_(SENTINEL)
    val.validate(W, skip=both, ended=both)
    after = val.val_cost.cpu().numpy()
    assert after[flagged] == SENTINEL
    others = [d for d in range(D) if d != flagged]
    assert (_bits(val.val_cost)[others] == _bits(cost)[others]).all()
    assert both.cpu().numpy().tolist() == [1 if d == flagged else want[d] for d in range(D)]
    # a flag that only skip carries: the device's flag in `ended` is not raised though it would be
    only = np.zeros(D, dtype=np.int32)
    only[below] = 1
    ended = torch.zeros(D, dtype=torch.int32, device="cuda")
    val.validate(W, skip=_cuda(only), ended=ended)
    assert ended.cpu().numpy().tolist() == [0 if d == below else want[d] for d in range(D)]


@pytest.mark.parametrize("name", NAMES)
def test_loss_is_the_validation_kernels_batch_loss(gpu, name):
    """The shared forward and loss phase: loss[d] has the bits of float32(val_cost[d]) of a
    one-batch validation on the same samples."""
    _, _, models = hc.data(name)
    _, loss = _grad(gpu, name, models)
    cost = _validation(gpu, name, batches=1, loss="huber").validate(_stack(models)).cpu().numpy()
    assert (cost.astype(np.float32).view(np.uint32) == _bits(loss)).all()
    assert (cost.astype(np.float32).astype(np.float64) == cost).all()  # one fp32 batch loss, widened


def test_src_evaluates_another_row_on_the_devices_own_data(gpu):
    name = "lenet1"
    _, _, models = hc.data(name)
    x, labels = hc.per_device(name)
    src = [1, 2, 0]
    out, loss = _grad(gpu, name, models, x, labels, src=_cuda(np.array(src, dtype=np.int32)))
    g, l = out.cpu().numpy(), loss.cpu().numpy()
    for d in range(D):
        _assert_parity(name, g[d], l[d], src[d], shift=hc.shifts(name)[d], what="src")
    plain, _ = _grad(gpu, name, models, x, labels)
    assert not (_bits(out) == _bits(plain)).all(axis=1).any()
    tr = _training(gpu, name, per_device=True, loss="huber")
    assert (_bits(tr.gradients(_stack(models), src=src)) == _bits(out)).all()
    assert (_bits(tr.loss) == _bits(loss)).all()


@pytest.mark.parametrize("name", ["lenet1", "pool2_drops"])
def test_first_selects_each_devices_batch_and_wraps(gpu, name):
    _, batch, Nt, _ = hc.CASES[name]
    _, _, models = hc.data(name)
    first = hc.firsts(name)
    assert first[2] % Nt + batch > Nt and first[1] >= Nt  # one wraps, one lies a set further
    out, loss = _grad(gpu, name, models, first=_cuda(np.array(first, dtype=np.int64)))
    g, l = out.cpu().numpy(), loss.cpu().numpy()
    for d in range(D):
        _assert_parity(name, g[d], l[d], d, first=first[d], what="first")
    zero, _ = _grad(gpu, name, models)
    assert not (_bits(out) == _bits(zero)).all(axis=1).any()


@pytest.mark.parametrize("name", ["lenet1", "finish_256"])
def test_a_per_device_set_matches_the_reference_of_its_own_samples(gpu, name):
    _, _, models = hc.data(name)
    tr = _training(gpu, name, per_device=True, loss="huber")
    g = tr.gradients(_stack(models)).cpu().numpy()
    l = tr.loss.cpu().numpy()
    for d in range(D):
        _assert_parity(name, g[d], l[d], d, shift=hc.shifts(name)[d], what="own set")


@pytest.mark.parametrize("name", ["lenet1", "pool2_drops"])
def test_a_row_does_not_depend_on_its_place(gpu, name):
    _, _, models = hc.data(name)
    out, loss = _grad(gpu, name, models)
    again, aloss = _grad(gpu, name, models)
    assert (_bits(again) == _bits(out)).all() and (_bits(aloss) == _bits(loss)).all()  # deterministic
    for d in range(D):  # alone
        one, oloss = _grad(gpu, name, models[d:d + 1])
        assert (_bits(one[0]) == _bits(out[d])).all() and _bits(oloss)[0] == _bits(loss)[d]
    perm = np.roll(np.arange(D), 1)  # row i of the permuted stack holds model perm[i]
    moved, mloss = _grad(gpu, name, models[perm])
    assert (_bits(moved) == _bits(out)[perm]).all() and (_bits(mloss) == _bits(loss)[perm]).all()


def test_captured_epoch_replays_the_eager_one(gpu):
    """validate -> epoch of 2 batches with Adam and clipnorm -> pop.rounds(1), all on the Huber
    objective, captured once after allocate and replayed twice: the bits of the same two eager
    epochs. Device 1 has ended from the start."""
    from federated_amd import topology as T
    from federated_amd._graphs import RoundGraphs
    from federated_amd.local_optim import PopulationOptimizer
    from federated_amd.tf2_validation import lenet_layer_shapes
    name, steps = hc.CAPTURED
    assert steps == 4
    geom, batch, Nt, _ = hc.CASES[name]
    _, _, models = hc.data(name)
    lists = [[(d - 1) % D, (d + 1) % D] for d in range(D)]

    def run(graph):
        pop = T.PopulationRound(gpu, _stack(models), _stack(np.zeros_like(models)))
        pop.set_topology(lists, T.alphas_tf2)
        pop.set_ended_rule("copy", propagate=False)
        pop.set_ended([1])
        val = _validation(gpu, name, target=1e-3, log_cap=2, loss="huber").allocate(D)
        tr = _training(gpu, name, loss="huber").allocate(D)
        opt = PopulationOptimizer(gpu, D, lenet_layer_shapes(geom), "adam", 1e-3, clipnorm=1.0)

        def step():
            val.validate(pop.models, skip=pop.ended, ended=pop.ended)
            tr.epoch(pop.models, opt, 2, skip=pop.ended)
            pop.rounds(1)

        if graph:
            RoundGraphs(pop.models.device, step, 1, lambda: 0).run(2)
        else:
            step()
            step()
        torch.cuda.synchronize()
        return (_bits(pop.models), _bits(tr.grads), _bits(tr.loss), _bits(val.val_cost), _bits(val.val_log),
                tr.cursor.cpu().numpy().tolist(), opt.steps_done.tolist(), pop.ended.cpu().numpy().tolist())

    eager, replay = run(False), run(True)  # eager first: it also loads every torch kernel the capture uses
    assert eager[5] == replay[5] == [4 * batch % Nt, 0, 4 * batch % Nt]
    assert eager[6] == replay[6] == [4, 0, 4] and eager[7] == replay[7] == [0, 1, 0]
    for a, b in zip(eager[:5], replay[:5]):
        assert (a == b).all()
    assert not (eager[0][0] == models.view(np.uint32)[0]).all()
    # and the chain ran on the Huber objective: its last loss is not the cross-entropy chain's
    assert eager[2].view(np.float32)[0] < 1.2  # a Huber batch loss of this set; -log p is above 1.8 here


@pytest.mark.parametrize("name", ["lenet1", "pool2_drops"])
def test_cross_entropy_is_the_default_and_untouched(gpu, name):
    """loss="xent" gives the bits of omitting it, for both classes and for the Engine, and the bits of
    the entry points that take no loss."""
    from federated_amd import _lib
    geom, batch, Nt, _ = hc.CASES[name]
    x, labels, models = hc.data(name)
    W = _stack(models)
    plain = _training(gpu, name)
    named = _training(gpu, name, loss="xent")
    assert plain.loss_kind == named.loss_kind == "xent"
    g0, g1 = plain.gradients(W).clone(), named.gradients(W).clone()
    assert (_bits(g0) == _bits(g1)).all() and (_bits(plain.loss) == _bits(named.loss)).all()
    # cfa_lenet_grad_f32 itself, which the Python no longer calls
    xs, ls = _cuda(x), _cuda(labels)
    out = torch.full((D, g0.stride(0)), SENTINEL, dtype=torch.float32, device="cuda")
    loss = torch.full((D,), SENTINEL, dtype=torch.float32, device="cuda")
    _lib.call("cfa_lenet_grad_f32", xs.data_ptr(), 0, ls.data_ptr(), 0, Nt, *geom, W.data_ptr(), int(W.stride(0)), D,
              None, None, batch, None, out.data_ptr(), int(out.stride(0)), loss.data_ptr(),
              plain.workspace.data_ptr(), plain.workspace.numel() * 4, None)
    torch.cuda.synchronize()
    assert (_bits(out[:, :plain.P]) == _bits(g0)).all() and (_bits(loss) == _bits(plain.loss)).all()
    assert not (_bits(_training(gpu, name, loss="huber").gradients(W)) == _bits(g0)).all(axis=1).any()
    v0 = _validation(gpu, name).validate(W).clone()
    vnamed = _validation(gpu, name, loss="xent")
    v1 = vnamed.validate(W).clone()
    assert (_bits(v0) == _bits(v1)).all()
    cost = torch.full((D,), SENTINEL, dtype=torch.float64, device="cuda")
    _lib.call("cfa_lenet_eval_f32", xs.data_ptr(), 0, ls.data_ptr(), 0, Nt, *geom, W.data_ptr(), int(W.stride(0)), D,
              batch, hc.VAL_BATCHES, None, 0.0, None, cost.data_ptr(), None, 0, None, vnamed.workspace.data_ptr(),
              vnamed.workspace.numel() * 4, None)
    torch.cuda.synchronize()
    assert (_bits(cost) == _bits(v0)).all()
    assert not (_bits(_validation(gpu, name, loss="huber").validate(W)) == _bits(v0)).any()


@pytest.mark.parametrize("name", ["lenet1", "lanes_64"])
def test_a_label_out_of_range_gives_that_device_nan(gpu, name):
    geom, batch, Nt, _ = hc.CASES[name]
    x, labels, models = hc.data(name)
    own = np.stack([labels] * D)
    own[1, batch - 1] = -1  # device 1's last sample of the batch
    plain, ploss = _grad(gpu, name, models)
    out, loss = _grad(gpu, name, models, np.stack([x] * D), own)
    assert np.isnan(out[1].cpu().numpy()).all() and np.isnan(float(loss[1]))
    for d in (0, 2):
        assert np.isfinite(out[d].cpu().numpy()).all()
        assert (_bits(out[d]) == _bits(plain[d])).all() and _bits(loss)[d] == _bits(ploss)[d]
    # the validation cost of that device is NaN too, the others' finite
    from federated_amd.tf2_validation import LenetValidation
    cost = torch.zeros(D, dtype=torch.float64, device="cuda")
    gpu.lenet_eval(geom, _cuda(np.stack([x] * D)), _cuda(own), _stack(models), batch, 1, cost,
                   gpu.lenet_workspace(D, 1), loss="huber")
    c = cost.cpu().numpy()
    assert np.isnan(c[1]) and np.isfinite(c[[0, 2]]).all()
    with pytest.raises(ValueError, match="labels"):
        LenetValidation(gpu, geom, _cuda(np.stack([x] * D)), _cuda(own), batch, 1, loss="huber")


def test_the_engine_refuses_an_unknown_loss_before_any_launch(gpu):
    name = "pool2_drops"
    geom, batch, Nt, _ = hc.CASES[name]
    x, labels, models = hc.data(name)
    xs, ls, W = _cuda(x), _cuda(labels), _stack(models)
    P = W.shape[1]
    grads = torch.full((D, P), SENTINEL, dtype=torch.float32, device="cuda")
    cost = torch.full((D,), SENTINEL, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="loss"):
        gpu.lenet_grad(geom, xs, ls, W, batch, grads, gpu.lenet_grad_workspace(D, batch, geom), loss_kind="l2")
    with pytest.raises(ValueError, match="loss"):
        gpu.lenet_eval(geom, xs, ls, W, batch, 2, cost, gpu.lenet_workspace(D, 2), loss="l2")
    with pytest.raises(ValueError, match="loss"):
        _training(gpu, name, loss="l2")
    with pytest.raises(ValueError, match="loss"):
        _validation(gpu, name, loss="l2")
    torch.cuda.synchronize()
    assert (grads.cpu().numpy() == SENTINEL).all() and (cost.cpu().numpy() == SENTINEL).all()
