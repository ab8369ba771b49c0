"""The CIFAR drivers' hidden-layer LeNet on the device (cfa_lenet_hidden_eval_loss_f32,
cfa_lenet_hidden_grad_loss_f32, a seven-number geometry on Engine.lenet_eval / lenet_grad,
LenetValidation and LenetTraining) against the fp64 restatement of tests/lenet_hidden_cases.py, whose
docstring has the cases, the seed rule that makes a 1e-5 comparison of gradients meaningful and the
launch plan (`path`) each case exists for; test_lenet_hidden_host.py pins the restatement and the seeds.
The tolerances are the max-pool tests': 1e-5 normwise per tensor, the loss within 1e-5 max(1, |ref|)."""
import numpy as np
import pytest
import torch

import lenet_cases as lc
import lenet_hidden_cases as hc
from conftest import normwise_close

pytestmark = pytest.mark.gpu

SENTINEL = -7.25


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()  # a copy: the shared reference data is read only


def _stack(models):
    """The models as a [D, P] CUDA view of a stack whose rows are pitched to 16 bytes; the padding is NaN."""
    n, P = models.shape
    full = torch.full((n, (P + 3) // 4 * 4), float("nan"), dtype=torch.float32, device="cuda")
    full[:, :P] = _cuda(models)
    return full[:, :P]


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _grad(gpu, name, models, x=None, labels=None, loss_kind="xent", **kw):
    """One Engine.lenet_grad call on the case's set (or x / labels): (grads [n, pitch + 3], loss [n]);
    the output's pitch differs from the models'."""
    geom, batch = hc.CASES[name][:2]
    x0, l0, _ = hc.data(name)
    xs, ls = _cuda(x0 if x is None else x), _cuda(l0 if labels is None else labels)
    W = _stack(models)
    n, P = W.shape
    out = torch.full((n, (P + 3) // 4 * 4 + 3), SENTINEL, dtype=torch.float32, device="cuda")
    loss = torch.full((n,), SENTINEL, dtype=torch.float32, device="cuda")
    ws = gpu.lenet_grad_workspace(n, batch, geom)
    gpu.lenet_grad(geom, xs, ls, W, batch, out[:, :P], ws, loss, loss_kind=loss_kind, **kw)
    torch.cuda.synchronize()
    return out, loss


def _validation(gpu, name, batch, batches, **kw):
    from federated_amd.tf2_validation import LenetValidation
    geom = (hc.CASES.get(name) or hc.EVAL_CASES[name])[0]
    x, labels, _ = hc.data(name)
    return LenetValidation(gpu, geom, _cuda(x), _cuda(labels), batch, batches, **kw)


def _training(gpu, name, per_device=False, loss="xent"):
    from federated_amd.tf2_training import LenetTraining
    geom, batch = hc.CASES[name][:2]
    x, labels = hc.per_device(name) if per_device else hc.data(name)[:2]
    return LenetTraining(gpu, geom, _cuda(x), _cuda(labels), batch, loss=loss)


def _assert_parity(name, got_row, got_loss, model, first=0, shift=0, loss="xent", what=""):
    geom = hc.CASES[name][0]
    ref, ref_loss = hc.reference(name, model, first, shift, loss)
    for i, (a, b) in enumerate(zip(hc.tensors(got_row, geom), hc.tensors(ref, geom))):
        err = np.max(np.abs(a.astype(np.float64) - b)) / np.max(np.abs(b))
        print(name, loss, what, "model", model, "first", first, "tensor", i, "normwise error", err)
        assert normwise_close(a, b, rtol=1e-5), (name, loss, what, model, i, err)
    print(name, loss, what, "model", model, "loss", got_loss, "error", abs(got_loss - ref_loss))
    assert abs(float(got_loss) - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))


def _val_shapes():
    out = [(n, c[1], c[2] // c[1]) for n, c in hc.CASES.items()]
    return out + [(n, c[1], c[2]) for n, c in hc.EVAL_CASES.items()]


@pytest.mark.parametrize("loss", hc.LOSSES)
@pytest.mark.parametrize("name, batch, batches", _val_shapes(), ids=[v[0] for v in _val_shapes()])
def test_validation_cost_parity(gpu, name, batch, batches, loss):
    for text, ok in hc.path(name).items():
        assert ok, (name, text)
    models = hc.data(name)[2]
    ref = hc.costs(name, batch, batches, loss)
    val = _validation(gpu, name, batch, batches, loss=loss)
    cost = val.validate(_stack(models)).cpu().numpy()
    print(name, loss, "cost", cost, "normwise error", np.max(np.abs(cost - ref)) / np.max(np.abs(ref)))
    assert cost.dtype == np.float64 and normwise_close(cost, ref, rtol=1e-5)
    again = val.validate(_stack(models)).cpu().numpy()
    assert (again.view(np.uint64) == cost.view(np.uint64)).all()  # deterministic


@pytest.mark.parametrize("loss", hc.LOSSES)
@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_gradient_and_loss_parity(gpu, name, loss):
    D = hc.CASES[name][3]
    models = hc.data(name)[2]
    P = models.shape[1]
    out, lossv = _grad(gpu, name, models, loss_kind=loss)
    g, l = out.cpu().numpy(), lossv.cpu().numpy()
    for d in range(D):
        _assert_parity(name, g[d, :P], l[d], d, loss=loss)
    assert (g[:, P:] == SENTINEL).all()  # the rows' padding is not written
    again, aloss = _grad(gpu, name, models, loss_kind=loss)
    assert (_bits(again) == _bits(out)).all() and (_bits(aloss) == _bits(lossv)).all()  # two identical calls


def test_flags_and_log_as_the_family_keeps_them(gpu):
    name, batch, batches = "generic_k", 5, 2
    models = hc.data(name)[2]
    D = len(models)
    ref = hc.costs(name, batch, batches)
    target = float(np.sort(ref)[1:3].mean())  # the two cheapest devices end
    val = _validation(gpu, name, batch, batches, target=target, log_cap=2)
    ended = torch.zeros(D, dtype=torch.int32, device="cuda")
    W = _stack(models)
    cost = val.validate(W, ended=ended).cpu().numpy()
    assert ended.cpu().numpy().tolist() == lc.flags(ref, target).tolist() and sum(ended.cpu().numpy()) == 2
    # skip = ended: the ended devices keep cost and flag, the log takes their untouched cost
    val.val_cost.fill_(SENTINEL)
    before = ended.clone()
    val.validate(W, skip=ended, ended=ended)
    val.validate(W, skip=ended, ended=ended)  # a third call lands in the log's last row again
    c2 = val.val_cost.cpu().numpy()
    flags = before.cpu().numpy()
    assert (c2[flags == 1] == SENTINEL).all() and (c2[flags == 0].view(np.uint64) == cost[flags == 0].view(np.uint64)).all()
    assert (ended == before).all() and val.epochs_done == 3
    log = val.val_log.cpu().numpy()
    assert (log[0].view(np.uint64) == cost.view(np.uint64)).all() and (log[1] == c2).all()


@pytest.mark.parametrize("loss", hc.LOSSES)
@pytest.mark.parametrize("name", ["cin3_map1", "generic_k", "two_groups", "hidden_wide"])
def test_a_row_does_not_depend_on_its_place(gpu, name, loss):
    D = hc.CASES[name][3]
    models = hc.data(name)[2]
    P = models.shape[1]
    out, lossv = _grad(gpu, name, models, loss_kind=loss)
    for d in range(D):
        one, oloss = _grad(gpu, name, models[d:d + 1], loss_kind=loss)  # alone
        assert (_bits(one[0, :P]) == _bits(out[d, :P])).all() and _bits(oloss)[0] == _bits(lossv)[d]
        skip = np.ones(D, dtype=np.int32)
        skip[d] = 0  # in the population, its neighbours skipped
        only, sloss = _grad(gpu, name, models, loss_kind=loss, skip=_cuda(skip))
        assert (_bits(only[d]) == _bits(out[d])).all() and _bits(sloss)[d] == _bits(lossv)[d]
        others = [e for e in range(D) if e != d]
        assert (only[others].cpu().numpy() == SENTINEL).all() and (sloss[others].cpu().numpy() == SENTINEL).all()
    perm = np.roll(np.arange(D), 1)
    moved, mloss = _grad(gpu, name, models[perm], loss_kind=loss)
    assert (_bits(moved[:, :P]) == _bits(out[:, :P])[perm]).all() and (_bits(mloss) == _bits(lossv)[perm]).all()


@pytest.mark.parametrize("loss", hc.LOSSES)
def test_validation_cost_does_not_depend_on_the_population(gpu, loss):
    name, batch, batches = "generic_k", 5, 2
    geom = hc.CASES[name][0]
    x, labels, models = hc.data(name)
    D = len(models)
    cost = _validation(gpu, name, batch, batches, loss=loss).validate(_stack(models)).cpu().numpy()
    for d in range(D):
        one = _validation(gpu, name, batch, batches, loss=loss).validate(_stack(models[d:d + 1])).cpu().numpy()
        assert one.view(np.uint64)[0] == cost.view(np.uint64)[d]


def test_src_and_first(gpu):
    name = "generic_k"
    geom, batch, Nt, D, _ = hc.CASES[name]
    models = hc.data(name)[2]
    P = models.shape[1]
    x, labels = hc.per_device(name)  # device d's set: the shared one rolled by d
    src = [1, 2, 0]
    out, loss = _grad(gpu, name, models, x, labels, src=_cuda(np.array(src, dtype=np.int32)))
    g, l = out.cpu().numpy(), loss.cpu().numpy()
    for d in range(D):
        _assert_parity(name, g[d, :P], l[d], src[d], shift=d, what="src")
    # src[d] = r: the bits of row r evaluated in place r of a stack, on device d's data
    for d in range(D):
        xs, ls = np.stack([x[d]] * D), np.stack([labels[d]] * D)
        plain, ploss = _grad(gpu, name, models, xs, ls)
        assert (_bits(plain[src[d], :P]) == _bits(out[d, :P])).all() and _bits(ploss)[src[d]] == _bits(loss)[d]
    tr = _training(gpu, name, per_device=True)
    assert (_bits(tr.gradients(_stack(models), src=src)) == _bits(out[:, :P])).all()
    first = [2, 0, Nt - 1]  # the last one wraps after one sample
    out, loss = _grad(gpu, name, models, first=_cuda(np.array(first, dtype=np.int64)))
    g, l = out.cpu().numpy(), loss.cpu().numpy()
    for d in range(D):
        _assert_parity(name, g[d, :P], l[d], d, first=first[d], what="first")
    far, _ = _grad(gpu, name, models, first=_cuda(np.array(first, dtype=np.int64) + Nt))
    assert (_bits(far) == _bits(out)).all()


def test_an_out_of_range_src_gives_that_row_nan(gpu):
    """The existing contract of the family: nothing is read through such a value."""
    name = "cin3_map1"
    D = hc.CASES[name][3]
    models = hc.data(name)[2]
    P = models.shape[1]
    plain, ploss = _grad(gpu, name, models)
    out, loss = _grad(gpu, name, models, src=_cuda(np.array([0, D, 2], dtype=np.int32)))
    assert np.isnan(out[1, :P].cpu().numpy()).all() and np.isnan(float(loss[1]))
    for d in (0, 2):
        assert (_bits(out[d]) == _bits(plain[d])).all() and _bits(loss)[d] == _bits(ploss)[d]


@pytest.mark.parametrize("loss", hc.LOSSES)
@pytest.mark.parametrize("name", ["generic_k", "two_groups", "hidden_wide", "cifar"])
def test_loss_is_the_validation_kernels_batch_loss(gpu, name, loss):
    """loss[d] has the bits of float32(val_cost[d]) of one validation batch, whatever the two chunks are."""
    batch = hc.CASES[name][1]
    models = hc.data(name)[2]
    _, lossv = _grad(gpu, name, models, loss_kind=loss)
    cost = _validation(gpu, name, batch, 1, loss=loss).validate(_stack(models)).cpu().numpy()
    assert (cost.astype(np.float32).view(np.uint32) == _bits(lossv)).all()
    assert (cost.astype(np.float32).astype(np.float64) == cost).all()


def test_a_label_out_of_range_gives_that_device_nan(gpu):
    name = "two_groups"
    geom, batch, Nt, D, _ = hc.CASES[name]
    x, labels, models = hc.data(name)
    P = models.shape[1]
    own = np.stack([labels] * D)
    own[1, batch - 1] = geom[6]  # device 1's last sample of the batch
    plain, ploss = _grad(gpu, name, models)
    out, loss = _grad(gpu, name, models, np.stack([x] * D), own)
    assert np.isnan(out[1, :P].cpu().numpy()).all() and np.isnan(float(loss[1]))
    for d in (0, 2):
        assert (_bits(out[d]) == _bits(plain[d])).all() and _bits(loss)[d] == _bits(ploss)[d]
    cost = torch.zeros(D, dtype=torch.float64, device="cuda")
    ws = gpu.lenet_workspace(D, 1, geom=geom)
    gpu.lenet_eval(geom, _cuda(np.stack([x] * D)), _cuda(own), _stack(models), batch, 1, cost, ws)
    c = cost.cpu().numpy()
    assert np.isnan(c[1]) and np.isfinite(c[[0, 2]]).all()


def test_refusals_leave_the_outputs_untouched(gpu):
    from federated_amd import _lib
    name = "cin3_map1"
    geom, batch, Nt, D, _ = hc.CASES[name]
    x, labels, models = hc.data(name)
    xs, ls, W = _cuda(x), _cuda(labels), _stack(models)
    P = hc.size(geom)
    grads = torch.full((D, P), SENTINEL, dtype=torch.float32, device="cuda")
    loss = torch.full((D,), SENTINEL, dtype=torch.float32, device="cuda")
    cost = torch.full((D,), SENTINEL, dtype=torch.float64, device="cuda")
    gws, ews = gpu.lenet_grad_workspace(D, batch, geom), gpu.lenet_workspace(D, 2, geom=geom)
    assert gws.numel() * 4 == hc.grad_workspace_bytes(geom, batch, D) and ews.numel() * 4 == 4 * D * 2
    # one sample's state beyond the device's LDS (hc.TOO_LARGE, from the LDS formula): a clear refusal
    big = hc.TOO_LARGE
    assert hc.grad_lds_bytes(big, 1) > hc.LDS_LIMIT and hc.eval_lds_bytes(big, 1, 2) > hc.LDS_LIMIT
    xb = torch.zeros(2, big[0], big[0], big[1], device="cuda")
    lb = torch.zeros(2, dtype=torch.int32, device="cuda")
    Wb = torch.zeros(D, hc.size(big), device="cuda")
    gb = torch.full((D, hc.size(big)), SENTINEL, device="cuda")
    with pytest.raises(_lib.CFAError, match="do not fit one workgroup's LDS") as e:
        gpu.lenet_eval(big, xb, lb, Wb, 2, 1, cost, gpu.lenet_workspace(D, 1, geom=big))
    assert e.value.code == _lib.CFA_E_UNSUPPORTED
    with pytest.raises(_lib.CFAError, match="do not fit one workgroup's LDS") as e:
        gpu.lenet_grad(big, xb, lb, Wb, 2, gb, gpu.lenet_grad_workspace(D, 2, big))
    assert e.value.code == _lib.CFA_E_UNSUPPORTED
    # the wrapper's own refusals
    with pytest.raises(ValueError, match="pool"):
        gpu.lenet_grad(geom, xs, ls, W, batch, grads, gws, loss, pool="max")
    with pytest.raises(ValueError, match="pool"):
        gpu.lenet_eval(geom, xs, ls, W, batch, 2, cost, ews, pool="max")
    with pytest.raises(TypeError, match="channels"):
        gpu.lenet_grad(geom, xs[..., 0].contiguous(), ls, W, batch, grads, gws, loss)  # no channel axis
    with pytest.raises(ValueError, match="x and labels must be"):
        gpu.lenet_grad(geom, xs.permute(0, 3, 1, 2).contiguous(), ls, W, batch, grads, gws, loss)  # NCHW
    with pytest.raises(ValueError, match="row size"):
        gpu.lenet_eval(geom[:5] + (6,) + geom[6:], xs, ls, W, batch, 2, cost, ews)
    torch.cuda.synchronize()
    assert (grads.cpu().numpy() == SENTINEL).all() and (loss.cpu().numpy() == SENTINEL).all()
    assert (cost.cpu().numpy() == SENTINEL).all() and (gb.cpu().numpy() == SENTINEL).all()
    # and the good calls run
    gpu.lenet_grad(geom, xs, ls, W, batch, grads, gws, loss)
    gpu.lenet_eval(geom, xs, ls, W, batch, 2, cost, ews)
    torch.cuda.synchronize()
    assert (grads.cpu().numpy() != SENTINEL).all() and (cost.cpu().numpy() != SENTINEL).all()


def _optimizer(gpu, geom, D, lr):
    from federated_amd.local_optim import PopulationOptimizer
    from federated_amd.tf2_validation import lenet_layer_shapes
    return PopulationOptimizer(gpu, D, lenet_layer_shapes(geom), "adam", lr, clipnorm=1.0)


@pytest.mark.parametrize("loss", hc.LOSSES)
def test_three_epochs_as_the_drivers_run_them(gpu, loss):
    """hc.EPOCHS: val.validate -> train.epoch of 2 batches (Adam, clipnorm 1) -> one ended-aware round
    ("copy") on a ring, three times, every device on its own set, no flag at the start and the target of
    hc.epochs_target: the first epoch mixes all three rows, the second epoch's validation raises one flag,
    that device is skipped from there on and its neighbours copy its row. After the third epoch
    pop.models (per tensor), val_cost and the flags against hc.drivers_epochs, the whole sequence stepped
    in numpy fp64, at 1e-5 normwise; and the same sequence captured into a graph and replayed equals the
    eager run bit for bit."""
    from federated_amd import topology as T
    from federated_amd._graphs import RoundGraphs
    name, E = hc.EPOCHS["case"], hc.EPOCHS
    geom, batch, Nt, D, _ = hc.CASES[name]
    models = hc.data(name)[2]
    xs, ls = hc.per_device(name)
    target = hc.epochs_target(loss)
    want, want_cost, want_ended, history = hc.drivers_epochs(loss, target)
    assert [h[1].tolist() for h in history][0] == [0] * D and sum(history[1][1]) == 1  # the design holds
    lists = [[(d - 1) % D, (d + 1) % D] for d in range(D)]

    def run(graph):
        from federated_amd.tf2_training import LenetTraining
        from federated_amd.tf2_validation import LenetValidation
        pop = T.PopulationRound(gpu, _stack(models), _stack(np.zeros_like(models)))
        pop.set_topology(lists, T.alphas_tf2)
        pop.set_ended_rule("copy", propagate=False)
        val = LenetValidation(gpu, geom, _cuda(xs), _cuda(ls), batch, E["val_batches"], target=target,
                              loss=loss).allocate(D)
        tr = LenetTraining(gpu, geom, _cuda(xs), _cuda(ls), batch, loss=loss).allocate(D)
        opt = _optimizer(gpu, geom, D, E["lr"])

        def step():
            val.validate(pop.models, skip=pop.ended, ended=pop.ended)
            tr.epoch(pop.models, opt, E["steps"], skip=pop.ended)
            pop.rounds(1)

        if graph:
            RoundGraphs(pop.models.device, step, 1, lambda: 0).run(E["epochs"])
        else:
            for _ in range(E["epochs"]):
                step()
        torch.cuda.synchronize()
        return (pop.models.cpu().numpy(), tr.grads.cpu().numpy(), tr.loss.cpu().numpy(), val.val_cost.cpu().numpy(),
                tr.cursor.cpu().numpy().tolist(), opt.steps_done.tolist(), pop.ended.cpu().numpy().tolist())

    eager, replay = run(False), run(True)  # eager first: it also loads every torch kernel the capture uses
    got, cost = eager[0], eager[3]
    for d in range(D):
        for i, (a, b) in enumerate(zip(hc.tensors(got[d], geom), hc.tensors(want[d], geom))):
            print(loss, "device", d, "tensor", i, "normwise error", np.max(np.abs(a - b)) / np.max(np.abs(b)))
    print(loss, "cost", cost, "reference", want_cost, "normwise error",
          np.max(np.abs(cost - want_cost)) / np.max(np.abs(want_cost)))
    print(loss, "ended", eager[6], "reference", want_ended.tolist(), "steps", eager[5], "reference", history[-1][2].tolist())
    assert eager[6] == want_ended.tolist() and eager[5] == history[-1][2].tolist()
    assert eager[4] == [int(t) * batch % Nt for t in history[-1][2]]
    assert normwise_close(cost, want_cost, rtol=1e-5)
    for d in range(D):
        for a, b in zip(hc.tensors(got[d], geom), hc.tensors(want[d], geom)):
            assert normwise_close(a, b, rtol=1e-5), (loss, d)
    for a, b in zip(eager[:4], replay[:4]):
        assert (np.ascontiguousarray(a).view(np.uint8) == np.ascontiguousarray(b).view(np.uint8)).all()
    assert eager[4:] == replay[4:]
