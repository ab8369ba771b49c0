"""The max-pool CNNs of the TF2 drivers on the device (cfa_lenet_max_eval_loss_f32,
cfa_lenet_max_grad_loss_f32, `pool="max"` on Engine.lenet_eval / lenet_grad, LenetValidation and
LenetTraining) against the fp64 restatement of tests/lenet_max_cases.py, whose docstring has the
cases, the seed rule that makes a 1e-5 comparison of gradients meaningful and the launch plan
(`path`) each case exists for; test_lenet_max_host.py pins the restatement and the seeds."""
import numpy as np
import pytest
import torch

import lenet_cases as lc
import lenet_grad_cases as gc
import lenet_max_cases as mc
from conftest import normwise_close

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
E2E = (mc.MNIST_CNN14, 2, 2, 4, 932)  # geometry, batch, Nt, D, seed: the end-to-end population (the seed rule holds)


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
    """One Engine.lenet_grad call at pool="max" on the case's set (or x / labels): (grads [n, pitch], loss [n])."""
    geom, batch = mc.CASES[name][:2]
    x0, l0, _ = mc.data(name)
    xs, ls = _cuda(x0 if x is None else x), _cuda(l0 if labels is None else labels)
    W = _stack(models)
    n, P = W.shape
    out = torch.full((n, (P + 3) // 4 * 4 + 3), SENTINEL, dtype=torch.float32, device="cuda")
    loss = torch.full((n,), SENTINEL, dtype=torch.float32, device="cuda")
    ws = gpu.lenet_grad_workspace(n, batch, geom, "max")
    gpu.lenet_grad(geom, xs, ls, W, batch, out[:, :P], ws, loss, loss_kind=loss_kind, pool="max", **kw)
    torch.cuda.synchronize()
    return out, loss


def _validation(gpu, name, batch, batches, **kw):
    from federated_amd.tf2_validation import LenetValidation
    geom = (mc.CASES.get(name) or mc.EVAL_CASES[name])[0]
    x, labels, _ = mc.data(name)
    return LenetValidation(gpu, geom, _cuda(x), _cuda(labels), batch, batches, pool="max", **kw)


def _training(gpu, name, per_device=False, loss="xent"):
    from federated_amd.tf2_training import LenetTraining
    geom, batch = mc.CASES[name][:2]
    x, labels = mc.per_device(name) if per_device else mc.data(name)[:2]
    return LenetTraining(gpu, geom, _cuda(x), _cuda(labels), batch, loss=loss, pool="max")


def _assert_parity(name, got_row, got_loss, model, first=0, shift=0, loss="xent", what=""):
    geom = mc.CASES[name][0]
    ref, ref_loss = mc.reference(name, model, first, shift, loss)
    for i, (a, b) in enumerate(zip(gc.tensors(got_row, geom), gc.tensors(ref, geom))):
        err = np.max(np.abs(a.astype(np.float64) - b)) / np.max(np.abs(b))
        print(name, loss, what, "model", model, "first", first, "tensor", i, "normwise error", err)
        assert normwise_close(a, b, rtol=1e-5), (name, loss, what, model, i, err)
    print(name, loss, what, "model", model, "loss", got_loss, "error", abs(got_loss - ref_loss))
    assert abs(float(got_loss) - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))


def _val_shapes():
    out = [(n, c[1], c[2] // c[1]) for n, c in mc.CASES.items()]
    return out + [(n, c[1], c[2]) for n, c in mc.EVAL_CASES.items()]


@pytest.mark.parametrize("loss", mc.LOSSES)
@pytest.mark.parametrize("name, batch, batches", _val_shapes(), ids=[v[0] for v in _val_shapes()])
def test_validation_cost_parity(gpu, name, batch, batches, loss):
    for text, ok in mc.path(name).items():
        assert ok, (name, text)
    models = mc.data(name)[2]
    ref = mc.costs(name, batch, batches, loss)
    val = _validation(gpu, name, batch, batches, loss=loss)
    cost = val.validate(_stack(models)).cpu().numpy()
    print(name, loss, "cost", cost, "normwise error", np.max(np.abs(cost - ref)) / np.max(np.abs(ref)))
    assert cost.dtype == np.float64 and normwise_close(cost, ref, rtol=1e-5)
    again = val.validate(_stack(models)).cpu().numpy()
    assert (again.view(np.uint64) == cost.view(np.uint64)).all()  # deterministic


@pytest.mark.parametrize("loss", mc.LOSSES)
@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_gradient_and_loss_parity(gpu, name, loss):
    D = mc.CASES[name][3]
    models = mc.data(name)[2]
    P = models.shape[1]
    out, lossv = _grad(gpu, name, models, loss_kind=loss)
    g, l = out.cpu().numpy(), lossv.cpu().numpy()
    for d in range(D):
        _assert_parity(name, g[d, :P], l[d], d, loss=loss)
    assert (g[:, P:] == SENTINEL).all()  # the rows' padding is not written
    again, aloss = _grad(gpu, name, models, loss_kind=loss)
    assert (_bits(again) == _bits(out)).all() and (_bits(aloss) == _bits(lossv)).all()  # two identical calls


def test_flags_and_log_as_the_average_pool_pass_keeps_them(gpu):
    name, batch, batches = "generic_k", 5, 2
    models = mc.data(name)[2]
    D = len(models)
    ref = mc.costs(name, batch, batches)
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


@pytest.mark.parametrize("loss", mc.LOSSES)
@pytest.mark.parametrize("name", ["pool2_drops", "generic_k", "two_groups"])
def test_a_row_does_not_depend_on_its_place(gpu, name, loss):
    D = mc.CASES[name][3]
    models = mc.data(name)[2]
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


def test_src_and_first(gpu):
    name = "generic_k"
    geom, batch, Nt, D, _ = mc.CASES[name]
    models = mc.data(name)[2]
    P = models.shape[1]
    x, labels = mc.per_device(name)  # device d's set: the shared one rolled by d
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


@pytest.mark.parametrize("loss", mc.LOSSES)
@pytest.mark.parametrize("name", ["generic_k", "two_groups", "cnn32"])
def test_loss_is_the_validation_kernels_batch_loss(gpu, name, loss):
    """loss[d] has the bits of float32(val_cost[d]) of one validation batch, whatever the two chunks are."""
    batch = mc.CASES[name][1]
    models = mc.data(name)[2]
    _, lossv = _grad(gpu, name, models, loss_kind=loss)
    cost = _validation(gpu, name, batch, 1, loss=loss).validate(_stack(models)).cpu().numpy()
    assert (cost.astype(np.float32).view(np.uint32) == _bits(lossv)).all()
    assert (cost.astype(np.float32).astype(np.float64) == cost).all()


@pytest.mark.parametrize("name", ["pool2_drops", "two_groups"])
def test_a_label_out_of_range_gives_that_device_nan(gpu, name):
    geom, batch, Nt, D, _ = mc.CASES[name]
    x, labels, models = mc.data(name)
    P = models.shape[1]
    own = np.stack([labels] * D)
    own[1, batch - 1] = geom[4]  # device 1's last sample of the batch
    plain, ploss = _grad(gpu, name, models)
    out, loss = _grad(gpu, name, models, np.stack([x] * D), own)
    assert np.isnan(out[1, :P].cpu().numpy()).all() and np.isnan(float(loss[1]))
    for d in (0, 2):
        assert (_bits(out[d]) == _bits(plain[d])).all() and _bits(loss)[d] == _bits(ploss)[d]
    cost = torch.zeros(D, dtype=torch.float64, device="cuda")
    ws = gpu.lenet_workspace(D, 1, "max")
    gpu.lenet_eval(geom, _cuda(np.stack([x] * D)), _cuda(own), _stack(models), batch, 1, cost, ws, pool="max")
    c = cost.cpu().numpy()
    assert np.isnan(c[1]) and np.isfinite(c[[0, 2]]).all()


def test_refusals_leave_the_outputs_untouched(gpu):
    from federated_amd import _lib
    name = "pool2_drops"
    geom, batch, Nt, D, _ = mc.CASES[name]
    x, labels, models = mc.data(name)
    xs, ls, W = _cuda(x), _cuda(labels), _stack(models)
    P = lc.size(geom)
    grads = torch.full((D, P), SENTINEL, dtype=torch.float32, device="cuda")
    loss = torch.full((D,), SENTINEL, dtype=torch.float32, device="cuda")
    cost = torch.full((D,), SENTINEL, dtype=torch.float64, device="cuda")
    gws, ews = gpu.lenet_grad_workspace(D, batch, geom, "max"), gpu.lenet_workspace(D, 2, "max")

    def grad(fn="cfa_lenet_max_grad_loss_f32", g=geom, pitch=int(W.stride(0)), gpitch=P, ws_bytes=gws.numel() * 4, kind=0):
        _lib.call(fn, xs.data_ptr(), 0, ls.data_ptr(), 0, Nt, *g, W.data_ptr(), pitch, D, None, None, batch, None,
                  grads.data_ptr(), gpitch, loss.data_ptr(), gws.data_ptr(), ws_bytes, kind, None)

    def evaluate(fn="cfa_lenet_max_eval_loss_f32", g=geom, pitch=int(W.stride(0)), ws_bytes=ews.numel() * 4, kind=0):
        _lib.call(fn, xs.data_ptr(), 0, ls.data_ptr(), 0, Nt, *g, W.data_ptr(), pitch, D, batch, 2, None, 0.0, None,
                  cost.data_ptr(), None, 0, None, ews.data_ptr(), ws_bytes, kind, None)

    assert gws.numel() * 4 == mc.grad_workspace_bytes(geom, batch, D) and ews.numel() * 4 == 4 * D * 2
    for call in (grad, evaluate):
        for kw, code in ((dict(g=geom[:4] + (65,), pitch=1 << 20), _lib.CFA_E_UNSUPPORTED),
                         (dict(ws_bytes=(gws if call is grad else ews).numel() * 4 - 1), _lib.CFA_E_INVALID),
                         (dict(kind=2), _lib.CFA_E_INVALID)):
            if call is grad and "pitch" in kw:
                kw = dict(kw, gpitch=1 << 20)
            with pytest.raises(_lib.CFAError) as e:
                call(**kw)
            assert e.value.code == code, kw
    # the average-pool entries still refuse the drivers' max-pool geometry, not approximate it
    big = lc.UNSUPPORTED
    xb = torch.zeros(4, 28, 28, device="cuda")
    lb = torch.zeros(4, dtype=torch.int32, device="cuda")
    Wb = torch.zeros(D, lc.size(big), device="cuda")
    gb = torch.full((D, lc.size(big)), SENTINEL, device="cuda")
    wsb = gpu.lenet_grad_workspace(D, 2, big)
    for pool, ok in (("avg", False), ("max", True)):
        costb = torch.full((D,), SENTINEL, dtype=torch.float64, device="cuda")
        if ok:
            gpu.lenet_eval(big, xb, lb, Wb, 2, 2, costb, gpu.lenet_workspace(D, 2, pool), pool=pool)
            gpu.lenet_grad(big, xb, lb, Wb, 2, gb, gpu.lenet_grad_workspace(D, 2, big, pool), pool=pool)
            torch.cuda.synchronize()
            assert np.allclose(costb.cpu().numpy(), np.log(10.0)) and (gb.cpu().numpy() != SENTINEL).all()
        else:
            with pytest.raises(_lib.CFAError) as e:
                gpu.lenet_eval(big, xb, lb, Wb, 2, 2, costb, gpu.lenet_workspace(D, 2, pool), pool=pool)
            assert e.value.code == _lib.CFA_E_UNSUPPORTED
            with pytest.raises(_lib.CFAError) as e:
                gpu.lenet_grad(big, xb, lb, Wb, 2, gb, wsb, pool=pool)
            assert e.value.code == _lib.CFA_E_UNSUPPORTED
            torch.cuda.synchronize()
            assert (costb.cpu().numpy() == SENTINEL).all() and (gb.cpu().numpy() == SENTINEL).all()
    torch.cuda.synchronize()
    assert (grads.cpu().numpy() == SENTINEL).all() and (loss.cpu().numpy() == SENTINEL).all()
    assert (cost.cpu().numpy() == SENTINEL).all()
    for bad in ("min", None):
        with pytest.raises(ValueError, match="pool"):
            gpu.lenet_grad(geom, xs, ls, W, batch, grads, gws, pool=bad)
        with pytest.raises(ValueError, match="pool"):
            gpu.lenet_eval(geom, xs, ls, W, batch, 2, cost, ews, pool=bad)
        with pytest.raises(ValueError, match="pool"):
            gpu.lenet_workspace(D, 2, bad)
    # and the good calls run
    grad()
    evaluate()
    torch.cuda.synchronize()
    assert (grads.cpu().numpy() != SENTINEL).all() and (cost.cpu().numpy() != SENTINEL).all()


def _optimizer(gpu, geom, D):
    from federated_amd.local_optim import PopulationOptimizer
    from federated_amd.tf2_validation import lenet_layer_shapes
    return PopulationOptimizer(gpu, D, lenet_layer_shapes(geom), "adam", 1e-3, clipnorm=1.0)


@pytest.mark.parametrize("loss", mc.LOSSES)
def test_captured_epoch_replays_the_eager_one(gpu, loss):
    """validate -> epoch of 2 batches -> pop.rounds(1) at pool="max", captured once after allocate and
    replayed twice: the bits of the same two eager epochs. Device 1 has ended from the start."""
    from federated_amd import topology as T
    from federated_amd._graphs import RoundGraphs
    name = "generic_k"
    geom, batch, Nt, D, _ = mc.CASES[name]
    models = mc.data(name)[2]
    lists = [[(d - 1) % D, (d + 1) % D] for d in range(D)]

    def run(graph):
        pop = T.PopulationRound(gpu, _stack(models), _stack(np.zeros_like(models)))
        pop.set_topology(lists, T.alphas_tf2)
        pop.set_ended_rule("copy", propagate=False)
        pop.set_ended([1])
        val = _validation(gpu, name, batch, 2, target=1e-3, loss=loss).allocate(D)
        tr, opt = _training(gpu, name, loss=loss).allocate(D), _optimizer(gpu, geom, D)

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
        return (_bits(pop.models), _bits(tr.grads), _bits(tr.loss), _bits(val.val_cost.float()),
                tr.cursor.cpu().numpy().tolist(), opt.steps_done.tolist(), pop.ended.cpu().numpy().tolist())

    eager, replay = run(False), run(True)  # eager first: it also loads every torch kernel the capture uses
    assert eager[4] == replay[4] == [4 * batch % Nt, 0, 4 * batch % Nt]
    assert eager[5] == replay[5] == [4, 0, 4] and eager[6] == replay[6] == [0, 1, 0]
    for a, b in zip(eager[:4], replay[:4]):
        assert (a == b).all()
    assert not (eager[0][0] == models.view(np.uint32)[0]).all()


def test_a_cnn14_population_trains_end_to_end(gpu):
    """D = 4 MNIST_CNN14 models on a ring: two epochs of validate / train.epoch / rounds(1) run and
    leave finite models; after the first batch the models equal those of the same optimizer step
    fed the restatement's gradient rows, 1e-5 normwise (later batches compound)."""
    from federated_amd import topology as T
    geom, batch, Nt, D, seed = E2E
    assert mc.meets_the_seed_rule(geom, batch, Nt, D, seed)
    x, labels, models = lc.make(geom, D, Nt, seed)
    from federated_amd.tf2_training import LenetTraining
    from federated_amd.tf2_validation import LenetValidation
    ref = np.stack([mc.grads(x[:batch], labels[:batch], row, geom)[0] for row in models]).astype(np.float32)
    after = []
    for restated in (False, True):
        W, opt = _stack(models), _optimizer(gpu, geom, D)
        tr = LenetTraining(gpu, geom, _cuda(x), _cuda(labels), batch, pool="max").allocate(D)
        g = tr.gradients(W)
        if restated:
            g.copy_(_cuda(ref))
        opt.step(W, g, None)
        after.append(W.cpu().numpy())
    moved = after[0] - models
    assert np.abs(moved).max() > 0
    for d in range(D):
        for a, b in zip(gc.tensors(after[0][d], geom), gc.tensors(after[1][d], geom)):
            assert normwise_close(a, b, rtol=1e-5)
    pop = T.PopulationRound(gpu, _stack(models), _stack(np.zeros_like(models)))
    pop.set_topology([[(d - 1) % D, (d + 1) % D] for d in range(D)], T.alphas_tf2)
    pop.set_ended_rule("copy", propagate=False)
    val = LenetValidation(gpu, geom, _cuda(x), _cuda(labels), batch, 1, target=1e-3, pool="max").allocate(D)
    tr = LenetTraining(gpu, geom, _cuda(x), _cuda(labels), batch, pool="max").allocate(D)
    opt = _optimizer(gpu, geom, D)
    for _ in range(2):
        val.validate(pop.models, skip=pop.ended, ended=pop.ended)
        tr.epoch(pop.models, opt, 2, skip=pop.ended)
        pop.rounds(1)
    torch.cuda.synchronize()
    out = pop.models.cpu().numpy()
    assert np.isfinite(out).all() and np.isfinite(val.val_cost.cpu().numpy()).all()
    assert not (out == models).all(axis=1).any() and pop.ended.cpu().numpy().tolist() == [0] * D
