"""The local batches of a TF2 LeNet-1 population on the device (cfa_lenet_grad_f32,
Engine.lenet_grad, tf2_training.LenetTraining) against the fp64 backward restatement of
tests/lenet_grad_cases.py (its docstring has the cases and the relu-gate margin that makes a 1e-5
comparison meaningful; test_lenet_training_host.py pins the restatement by torch's autograd).

Every case has D = 3 devices. LeNet-1 runs the compile-time kernel side with a batch of 6: one
full group of two chunks and a second group of one chunk; `generic_k` the runtime kernel side with
two groups and a partial chunk; the others the smallest geometries whose pools drop a row and
column or leave a 1 x 1 map, with a batch of 3 (one group, a full and a partial chunk)."""
import numpy as np
import pytest
import torch

import lenet_cases as lc
import lenet_grad_cases as gc
from conftest import normwise_close

pytestmark = pytest.mark.gpu

D = gc.D
SENTINEL = -7.25
NAMES = sorted(n for n in gc.CASES if n not in gc.PATHS)  # those: test_gpu_lenet_paths.py


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()  # a copy: the shared reference data is read only


def _stack(models, pitch=None):
    """The models as a [D, P] CUDA view of a stack whose rows are pitched to 16 bytes (2 204 floats
    for LeNet-1, as the populations keep them) or to `pitch`; the padding is NaN."""
    n, P = models.shape
    full = torch.full((n, pitch or (P + 3) // 4 * 4), float("nan"), dtype=torch.float32, device="cuda")
    full[:, :P] = _cuda(models)
    return full[:, :P]


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _grad(gpu, name, models, x=None, labels=None, pad=0, **kw):
    """One Engine.lenet_grad call on the case's set (or x / labels): (grads [n, P] view, loss [n])."""
    geom, batch, _, _ = gc.CASES[name]
    x0, l0, _ = gc.data(name)
    xs, ls = _cuda(x0 if x is None else x), _cuda(l0 if labels is None else labels)
    W = _stack(models)
    n, P = W.shape
    out = torch.full((n, (P + 3) // 4 * 4 + pad), SENTINEL, dtype=torch.float32, device="cuda")
    loss = torch.full((n,), SENTINEL, dtype=torch.float32, device="cuda")
    ws = gpu.lenet_grad_workspace(n, batch, geom)
    gpu.lenet_grad(geom, xs, ls, W, batch, out[:, :P], ws, loss, **kw)
    torch.cuda.synchronize()
    return out, loss


def _training(gpu, name, per_device=False):
    from federated_amd.tf2_training import LenetTraining
    geom, batch, _, _ = gc.CASES[name]
    x, labels = gc.per_device(name) if per_device else gc.data(name)[:2]
    return LenetTraining(gpu, geom, _cuda(x), _cuda(labels), batch)


def _assert_parity(name, got_row, got_loss, model, first=0, shift=0, what=""):
    geom = gc.CASES[name][0]
    ref, ref_loss = gc.reference(name, model, first, shift)
    worst = 0.0
    for i, (a, b) in enumerate(zip(gc.tensors(got_row, geom), gc.tensors(ref, geom))):
        err = np.max(np.abs(a.astype(np.float64) - b)) / np.max(np.abs(b))
        worst = max(worst, err)
        print(name, what, "model", model, "first", first, "tensor", i, "normwise error", err)
        assert normwise_close(a, b, rtol=1e-5), (name, what, model, i, err)
    print(name, what, "model", model, "loss", got_loss, "error", abs(got_loss - ref_loss), "worst tensor", worst)
    assert abs(float(got_loss) - ref_loss) <= 1e-5
    return worst


@pytest.mark.parametrize("name", NAMES)
def test_gradient_and_loss_parity(gpu, name):
    _, _, models = gc.data(name)
    P = models.shape[1]
    out, loss = _grad(gpu, name, models)
    assert out.stride(0) == (P + 3) // 4 * 4  # 2 204 for LeNet-1
    g, l = out.cpu().numpy(), loss.cpu().numpy()
    for d in range(D):
        _assert_parity(name, g[d, :P], l[d], d)
    assert (g[:, P:] == SENTINEL).all()
    # grads rows with a pitch well above P: the same bits, the padding untouched
    wide, wloss = _grad(gpu, name, models, pad=7)
    assert wide.stride(0) >= P + 7
    assert (_bits(wide[:, :P]) == _bits(out[:, :P])).all() and (_bits(wloss) == _bits(loss)).all()
    assert (wide[:, P:].cpu().numpy() == SENTINEL).all()


@pytest.mark.parametrize("name", ["lenet1", "generic_k", "pool1_drops"])
def test_loss_is_the_validation_kernels_batch_loss(gpu, name):
    """The shared forward: loss[d] has the bits of float32(val_cost[d]) of one validation batch."""
    from federated_amd.tf2_validation import LenetValidation
    geom, batch, _, _ = gc.CASES[name]
    x, labels, models = gc.data(name)
    _, loss = _grad(gpu, name, models)
    val = LenetValidation(gpu, geom, _cuda(x), _cuda(labels), batch, batches=1)
    cost = val.validate(_stack(models)).cpu().numpy()
    assert (cost.astype(np.float32).view(np.uint32) == _bits(loss)).all()
    assert (cost.astype(np.float32).astype(np.float64) == cost).all()  # one fp32 batch loss, widened


@pytest.mark.parametrize("name", ["lenet1", "generic_k"])
def test_a_row_does_not_depend_on_its_place(gpu, name):
    _, _, models = gc.data(name)
    P = models.shape[1]
    out, loss = _grad(gpu, name, models)
    again, _ = _grad(gpu, name, models)
    assert (_bits(again) == _bits(out)).all()  # deterministic
    for d in range(D):  # alone
        one, oloss = _grad(gpu, name, models[d:d + 1])
        assert (_bits(one[0, :P]) == _bits(out[d, :P])).all() and _bits(oloss)[0] == _bits(loss)[d]
    perm = np.roll(np.arange(D), 1)  # row i of the permuted stack holds model perm[i]
    moved, mloss = _grad(gpu, name, models[perm])
    assert (_bits(moved[:, :P]) == _bits(out[:, :P])[perm]).all() and (_bits(mloss) == _bits(loss)[perm]).all()


def test_src_evaluates_another_row_on_the_devices_own_data(gpu):
    name = "lenet1"
    _, _, models = gc.data(name)
    P = models.shape[1]
    x, labels = gc.per_device(name)  # device d's set: the shared one rolled by d
    src = [1, 2, 0]
    out, loss = _grad(gpu, name, models, x, labels, src=_cuda(np.array(src, dtype=np.int32)))
    g, l = out.cpu().numpy(), loss.cpu().numpy()
    for d in range(D):
        _assert_parity(name, g[d, :P], l[d], src[d], shift=d, what="src")
    plain, ploss = _grad(gpu, name, models, x, labels)
    same, sloss = _grad(gpu, name, models, x, labels, src=_cuda(np.arange(D, dtype=np.int32)))
    assert (_bits(same) == _bits(plain)).all() and (_bits(sloss) == _bits(ploss)).all()
    assert not (_bits(out[:, :P]) == _bits(plain[:, :P])).all(axis=1).any()
    # LenetTraining takes a host array, checks it and copies it
    tr = _training(gpu, name, per_device=True)
    W = _stack(models)
    assert (_bits(tr.gradients(W, src=src)) == _bits(out[:, :P])).all()
    with pytest.raises(ValueError, match="src"):
        tr.gradients(W, src=[1, 2, 3])


def test_first_selects_each_devices_batch_and_wraps(gpu):
    name = "generic_k"
    geom, batch, Nt, _ = gc.CASES[name]
    _, _, models = gc.data(name)
    P = models.shape[1]
    first = [2, 0, Nt - 1]  # the last one wraps after one sample
    out, loss = _grad(gpu, name, models, first=_cuda(np.array(first, dtype=np.int64)))
    g, l = out.cpu().numpy(), loss.cpu().numpy()
    for d in range(D):
        _assert_parity(name, g[d, :P], l[d], d, first=first[d], what="first")
    zero, _ = _grad(gpu, name, models)
    assert (_bits(out[1]) == _bits(zero[1])).all() and not (_bits(out[0]) == _bits(zero[0])).all()
    # first + Nt is the same batch
    far, _ = _grad(gpu, name, models, first=_cuda(np.array(first, dtype=np.int64) + Nt))
    assert (_bits(far) == _bits(out)).all()


def test_skip_leaves_row_and_loss_untouched(gpu):
    name = "pool2_drops"
    _, _, models = gc.data(name)
    plain, ploss = _grad(gpu, name, models)
    out, loss = _grad(gpu, name, models, skip=_cuda(np.array([0, 1, 0], dtype=np.int32)))
    assert (out[1].cpu().numpy() == SENTINEL).all() and float(loss[1]) == SENTINEL
    for d in (0, 2):
        assert (_bits(out[d]) == _bits(plain[d])).all() and _bits(loss)[d] == _bits(ploss)[d]


@pytest.mark.parametrize("name", ["lenet1", "map_1x1"])
def test_shared_and_replicated_sets_agree(gpu, name):
    x, labels, models = gc.data(name)
    shared, sloss = _grad(gpu, name, models)
    own, oloss = _grad(gpu, name, models, np.stack([x] * D), np.stack([labels] * D))
    assert (_bits(own) == _bits(shared)).all() and (_bits(oloss) == _bits(sloss)).all()


def _optimizer(gpu, name, rule):
    from federated_amd.local_optim import PopulationOptimizer
    from federated_amd.tf2_validation import lenet_layer_shapes
    shapes = lenet_layer_shapes(gc.CASES[name][0])
    if rule == "adam":
        return PopulationOptimizer(gpu, D, shapes, "adam", 1e-3, clipnorm=1.0)
    return PopulationOptimizer(gpu, D, shapes, "sgd", 0.05)


@pytest.mark.parametrize("rule", ["sgd", "adam"])
def test_epoch_is_its_sequence_of_public_calls(gpu, rule):
    name = "generic_k"
    geom, batch, Nt, _ = gc.CASES[name]
    _, _, models = gc.data(name)
    skip = _cuda(np.array([0, 0, 1], dtype=np.int32))
    results = []
    for manual in (False, True):
        tr, opt, W = _training(gpu, name).allocate(D), _optimizer(gpu, name, rule), _stack(models)
        if manual:
            for _ in range(3):
                g = tr.gradients(W, skip=skip)
                opt.step(W, g, skip)
                tr.advance(skip)
        else:
            assert tr.epoch(W, opt, 3, skip) is W
        assert tr.cursor.cpu().numpy().tolist() == [3 * batch % Nt, 3 * batch % Nt, 0]
        assert opt.steps_done.tolist() == [3, 3, 0]
        results.append((_bits(W), _bits(tr.grads), _bits(tr.loss)))
    for a, b in zip(*results):
        assert (a == b).all()
    assert (results[0][0][2] == models.view(np.uint32)[2]).all()      # the skipped device's model
    assert not (results[0][0][0] == models.view(np.uint32)[0]).all()  # the others moved
    # the second batch is the set's next samples: the last call's gradient is that of first = 2 * batch
    assert 3 * batch > Nt  # and the third wrapped


def test_captured_epoch_replays_the_eager_one(gpu):
    """validate -> epoch of 2 batches -> pop.rounds(1), captured once after allocate and replayed
    twice: the bits of the same two eager epochs. Device 1 has ended from the start."""
    from federated_amd import topology as T
    from federated_amd._graphs import RoundGraphs
    from federated_amd.tf2_validation import LenetValidation
    name = "lenet1"
    geom, batch, Nt, _ = gc.CASES[name]
    x, labels, models = gc.data(name)
    lists = [[(d - 1) % D, (d + 1) % D] for d in range(D)]

    def run(graph):
        pop = T.PopulationRound(gpu, _stack(models), _stack(np.zeros_like(models)))
        pop.set_topology(lists, T.alphas_tf2)
        pop.set_ended_rule("copy", propagate=False)
        pop.set_ended([1])
        val = LenetValidation(gpu, geom, _cuda(x), _cuda(labels), batch, 2, target=1e-3).allocate(D)
        tr, opt = _training(gpu, name).allocate(D), _optimizer(gpu, name, "adam")

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
        return (_bits(pop.models), _bits(tr.grads), _bits(tr.loss), tr.cursor.cpu().numpy().tolist(),
                opt.steps_done.tolist(), pop.ended.cpu().numpy().tolist())

    eager, replay = run(False), run(True)  # eager first: it also loads every torch kernel the capture uses
    assert eager[3] == replay[3] == [4 * batch % Nt, 0, 4 * batch % Nt]
    assert eager[4] == replay[4] == [4, 0, 4] and eager[5] == replay[5] == [0, 1, 0]
    for a, b in zip(eager[:3], replay[:3]):
        assert (a == b).all()
    assert not (eager[0][0] == models.view(np.uint32)[0]).all()


def test_refusals(gpu):
    from federated_amd import _lib
    name = "pool2_drops"
    geom, batch, Nt, _ = gc.CASES[name]
    x, labels, models = gc.data(name)
    xs, ls, W = _cuda(x), _cuda(labels), _stack(models)
    P = lc.size(geom)
    grads = torch.full((D, P), SENTINEL, dtype=torch.float32, device="cuda")
    loss = torch.full((D,), SENTINEL, dtype=torch.float32, device="cuda")
    ws = gpu.lenet_grad_workspace(D, batch, geom)
    good = dict(x=xs.data_ptr(), xstride=0, labels=ls.data_ptr(), lstride=0, Nt=Nt, geom=geom, models=W.data_ptr(),
                pitch=int(W.stride(0)), D=D, src=None, first=None, batch=batch, skip=None, grads=grads.data_ptr(),
                gpitch=P, loss=loss.data_ptr(), ws=ws.data_ptr(), ws_bytes=ws.numel() * 4)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        _lib.call("cfa_lenet_grad_f32", a["x"], a["xstride"], a["labels"], a["lstride"], a["Nt"], *a["geom"],
                  a["models"], a["pitch"], a["D"], a["src"], a["first"], a["batch"], a["skip"], a["grads"],
                  a["gpitch"], a["loss"], a["ws"], a["ws_bytes"], None)

    invalid = [
        (dict(x=None), "null buffer"), (dict(labels=None), "null buffer"), (dict(models=None), "null buffer"),
        (dict(grads=None), "null buffer"), (dict(ws=None), "null buffer"),
        (dict(D=0), "must be >= 1"), (dict(batch=0), "must be >= 1"), (dict(Nt=0), "must be >= 1"),
        (dict(geom=(12, 3, 0, 3, 4)), "bad geometry"), (dict(geom=(12, 0, 2, 3, 4)), "bad geometry"),
        (dict(geom=(6, 3, 2, 3, 4)), "bad geometry"),  # p1 = 2 < kernel: p2 < 1
        (dict(batch=Nt + 1), "does not fit"),
        (dict(pitch=P - 1), "pitch"), (dict(gpitch=P - 1), "gpitch"),
        (dict(xstride=Nt * 12 * 12 - 1), "device strides"), (dict(lstride=Nt - 1), "device strides"),
        (dict(ws_bytes=ws.numel() * 4 - 1), "workspace"),
    ]
    for kw, text in invalid:
        with pytest.raises(_lib.CFAError, match=text) as e:
            call(**kw)
        assert e.value.code == _lib.CFA_E_INVALID, kw
    # beyond the one-workgroup LDS plan, and beyond 64 classes: refused, not launched
    big = lc.UNSUPPORTED
    Pb = lc.size(big)
    xb = torch.zeros(4, 28, 28, device="cuda")
    lb = torch.zeros(4, dtype=torch.int32, device="cuda")
    Wb = torch.zeros(D, Pb, device="cuda")
    for kw in (dict(geom=big, x=xb.data_ptr(), labels=lb.data_ptr(), Nt=4, models=Wb.data_ptr(), pitch=Pb, gpitch=Pb,
                    batch=2),
               dict(geom=geom[:4] + (65,), pitch=1 << 20, gpitch=1 << 20)):
        with pytest.raises(_lib.CFAError) as e:
            call(**kw)
        assert e.value.code == _lib.CFA_E_UNSUPPORTED, kw
    torch.cuda.synchronize()
    assert (grads.cpu().numpy() == SENTINEL).all() and (loss.cpu().numpy() == SENTINEL).all()
    # the Engine's own checks
    with pytest.raises(ValueError):
        gpu.lenet_grad(geom, xs, ls, W[:, :-1], batch, grads, ws)
    with pytest.raises(TypeError):
        gpu.lenet_grad(geom, xs, ls.long(), W, batch, grads, ws)
    with pytest.raises(ValueError):
        gpu.lenet_grad(geom, xs, ls, W, Nt + 1, grads, ws)
    with pytest.raises(ValueError):
        gpu.lenet_grad(geom, xs, ls, W, batch, grads[:, :-1], ws)
    with pytest.raises(TypeError):
        gpu.lenet_grad(geom, xs, ls, W, batch, grads, ws, loss.double())
    with pytest.raises(TypeError):
        gpu.lenet_grad(geom, xs, ls, W, batch, grads, ws, first=torch.zeros(D, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        gpu.lenet_grad(geom, xs, ls, W, batch, grads, ws, skip=torch.zeros(D + 1, dtype=torch.int32, device="cuda"))
    # and the good call still runs, loss or none
    call(loss=None)
    torch.cuda.synchronize()
    assert (grads.cpu().numpy() != SENTINEL).all() and (loss.cpu().numpy() == SENTINEL).all()


@pytest.mark.parametrize("name", ["lenet1", "pool2_drops"])
def test_a_label_out_of_range_gives_that_device_nan(gpu, name):
    geom, batch, Nt, _ = gc.CASES[name]
    x, labels, models = gc.data(name)
    P = models.shape[1]
    own = np.stack([labels] * D)
    own[1, batch - 1] = geom[4]  # device 1's last sample of the batch
    plain, ploss = _grad(gpu, name, models)
    out, loss = _grad(gpu, name, models, np.stack([x] * D), own)
    assert np.isnan(out[1, :P].cpu().numpy()).all() and np.isnan(float(loss[1]))
    for d in (0, 2):
        assert (_bits(out[d]) == _bits(plain[d])).all() and _bits(loss)[d] == _bits(ploss)[d]
    from federated_amd.tf2_training import LenetTraining
    with pytest.raises(ValueError, match="labels"):
        LenetTraining(gpu, geom, _cuda(np.stack([x] * D)), _cuda(own), batch)
