"""The validation pass of a TF2 LeNet-1 population on the device (cfa_lenet_eval_f32,
Engine.lenet_eval, tf2_validation.LenetValidation) against the fp64 restatement of
tests/lenet_cases.py (its docstring has the family, the data and the tolerance's margin;
test_lenet_validation_host.py pins the restatement by a second implementation).

Geometries: LeNet-1 at the driver's batch of 100 (the kernel's compile-time kernel side), and the
smallest ones that reach each other path (a pool that drops a row and column, in either stage; a
1 x 1 map; rows that are not 16-byte aligned), with batch 3, batches 2 and Nt = 7, one tail
sample unused, D in {1, 5} and pitch > P."""
import numpy as np
import pytest
import torch

import lenet_cases as lc
from conftest import normwise_close

pytestmark = pytest.mark.gpu

SMALL = ("pool2_drops", "pool1_drops", "map_1x1")
SENTINEL = -7.25


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()  # a copy: the shared reference data is read only


def _stack(models, pad=0):
    """The models as a [D, P] CUDA view of a stack with `pad` extra floats per row (NaN)."""
    D, P = models.shape
    full = torch.full((D, P + pad), float("nan"), dtype=torch.float32, device="cuda")
    full[:, :P] = _cuda(models)
    return full[:, :P]


def _validation(gpu, name, x, labels, **kw):
    from federated_amd.tf2_validation import LenetValidation
    geom, batch, batches, _ = lc.CASES[name]
    return LenetValidation(gpu, geom, _cuda(x), _cuda(labels), batch, batches, **kw)


def _bits(t):
    return t.cpu().numpy().view(np.uint64)


def _gap_target(ref):
    """The midpoint of the widest gap between neighbouring sorted costs; the gap must exceed 1e-3
    relative, so that rounding cannot flip a comparison."""
    s = np.sort(ref)
    i = int(np.argmax(np.diff(s)))
    assert s[i + 1] - s[i] > 1e-3 * s[i + 1]
    return 0.5 * (s[i] + s[i + 1])


PARITY = [("lenet1", 3, 0)] + [(n, D, pad) for n in SMALL for D, pad in ((1, 0), (5, 0), (5, 3))]


@pytest.mark.parametrize("name,D,pad", PARITY)
def test_cost_parity(gpu, name, D, pad):
    x, labels, models, ref = lc.reference(name, D)
    val = _validation(gpu, name, x, labels)
    assert val.P == lc.size(lc.CASES[name][0])
    cost = val.validate(_stack(models, pad)).cpu().numpy()
    print(name, D, pad, "cost", cost, "max rel err", np.max(np.abs(cost - ref)) / np.max(np.abs(ref)))
    assert normwise_close(cost, ref, 1e-5)


@pytest.mark.parametrize("name,D", [("lenet1", 3), ("pool2_drops", 5)])
def test_flag_rule(gpu, name, D):
    x, labels, models, ref = lc.reference(name, D)
    target = _gap_target(ref)
    val = _validation(gpu, name, x, labels, target=target)
    W = _stack(models)
    ended = torch.zeros(D, dtype=torch.int32, device="cuda")
    val.validate(W, ended=ended)
    want = lc.flags(ref, target)
    assert 0 < want.sum() < D and ended.cpu().numpy().tolist() == want.tolist()
    # a flag set beforehand stays set, though that device's cost is above the target
    above = int(np.argmax(ref))
    before = np.zeros(D, dtype=np.int32)
    before[above] = 1
    ended = _cuda(before)
    val.validate(W, ended=ended)
    assert ref[above] > target and ended.cpu().numpy().tolist() == lc.flags(ref, target, before).tolist()
    with pytest.raises(ValueError, match="target"):
        _validation(gpu, name, x, labels).validate(W, ended=ended)


@pytest.mark.parametrize("same_tensor", [False, True])
def test_skip(gpu, same_tensor):
    name, D = "pool1_drops", 5
    x, labels, models, ref = lc.reference(name, D)
    target = _gap_target(ref)
    W = _stack(models, 1)
    val = _validation(gpu, name, x, labels, target=target, log_cap=1)
    plain = val.validate(W).clone()
    skipped = [1, 3]  # these devices have left their loops
    flags = np.zeros(D, dtype=np.int32)
    flags[skipped] = 1
    skip = _cuda(flags)
    ended = skip if same_tensor else torch.zeros(D, dtype=torch.int32, device="cuda")
    val.val_cost.fill_(SENTINEL)
    val.validate(W, skip=skip, ended=ended)
    cost = val.val_cost.cpu().numpy()
    others = [d for d in range(D) if d not in skipped]
    assert (cost[skipped] == SENTINEL).all()
    assert (_bits(val.val_cost)[others] == _bits(plain)[others]).all()
    want = lc.flags(ref, target, before=flags if same_tensor else None, skip=flags)
    assert ended.cpu().numpy().tolist() == want.tolist()
    assert skip.cpu().numpy().tolist() == (want if same_tensor else flags).tolist()
    # a skipped device's log entry is its untouched cost
    assert (_bits(val.val_log[0]) == _bits(val.val_cost)).all()


def test_log(gpu):
    name, D = "map_1x1", 5
    x, labels, models, ref = lc.reference(name, D)
    val = _validation(gpu, name, x, labels, log_cap=2)
    calls = []
    for c in range(3):  # another population each call
        m = lc.make(lc.CASES[name][0], D, 7, seed=10 + c)[2]
        calls.append(val.validate(_stack(m)).clone())
    assert val.epochs_done == 3
    assert (_bits(val.val_log[0]) == _bits(calls[0])).all() and (_bits(val.val_log[1]) == _bits(calls[2])).all()
    assert not (_bits(calls[0]) == _bits(calls[2])).any()


@pytest.mark.parametrize("name,D", [("lenet1", 3), ("pool2_drops", 5)])
def test_determinism_and_ownership(gpu, name, D):
    x, labels, models, ref = lc.reference(name, D)
    val = _validation(gpu, name, x, labels)
    first = val.validate(_stack(models)).clone()
    assert (_bits(val.validate(_stack(models))) == _bits(first)).all()
    # a model row moved to another device index: the same bits for that model
    perm = np.roll(np.arange(D), 1)
    moved = val.validate(_stack(models[perm])).clone()
    assert (_bits(moved) == _bits(first)[perm]).all()
    # a padded stack
    assert (_bits(val.validate(_stack(models, 5))) == _bits(first)).all()
    # every device its own set (non-zero strides), D copies of the shared one
    own = _validation(gpu, name, np.stack([x] * D), np.stack([labels] * D))
    assert own.per_device == D
    assert (_bits(own.validate(_stack(models))) == _bits(first)).all()


def test_graph_replay(gpu):
    from federated_amd._graphs import RoundGraphs
    name, D = "pool2_drops", 5
    x, labels, models, ref = lc.reference(name, D)
    target = _gap_target(ref)  # some devices end at the first call and are skipped by the next two
    W = _stack(models)

    def run(graph):
        val = _validation(gpu, name, x, labels, target=target, log_cap=2).allocate(D)
        flags = torch.zeros(D, dtype=torch.int32, device="cuda")
        step = lambda: val.validate(W, skip=flags, ended=flags)  # noqa: E731
        if graph:
            RoundGraphs(W.device, step, 1, lambda: 0).run(3)
        else:
            for _ in range(3):
                step()
        torch.cuda.synchronize()
        return _bits(val.val_cost), _bits(val.val_log), val.epochs_done, flags.cpu().numpy().tolist()

    eager, replay = run(False), run(True)
    assert eager[2] == replay[2] == 3 and eager[3] == replay[3] == lc.flags(ref, target).tolist()
    assert 0 < sum(eager[3]) < D
    assert (eager[0] == replay[0]).all() and (eager[1] == replay[1]).all()


def test_chain_with_population_round(gpu):
    """validate(pop.models, pop.ended, pop.ended) then a round: the models of set_ended(ids from the
    restatement) then a round."""
    from federated_amd import topology as T
    name, D = "pool2_drops", 5
    x, labels, models, ref = lc.reference(name, D)
    target = _gap_target(ref)
    ids = [d for d in range(D) if ref[d] < target]
    assert 0 < len(ids) < D
    lists = [[(d - 1) % D, (d + 1) % D] for d in range(D)]
    out = []
    for on_device in (True, False):
        # rows pitched to 16 bytes, as the population kernels expect (P = 93)
        pop = T.PopulationRound(gpu, _stack(models, 3), _stack(np.zeros_like(models), 3))
        pop.set_topology(lists, T.alphas_tf2)
        pop.set_ended_rule("copy", propagate=False)
        if on_device:
            val = _validation(gpu, name, x, labels, target=target)
            val.validate(pop.models, skip=pop.ended, ended=pop.ended)
            assert pop.ended.cpu().numpy().tolist() == lc.flags(ref, target).tolist()
        else:
            pop.set_ended(ids)
        out.append(pop.rounds(1).cpu().contiguous().numpy().view(np.uint32))
    assert (out[0] == out[1]).all()
    assert not (out[0] == models.view(np.uint32)).all()  # the round did something


def test_refusals(gpu):
    from federated_amd import _lib
    name, D = "pool2_drops", 2
    geom, batch, batches, Nt = lc.CASES[name]
    x, labels, models, _ = lc.reference(name, D)
    xs, ls, W = _cuda(x), _cuda(labels), _stack(models)
    P = lc.size(geom)
    cost = torch.full((D,), SENTINEL, dtype=torch.float64, device="cuda")
    ws = gpu.lenet_workspace(D, batches)
    log = torch.zeros(1, D, dtype=torch.float64, device="cuda")
    epoch = torch.zeros(1, dtype=torch.int64, device="cuda")
    flags = torch.zeros(D, dtype=torch.int32, device="cuda")
    good = dict(x=xs.data_ptr(), xstride=0, labels=ls.data_ptr(), lstride=0, Nt=Nt, geom=geom, models=W.data_ptr(),
                pitch=P, D=D, batch=batch, batches=batches, skip=None, target=0.5, ended=None, cost=cost.data_ptr(),
                log=None, cap=0, epoch=None, ws=ws.data_ptr(), ws_bytes=ws.numel() * 4)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        _lib.call("cfa_lenet_eval_f32", a["x"], a["xstride"], a["labels"], a["lstride"], a["Nt"], *a["geom"],
                  a["models"], a["pitch"], a["D"], a["batch"], a["batches"], a["skip"], a["target"], a["ended"],
                  a["cost"], a["log"], a["cap"], a["epoch"], a["ws"], a["ws_bytes"], None)

    invalid = [
        (dict(x=None), "null buffer"), (dict(labels=None), "null buffer"), (dict(models=None), "null buffer"),
        (dict(cost=None), "null buffer"), (dict(ws=None), "null buffer"),
        (dict(D=0), "must be >= 1"), (dict(batch=0), "must be >= 1"), (dict(batches=0), "must be >= 1"),
        (dict(geom=(12, 3, 0, 3, 4)), "bad geometry"), (dict(geom=(12, 3, 2, 0, 4)), "bad geometry"),
        (dict(geom=(12, 3, 2, 3, 0)), "bad geometry"), (dict(geom=(12, 0, 2, 3, 4)), "bad geometry"),
        (dict(geom=(6, 3, 2, 3, 4)), "bad geometry"),  # p1 = 2 < kernel: p2 < 1
        (dict(batches=3), "do not fit"),               # batch * batches = 9 > Nt = 7
        (dict(pitch=P - 1), "pitch"),
        (dict(xstride=Nt * 12 * 12 - 1), "device strides"), (dict(lstride=Nt - 1), "device strides"),
        (dict(log=log.data_ptr(), cap=1), "given together"), (dict(epoch=epoch.data_ptr()), "given together"),
        (dict(log=log.data_ptr(), cap=0, epoch=epoch.data_ptr()), "log_cap"),
        (dict(ws_bytes=ws.numel() * 4 - 1), "workspace"),
        (dict(ended=flags.data_ptr(), target=float("nan")), "finite"),
        (dict(ended=flags.data_ptr(), target=float("inf")), "finite"),
    ]
    for kw, text in invalid:
        with pytest.raises(_lib.CFAError, match=text) as e:
            call(**kw)
        assert e.value.code == _lib.CFA_E_INVALID, kw
    # beyond the one-workgroup LDS plan: refused, not approximated
    big = lc.UNSUPPORTED
    Pb = lc.size(big)
    xb = torch.zeros(4, 28, 28, device="cuda")
    lb = torch.zeros(4, dtype=torch.int32, device="cuda")
    Wb = torch.zeros(D, Pb, device="cuda")
    for kw in (dict(geom=big, x=xb.data_ptr(), labels=lb.data_ptr(), Nt=4, models=Wb.data_ptr(), pitch=Pb, batch=2),
               dict(geom=geom[:4] + (65,), pitch=1 << 20)):
        with pytest.raises(_lib.CFAError) as e:
            call(**kw)
        assert e.value.code == _lib.CFA_E_UNSUPPORTED, kw
    # nothing was launched: the cost, the counter and the flags are as they were
    torch.cuda.synchronize()
    assert (cost.cpu().numpy() == SENTINEL).all() and int(epoch.item()) == 0 and int(flags.sum().item()) == 0
    # the Engine's own checks
    with pytest.raises(ValueError):
        gpu.lenet_eval(geom, xs, ls, W[:, :-1], batch, batches, cost, ws)
    with pytest.raises(TypeError):
        gpu.lenet_eval(geom, xs, ls.long(), W, batch, batches, cost, ws)
    with pytest.raises(TypeError):
        gpu.lenet_eval(geom, xs.double(), ls, W, batch, batches, cost, ws)
    with pytest.raises((TypeError, ValueError)):
        gpu.lenet_eval(geom, xs, ls, W.cpu(), batch, batches, cost, ws)
    with pytest.raises(TypeError):
        gpu.lenet_eval(geom, xs, ls, W, batch, batches, cost.float(), ws)
    with pytest.raises(ValueError):
        gpu.lenet_eval(geom, xs, ls, W, batch, batches, cost[:1], ws)
    with pytest.raises(ValueError):
        gpu.lenet_eval(geom, xs, ls, W, batch, 3, cost, ws)
    # labels out of range are refused at construction
    from federated_amd.tf2_validation import LenetValidation
    bad = labels.copy()
    bad[2] = geom[4]
    with pytest.raises(ValueError, match="labels"):
        LenetValidation(gpu, geom, xs, _cuda(bad), batch, batches)
    # and the good call still runs
    call()
    torch.cuda.synchronize()
    assert (cost.cpu().numpy() != SENTINEL).all()
