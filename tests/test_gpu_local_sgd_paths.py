"""The local-SGD epoch kernels (csrc/cfa_local_sgd.hip) on the paths the four shapes of
test_gpu_local_training.py never take: the tail loops of Prefetch::store, the <16, 5> kernel
without register taps and on an input shorter than its filter, the generic CNN kernel at
F > kMaxTaps, S = 1 and L2 = 1, softmax widths 1, 16 and 64 (full and with dead lanes), the second
trips of the softmax and logits loops, a 2NN first layer of two slices with a last slice of one
input, both halves of the clip's gate, pooling ties, a dead relu, a CNN launch above 64 KiB of
LDS, more workgroups than compute units, an empty population and the refusals.

Cases, data, reference, tolerance and guards live in local_sgd_cases.py (its docstring has the
rules): every launch goes through Engine.local_sgd on a pitched stack with padding and is compared
per (device, tensor) with the float64 epoch at ``max(1e-5, 4 * s)``, the cost at 1e-5 relative;
every case asserts, before it launches, the condition that puts it on its path from the mirror of
the launch plan, and every randomised case the margin guard over its whole trajectory.
test_local_sgd_cases_host.py asserts the same on the CPU."""
import numpy as np
import pytest
import torch

import local_sgd_cases as lc
from test_gpu_local_training import LR, NAMES, _cuda, _kernel_geom, _run

pytestmark = pytest.mark.gpu


def _launch(gpu, c, update=True):
    x, y, W = c.data
    return _run(gpu, c.ml, c.geom, x, y, W, c.stride, c.rows, c.steps, update=update)


def _assert_epoch(c, got, cost, devices=None):
    """Every tensor of every device within its allowance of the float64 epoch (printed per tensor,
    as _assert_models of test_gpu_local_training.py does, and the case's largest), the cost within
    1e-5 relative."""
    ref = lc.reference(c)
    worst, bad = 0.0, []
    for d in range(c.D):
        for k in range(4):
            a, r = got[d, c.offs[k]:c.offs[k + 1]].astype(np.float64), ref["w64"][d, c.offs[k]:c.offs[k + 1]]
            err = np.max(np.abs(a - r)) / np.max(np.abs(r))
            if c.D <= 4:
                print(f"{c.name} device {d} {NAMES[k]}: normwise error {err:.3e}, allowed {ref['allow'][d][k]:.3e}")
            worst = max(worst, err)
            if not err <= ref["allow"][d][k]:
                bad.append((d, NAMES[k], err, ref["allow"][d][k]))
    allowed = min(min(a) for a in ref["allow"])
    print(f"case {c.name}: largest normwise error {worst:.3e}, allowed {allowed:.3e}, s {ref['s']:.2e}")
    assert not bad, bad
    print(f"case {c.name}: cost", cost, ref["c64"])
    assert np.all(np.abs(cost - ref["c64"]) <= 1e-5 * np.abs(ref["c64"]))


def _check(gpu, c):
    """The launch with update=True against the float64 epoch; returns its models."""
    got, padding, cost = _launch(gpu, c)
    assert np.all(padding == 7.5)
    _assert_epoch(c, got, cost)
    return got


# ------------------------------------------------------------------------------------------
# The table: A to H
# ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(lc.TABLE))
def test_path_matches_the_float64_epoch(gpu, name):
    c = lc.TABLE[name]
    lc.assert_path(c)
    lc.assert_guarded(c)
    got = _check(gpu, c)
    assert not np.array_equal(got, c.data[2])


@pytest.mark.parametrize("name", list(lc.TABLE))
def test_path_in_validation_mode(gpu, name):
    """update=False: the models keep their bits, the cost is the forward pass's."""
    c = lc.TABLE[name]
    lc.assert_path(c)
    ref = lc.reference(c, update=False)
    got, padding, cost = _launch(gpu, c, update=False)
    assert np.array_equal(got.view(np.uint32), c.data[2].view(np.uint32)) and np.all(padding == 7.5)
    print(f"case {name}: validation cost", cost, ref["c64"])
    assert np.all(np.abs(cost - ref["c64"]) <= 1e-5 * np.abs(ref["c64"]))


@pytest.mark.parametrize("name", list(lc.TABLE))
def test_path_gives_the_same_bits_twice(gpu, name):
    c = lc.TABLE[name]
    a, b = _launch(gpu, c), _launch(gpu, c)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[2], b[2])


# ------------------------------------------------------------------------------------------
# Built cases: the clip's gate, one class, pooling ties, a dead relu
# ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ml", [1, 2])
def test_clip_blocks_the_gradient_above_its_bound(gpu, ml):
    """Two steps; in each minibatch four labelled predictions in (0.99, 0.999), where the gate
    blocks the gradient, and four below 0.99, none within 1e-3 of the bound (asserted from the
    float64 forward pass at both steps). A gate without ``p <= kClipHi`` would move the float64
    result, normwise per tensor W1 b1 W2 b2, by 5.4e-5 7.8e-5 3.6e-3 4.6e-5 (CNN) and
    2.0e-5 3.1e-5 4.2e-3 4.0e-5 (2NN): W2 by some 400 times the allowance of 1e-5."""
    c = lc.CLIP_ABOVE[ml]
    effect = lc.assert_clip_above(c)
    print(f"case {c.name}: an open gate would move W1 b1 W2 b2 by", " ".join(f"{v:.2e}" for v in effect))
    _check(gpu, c)


@pytest.mark.parametrize("ml", [1, 2])
def test_clip_blocks_the_gradient_below_its_bound(gpu, ml):
    """One step; two of the six samples have their labelled logit 45 or more below the largest
    (pred < 1e-16): no gradient, and a cost of -log(1e-15) each."""
    c = lc.CLIP_BELOW[ml]
    lc.assert_clip_below(c)
    _check(gpu, c)


@pytest.mark.parametrize("ml", [1, 2])
def test_one_class_blocks_every_gradient(gpu, ml):
    """C = 1 (SW = 1, no shuffle): pred = 1, so update=True leaves every bit of the models and
    the cost is -log(0.99)."""
    c = lc.ONE_CLASS[ml]
    lc.assert_one_class(c)
    got, padding, cost = _launch(gpu, c)
    assert np.array_equal(got.view(np.uint32), c.data[2].view(np.uint32)) and np.all(padding == 7.5)
    print(f"case {c.name}: cost", cost, "relative distance to -log(0.99)", np.abs(cost + np.log(0.99)) / -np.log(0.99))
    assert np.all(np.abs(cost + np.log(0.99)) <= 1e-6 * -np.log(0.99))


@pytest.mark.parametrize("fast", [False, True], ids=["generic", "fast"])
def test_pooling_tie_goes_to_the_first_maximum(gpu, fast):
    """Small-integer samples and unit taps: two positions of a window tie at a positive value and
    the first takes the gradient (``h > best``), as in the oracle; one step."""
    c, ties, zero = lc.TIES[fast]
    assert c.plan.fast == fast and (c.plan.taps_in_regs or not fast)
    lc.assert_tie(c, ties, zero)
    _check(gpu, c)


@pytest.mark.parametrize("fast", [False, True], ids=["generic", "fast"])
def test_dead_relu_moves_only_the_last_bias(gpu, fast):
    """Device 0's pooled values are all 0: W1, b1 and W2 (gradient exactly 0) keep their bits, b2
    moves as the reference says. Device 1 is an ordinary one in the same launch."""
    c = lc.DEAD[fast]
    assert c.plan.fast == fast
    lc.assert_dead(c)
    got = _check(gpu, c)
    W = c.data[2]
    assert np.array_equal(got[0, :c.offs[3]].view(np.uint32), W[0, :c.offs[3]].view(np.uint32))
    assert np.all(got[0, c.offs[3]:] != W[0, c.offs[3]:])


# ------------------------------------------------------------------------------------------
# Grid and refusals
# ------------------------------------------------------------------------------------------

def test_more_workgroups_than_compute_units(gpu):
    """300 devices, each with its own samples and model, one minibatch: every row at 1e-5."""
    c = lc.MANY
    assert c.D == 300 > torch.cuda.get_device_properties(0).multi_processor_count
    lc.assert_guarded(c)
    assert all(a == 1e-5 for dev in lc.reference(c)["allow"] for a in dev)
    _check(gpu, c)


def test_empty_population_is_a_no_op(gpu):
    """D = 0: no launch, nothing written (the counter of a cost log would move with a launch)."""
    geom = lc.NN_TINY
    P, L, C = lc.plan(2, geom).P, geom["input_data"], geom["classes"]
    stack = torch.full((3, P + 3), 7.5, device="cuda")
    x, y = torch.empty(0, 4, L, device="cuda"), torch.empty(0, 4, C, device="cuda")
    cost = torch.empty(0, dtype=torch.float64, device="cuda")
    for ml, g in ((2, _kernel_geom(geom)), (1, {"filter": 4, "number": 1, "stride": 4})):
        models = stack[:0, :P] if ml == 2 else torch.empty(0, 4 + 1 + 2 * C + C, device="cuda")
        out = gpu.local_sgd(ml, x, y, models, g, 4, 4, 1, LR, True, cost)
        assert out is models
    torch.cuda.synchronize()
    assert bool((stack == 7.5).all())


@pytest.mark.parametrize("ml", [1, 2])
def test_more_than_64_classes_is_refused(gpu, ml):
    from federated_amd._lib import CFAError
    geom = lc._cnn(4, 4, 6, 37, 65) if ml == 1 else lc._nn(20, 5, 65)
    P = lc.plan(ml, geom).P
    x = torch.zeros(2, 4, geom["input_data"], device="cuda")
    y = torch.zeros(2, 4, 65, device="cuda")
    W = torch.full((2, P), -7.0, device="cuda")
    cost = torch.full((2,), -7.0, dtype=torch.float64, device="cuda")
    for update in (True, False):
        with pytest.raises(CFAError, match="more than 64 classes"):
            gpu.local_sgd(ml, x, y, W, _kernel_geom(geom), 4, 4, 1, LR, update, cost)
    torch.cuda.synchronize()
    assert bool((W == -7.0).all()) and bool((cost == -7.0).all())


@pytest.mark.parametrize("ml,geom,rows", lc.TOO_MUCH_LDS, ids=["cnn", "2nn"])
def test_minibatch_beyond_the_lds_is_refused(gpu, ml, geom, rows):
    from federated_amd._lib import CFAError
    assert lc.lds_bytes(ml, geom, rows) > lc.LDS_DEVICE  # more than a workgroup can have
    P = lc.plan(ml, geom).P
    x = torch.zeros(2, rows, geom["input_data"], device="cuda")
    y = torch.zeros(2, rows, geom["classes"], device="cuda")
    W = torch.full((2, P), -7.0, device="cuda")
    with pytest.raises(CFAError, match="bytes of LDS"):
        gpu.local_sgd(ml, x, y, W, _kernel_geom(geom), rows, rows, 1, LR)
    torch.cuda.synchronize()
    assert bool((W == -7.0).all())


@pytest.mark.parametrize("name", ["F", "H"])
def test_cost_log_is_written_without_a_cost_buffer(gpu, name):
    """cost=None with a log: row 0 of the log takes the launch's cost, the counter moves to 1."""
    c = lc.TABLE[name]
    x, y, W = c.data
    _, _, cost = _launch(gpu, c)
    log = torch.full((2, c.D), float("nan"), dtype=torch.float64, device="cuda")
    epoch = torch.zeros(1, dtype=torch.int64, device="cuda")
    gpu.local_sgd(c.ml, _cuda(x), _cuda(y), _cuda(W), _kernel_geom(c.geom), c.stride, c.rows, c.steps, LR, True, None,
                  log, epoch)
    torch.cuda.synchronize()
    assert int(epoch.item()) == 1
    assert np.array_equal(log[0].cpu().numpy(), cost) and bool(torch.isnan(log[1]).all())
