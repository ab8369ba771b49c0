#!/usr/bin/env python3
"""The local batches of a TF2 LeNet-1 population at the MNIST driver's defaults (30 devices, LeNet-1,
batches of 100 out of a per-device training set) timed in three forms on the same images and models:

* ``gradients``: LenetTraining.gradients, one batch's loss and gradient for the whole population in
  one cfa_lenet_grad_f32 call (two launches);
* ``epoch``: LenetTraining.epoch of ``--batches`` batches with Adam (gradients, the
  PopulationOptimizer step and the cursor advance, per batch), reported per batch;
* ``torch``: what a user of the device-resident populations has without it: D sequential
  torch-ROCm forward passes (conv2d, avg_pool2d, matmul, log_softmax) with autograd.grad on the same
  batch, the six gradients of each device copied into its row of a [D, P] stack.

``--loss huber`` times all three on the Huber drivers' objective instead of the cross-entropy one.

Every form runs windows of back-to-back calls between two device events, ending in a
synchronise; the forms alternate window by window after ``--warmup`` untimed windows each.
Reported: the median window over ``--reps`` per call in milliseconds with its extremes, torch's
median over the device's, and how far the two forms' gradients are apart normwise (the largest
over the six tensors and the devices). Prints one JSON line and appends it to ``--out``.
Usage: python tools/lenet_training.py [--loss xent|huber] [--out profiles/lenet_training.jsonl]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

D, NT, BATCH = 30, 800, 100


def macs_per_image(geom):
    """Multiply-adds of one sample's forward and backward pass (no input gradient in stage 1)."""
    side, k, c1, c2, classes = geom
    s1 = side - k + 1
    p1 = s1 // 2
    s2 = p1 - k + 1
    p2 = s2 // 2
    conv1, conv2, dense = s1 * s1 * c1 * k * k, s2 * s2 * c2 * k * k * c1, p2 * p2 * c2 * classes
    return 2 * conv1 + 3 * conv2 + 3 * dense


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20, help="gradients calls per timed window")
    ap.add_argument("--batches", type=int, default=4, help="batches of the timed epoch")
    ap.add_argument("--epochs", type=int, default=5, help="epochs per timed window")
    ap.add_argument("--torch-calls", type=int, default=2, help="torch passes per timed window")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loss", choices=("xent", "huber"), default="xent", help="the drivers' objective, all forms")
    ap.add_argument("--out", default=os.path.join("profiles", "lenet_training.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lenet_training: no GPU; a timing needs the MI355X")
    from federated_amd.engine import get_engine
    from federated_amd.local_optim import PopulationOptimizer
    from federated_amd.tf2_training import LENET1, LenetTraining, lenet_layer_shapes, lenet_size
    eng = get_engine(0)
    geom, P = LENET1, lenet_size(LENET1)
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.random((D, NT, geom[0], geom[0])).astype(np.float32)).cuda()
    labels = torch.from_numpy(rng.integers(0, geom[4], (D, NT)).astype(np.int32)).cuda()
    W0 = torch.from_numpy((0.1 * rng.standard_normal((D, P))).astype(np.float32)).cuda()
    W = W0.clone()
    shapes = lenet_layer_shapes(geom)
    tr = LenetTraining(eng, geom, x, labels, BATCH, loss=a.loss).allocate(D)
    opt = PopulationOptimizer(eng, D, shapes, "adam", 1e-3, clipnorm=1.0)
    zero = torch.zeros(D, dtype=torch.int64, device="cuda")

    offs = np.concatenate(([0], np.cumsum([int(np.prod(s)) for s in shapes])))
    x4, lab64 = x[:, :, None], labels.long()
    tgrads = torch.zeros(D, P, device="cuda")

    def torch_form():
        for d in range(D):
            ts = [W0[d, offs[i]:offs[i + 1]].reshape(shapes[i]).detach().requires_grad_() for i in range(6)]
            K1, b1, K2, b2, Wd, bd = ts
            h = F.avg_pool2d(F.relu(F.conv2d(x4[d, :BATCH], K1.permute(3, 2, 0, 1), b1)), 2)
            h = F.avg_pool2d(F.relu(F.conv2d(h, K2.permute(3, 2, 0, 1), b2)), 2)
            h = h.permute(0, 2, 3, 1).reshape(BATCH, -1)
            if a.loss == "huber":  # Huber(label, softmax(z)[label]), delta = 1
                p = torch.softmax(h @ Wd + bd, dim=1).gather(1, lab64[d, :BATCH, None])[:, 0]
                loss = F.huber_loss(p, lab64[d, :BATCH].float(), delta=1.0)
            else:
                loss = F.nll_loss(F.log_softmax(h @ Wd + bd, dim=1), lab64[d, :BATCH])
            for i, g in enumerate(torch.autograd.grad(loss, ts)):
                tgrads[d, offs[i]:offs[i + 1]] = g.reshape(-1)

    def gradients_form():
        tr.gradients(W0, first=zero)

    def epoch_form():
        tr.epoch(W, opt, a.batches)

    forms = {"gradients": (gradients_form, a.calls, 1), "epoch": (epoch_form, a.epochs, a.batches),
             "torch": (torch_form, a.torch_calls, 1)}

    def window(fn, n, per):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(n):
            fn()
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) / (n * per)  # ms per call (per batch of an epoch)

    for _ in range(a.warmup):
        for fn, n, per in forms.values():
            window(fn, n, per)
    gradients_form()
    torch.cuda.synchronize()
    apart = 0.0
    for i in range(6):
        ours, theirs = tr.grads[:, offs[i]:offs[i + 1]].double(), tgrads[:, offs[i]:offs[i + 1]].double()
        apart = max(apart, float(((ours - theirs).abs().amax(dim=1) / theirs.abs().amax(dim=1)).max()))
    times = {name: [] for name in forms}
    for _ in range(a.reps):
        for name, (fn, n, per) in forms.items():
            times[name].append(window(fn, n, per))
    med = {n: statistics.median(t) for n, t in times.items()}
    macs = macs_per_image(geom) * BATCH * D
    rec = {"tool": "lenet_training", "device": torch.cuda.get_device_name(0), "loss": a.loss, "devices": D,
           "train_images": NT,
           "batch": BATCH, "epoch_batches": a.batches, "geom": list(geom), "params": P, "reps": a.reps,
           "calls_per_window": {"gradients": a.calls, "epoch": a.epochs, "torch": a.torch_calls},
           "gradients_ms": round(med["gradients"], 4), "epoch_ms_per_batch": round(med["epoch"], 4),
           "torch_ms": round(med["torch"], 3),
           "min_ms": {n: round(min(t), 4) for n, t in times.items()},
           "max_ms": {n: round(max(t), 4) for n, t in times.items()},
           "torch_over_gradients": round(med["torch"] / med["gradients"], 1),
           "torch_over_epoch_batch": round(med["torch"] / med["epoch"], 1),
           "gradients_apart_normwise": apart, "multiply_adds": macs,
           "gradients_tmacs_per_s": round(macs / (med["gradients"] * 1e-3) / 1e12, 3)}
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
