#!/usr/bin/env python3
"""One validation pass of a TF2 LeNet-1 population at the MNIST driver's defaults (30 devices, the
shared test set of 10 000 images, batches of 100: 100 forward batches per device) timed in two
forms on the same images and models:

* ``device``: LenetValidation.validate, the whole population in one cfa_lenet_eval_f32 call (two
  launches);
* ``torch``: what a user of the device-resident populations has without it: D sequential
  torch-ROCm forward passes (conv2d, avg_pool2d, matmul, log_softmax) in batches of 100, the
  batch losses averaged on the device, one read-back of the D costs at the end.

Every form runs windows of back-to-back passes (``--passes`` / ``--torch-passes``) between two
device events and ending in a synchronise; the forms alternate window by window after
``--warmup`` untimed windows each. Reported: the median window over ``--reps``, per pass, in
milliseconds, torch's median over the device's, how far the two forms' costs are apart, and the
device form's multiply-add rate from the shapes. ``--loss huber`` times both forms on the Huber
drivers' objective instead of the cross-entropy one. Prints one JSON line and appends it to ``--out``.
Usage: python tools/lenet_validation.py [--loss xent|huber] [--out profiles/lenet_validation.jsonl]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

D, NT, BATCH = 30, 10000, 100


def macs_per_image(geom):
    side, k, c1, c2, classes = geom
    s1 = side - k + 1
    p1 = s1 // 2
    s2 = p1 - k + 1
    p2 = s2 // 2
    return s1 * s1 * c1 * k * k + s2 * s2 * c2 * k * k * c1 + p2 * p2 * c2 * classes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=20, help="device passes per timed window")
    ap.add_argument("--torch-passes", type=int, default=1, help="torch passes per timed window")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loss", choices=("xent", "huber"), default="xent", help="the drivers' objective, both forms")
    ap.add_argument("--out", default=os.path.join("profiles", "lenet_validation.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lenet_validation: no GPU; a timing needs the MI355X")
    from federated_amd.engine import get_engine
    from federated_amd.tf2_validation import LENET1, LenetValidation, lenet_layer_shapes, lenet_size
    eng = get_engine(0)
    geom, P = LENET1, lenet_size(LENET1)
    batches = NT // BATCH
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.random((NT, geom[0], geom[0])).astype(np.float32)).cuda()
    labels = torch.from_numpy(rng.integers(0, geom[4], NT).astype(np.int32)).cuda()
    W = torch.from_numpy((0.1 * rng.standard_normal((D, P))).astype(np.float32)).cuda()
    val = LenetValidation(eng, geom, x, labels, BATCH, loss=a.loss).allocate(D)

    # the torch form's tensors, cut out ahead of the timed windows
    shapes = lenet_layer_shapes(geom)
    offs = np.concatenate(([0], np.cumsum([int(np.prod(s)) for s in shapes])))
    layers = []
    for d in range(D):
        K1, b1, K2, b2, Wd, bd = (W[d, offs[i]:offs[i + 1]].reshape(shapes[i]) for i in range(6))
        layers.append((K1.permute(3, 2, 0, 1).contiguous(), b1, K2.permute(3, 2, 0, 1).contiguous(), b2, Wd, bd))
    x4 = x[:, None]
    lab64 = labels.long()
    tcost = torch.zeros(D, dtype=torch.float64, device="cuda")

    def device_form():
        val.validate(W)

    def torch_form():
        for d, (K1, b1, K2, b2, Wd, bd) in enumerate(layers):
            acc = torch.zeros((), dtype=torch.float64, device="cuda")
            for b in range(batches):
                sl = slice(b * BATCH, (b + 1) * BATCH)
                h = F.avg_pool2d(F.relu(F.conv2d(x4[sl], K1, b1)), 2)
                h = F.avg_pool2d(F.relu(F.conv2d(h, K2, b2)), 2)
                h = h.permute(0, 2, 3, 1).reshape(BATCH, -1)
                if a.loss == "huber":  # Huber(label, softmax(z)[label]), delta = 1
                    p = torch.softmax(h @ Wd + bd, dim=1).gather(1, lab64[sl, None])[:, 0]
                    acc += F.huber_loss(p, lab64[sl].float(), delta=1.0).double()
                else:
                    lp = F.log_softmax(h @ Wd + bd, dim=1)
                    acc += F.nll_loss(lp, lab64[sl]).double()
            tcost[d] = acc / batches

    forms = {"device": (device_form, a.passes), "torch": (torch_form, a.torch_passes)}

    def window(fn, n):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(n):
            fn()
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) / n  # ms per pass

    for _ in range(a.warmup):
        for fn, n in forms.values():
            window(fn, n)
    apart = float((val.val_cost - tcost).abs().max() / tcost.abs().max())
    times = {name: [] for name in forms}
    for _ in range(a.reps):
        for name, (fn, n) in forms.items():
            times[name].append(window(fn, n))
    med = {n: statistics.median(t) for n, t in times.items()}
    macs = macs_per_image(geom) * BATCH * batches * D
    rec = {"tool": "lenet_validation", "device": torch.cuda.get_device_name(0), "loss": a.loss, "devices": D,
           "test_images": NT,
           "batch": BATCH, "batches": batches, "geom": list(geom), "params": P, "reps": a.reps,
           "passes_per_window": {"device": a.passes, "torch": a.torch_passes},
           "device_ms": round(med["device"], 4), "torch_ms": round(med["torch"], 3),
           "min_ms": {n: round(min(t), 4) for n, t in times.items()},
           "max_ms": {n: round(max(t), 4) for n, t in times.items()},
           "torch_over_device": round(med["torch"] / med["device"], 1),
           "costs_apart_normwise": apart, "multiply_adds": macs,
           "device_tmacs_per_s": round(macs / (med["device"] * 1e-3) / 1e12, 3)}
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
