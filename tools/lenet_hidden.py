#!/usr/bin/env python3
"""One batch gradient and one validation pass of a population of the CIFAR drivers' hidden-layer
LeNet (CIFAR_LENET, seven numbers; 16 devices, batches of 100, 10 000 shared test images) timed
beside what a caller has without them, on the same images and models:

* ``gradients``: LenetTraining.gradients, one cfa_lenet_hidden_grad_loss_f32 call (two launches);
* ``validate``: LenetValidation.validate, one cfa_lenet_hidden_eval_loss_f32 call (two launches);
* ``torch_gradients`` / ``torch_validate``: D sequential torch-ROCm passes of the same model
  (conv2d, avg_pool2d, two matmuls, log_softmax), with autograd.grad and the eight gradients
  copied into a [D, P] stack, or forward only over the test set's batches.

Every form runs windows of back-to-back calls between two device events, ending in a synchronise;
the forms alternate window by window after ``--warmup`` untimed windows each. Reported per
geometry: the median window over ``--reps`` per call in milliseconds with its extremes, torch's
median over the device's, and how far the two forms' gradients and costs are apart normwise.
Prints one JSON line per geometry and appends it to ``--out``.
Usage: python tools/lenet_hidden.py [--out profiles/lenet_hidden.jsonl]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

D, NT, BATCH, N_TEST = 16, 800, 100, 10000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10, help="device calls per timed window")
    ap.add_argument("--torch-calls", type=int, default=1, help="torch passes per timed window")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "lenet_hidden.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lenet_hidden: no GPU; a timing needs the MI355X")
    from federated_amd.engine import get_engine
    from federated_amd.tf2_training import CIFAR_LENET, LenetTraining, lenet_layer_shapes, lenet_size
    from federated_amd.tf2_validation import LenetValidation
    eng = get_engine(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for geom in (CIFAR_LENET,):
        P, shapes = lenet_size(geom), lenet_layer_shapes(geom)
        rng = np.random.default_rng(0)
        x = torch.from_numpy(rng.random((D, NT, geom[0], geom[0], geom[1])).astype(np.float32)).cuda()
        labels = torch.from_numpy(rng.integers(0, geom[6], (D, NT)).astype(np.int32)).cuda()
        xt = torch.from_numpy(rng.random((N_TEST, geom[0], geom[0], geom[1])).astype(np.float32)).cuda()
        lt = torch.from_numpy(rng.integers(0, geom[6], N_TEST).astype(np.int32)).cuda()
        W0 = torch.from_numpy((0.1 * rng.standard_normal((D, P))).astype(np.float32)).cuda()
        tr = LenetTraining(eng, geom, x, labels, BATCH).allocate(D)
        val = LenetValidation(eng, geom, xt, lt, BATCH).allocate(D)
        zero = torch.zeros(D, dtype=torch.int64, device="cuda")
        offs = np.concatenate(([0], np.cumsum([int(np.prod(s)) for s in shapes])))
        x4, lab64 = x.permute(0, 1, 4, 2, 3).contiguous(), labels.long()  # NCHW for torch, converted once
        xt4, lt64 = xt.permute(0, 3, 1, 2).contiguous(), lt.long()
        tgrads = torch.zeros(D, P, device="cuda")
        tcost = torch.zeros(D, dtype=torch.float64, device="cuda")

        def logits(ts, images):
            K1, b1, K2, b2, Wh, bh, Wd, bd = ts
            h = F.avg_pool2d(F.relu(F.conv2d(images, K1.permute(3, 2, 0, 1), b1)), 2)
            h = F.avg_pool2d(F.relu(F.conv2d(h, K2.permute(3, 2, 0, 1), b2)), 2)
            return F.relu(h.permute(0, 2, 3, 1).reshape(images.shape[0], -1) @ Wh + bh) @ Wd + bd

        def torch_gradients():
            for d in range(D):
                ts = [W0[d, offs[i]:offs[i + 1]].reshape(shapes[i]).detach().requires_grad_() for i in range(8)]
                loss = F.nll_loss(F.log_softmax(logits(ts, x4[d, :BATCH]), dim=1), lab64[d, :BATCH])
                for i, g in enumerate(torch.autograd.grad(loss, ts)):
                    tgrads[d, offs[i]:offs[i + 1]] = g.reshape(-1)

        def torch_validate():
            with torch.no_grad():
                for d in range(D):
                    ts = [W0[d, offs[i]:offs[i + 1]].reshape(shapes[i]) for i in range(8)]
                    acc = torch.zeros((), dtype=torch.float64, device="cuda")
                    for b in range(val.batches):
                        s = slice(b * BATCH, (b + 1) * BATCH)
                        acc += F.nll_loss(F.log_softmax(logits(ts, xt4[s]), dim=1), lt64[s]).double()
                    tcost[d] = acc / val.batches

        forms = {"gradients": (lambda: tr.gradients(W0, first=zero), a.calls),
                 "validate": (lambda: val.validate(W0), a.calls),
                 "torch_gradients": (torch_gradients, a.torch_calls), "torch_validate": (torch_validate, a.torch_calls)}

        def window(fn, n):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(n):
                fn()
            end.record()
            torch.cuda.synchronize()
            return start.elapsed_time(end) / n  # ms per call

        for _ in range(a.warmup):
            for fn, n in forms.values():
                window(fn, n)
        torch.cuda.synchronize()
        apart = 0.0
        for i in range(8):
            ours, theirs = tr.grads[:, offs[i]:offs[i + 1]].double(), tgrads[:, offs[i]:offs[i + 1]].double()
            apart = max(apart, float(((ours - theirs).abs().amax(dim=1) / theirs.abs().amax(dim=1)).max()))
        cost_apart = float((val.val_cost - tcost).abs().max() / tcost.abs().max())
        times = {name: [] for name in forms}
        for _ in range(a.reps):
            for name, (fn, n) in forms.items():
                times[name].append(window(fn, n))
        med = {n: statistics.median(t) for n, t in times.items()}
        rec = {"tool": "lenet_hidden", "device": torch.cuda.get_device_name(0), "geom": list(geom), "params": P,
               "devices": D, "batch": BATCH, "test_images": N_TEST, "reps": a.reps,
               "calls_per_window": {n: c for n, (_, c) in forms.items()},
               "median_ms": {n: round(v, 4) for n, v in med.items()},
               "min_ms": {n: round(min(t), 4) for n, t in times.items()},
               "max_ms": {n: round(max(t), 4) for n, t in times.items()},
               "torch_over_gradients": round(med["torch_gradients"] / med["gradients"], 2),
               "torch_over_validate": round(med["torch_validate"] / med["validate"], 2),
               "gradients_apart_normwise": apart, "costs_apart_normwise": cost_apart,
               "grad_workspace_bytes": int(tr.workspace.numel() * 4)}
        line = json.dumps(rec)
        print(line, flush=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
