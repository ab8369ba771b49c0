#!/usr/bin/env python3
"""One local epoch of the config-3 population (16 devices, CNN, 24 samples of 512 inputs per
device, the drivers' slicing: 4 minibatches of 4 rows at a stride of 5) timed in two forms:

* ``one_launch``: Engine.local_sgd, the whole population's epoch in one launch;
* ``chain``: what the library offered before that entry point: per minibatch one
  Engine.grad_rows launch plus one torch AXPY, driven from Python (``chain_ws``: the same with
  the batch-split workspace, i.e. a gradient launch and its reduction launch per minibatch).

Every form runs windows of ``--epochs`` back-to-back epochs from the same starting models,
between two device events and ending in a synchronise; the forms alternate window by window
after ``--warmup`` untimed windows each. Reported: the median window over ``--reps``, per epoch,
in microseconds, the chain's median over the single launch's, and how far the two forms' models
are apart after one epoch. Prints one JSON line and appends it to ``--out``.
Usage: python tools/local_sgd_epoch.py [--out profiles/local_sgd_epoch.jsonl]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

GEOM = {"filter": 16, "number": 8, "stride": 5}
D, NS, L, C, P = 16, 24, 512, 8, 1488
STRIDE, ROWS, STEPS = 5, 4, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=200, help="epochs per timed window")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--out", default=os.path.join("profiles", "local_sgd_epoch.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("local_sgd_epoch: no GPU; a timing needs the MI355X")
    from federated_amd.engine import get_engine
    eng = get_engine(0)
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.standard_normal((D, NS, L)).astype(np.float32)).cuda()
    y = torch.from_numpy(np.eye(C, dtype=np.float32)[rng.integers(0, C, (D, NS))]).cuda()
    W0 = torch.from_numpy((rng.standard_normal((D, P)) * 0.1).astype(np.float32)).cuda()
    W = torch.empty_like(W0)
    cost = torch.zeros(D, dtype=torch.float64, device="cuda")
    G = torch.empty(D, P, device="cuda")
    rows = torch.arange(D, dtype=torch.int32, device="cuda")
    # the chain's minibatches, cut out ahead of the timed windows (grad_rows takes contiguous rows)
    xb = [x[:, STRIDE * i:STRIDE * i + ROWS].contiguous() for i in range(STEPS)]
    yb = [y[:, STRIDE * i:STRIDE * i + ROWS].contiguous() for i in range(STEPS)]
    ws = eng.grad_workspace(D, ROWS, P)
    lr = float(np.float32(a.lr))

    def one_launch():
        eng.local_sgd(1, x, y, W, GEOM, STRIDE, ROWS, STEPS, lr, True, cost)

    def chain(workspace=None):
        for i in range(STEPS):
            eng.grad_rows(1, xb[i], yb[i], W, rows, rows, G, GEOM, workspace=workspace)
            W.sub_(G, alpha=lr)

    forms = {"one_launch": one_launch, "chain": chain, "chain_ws": lambda: chain(ws)}

    def window(fn):
        W.copy_(W0)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(a.epochs):
            fn()
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) * 1e3 / a.epochs  # us per epoch

    after = {}
    for name, fn in forms.items():  # results first: one epoch of each form from the same models
        W.copy_(W0)
        fn()
        torch.cuda.synchronize()
        after[name] = W.clone()
    scale = float(after["chain"].abs().max())
    apart = {n: float((after[n] - after["chain"]).abs().max()) / scale for n in ("one_launch", "chain_ws")}
    for _ in range(a.warmup):
        for fn in forms.values():
            window(fn)
    times = {n: [] for n in forms}
    for _ in range(a.reps):
        for n, fn in forms.items():
            times[n].append(window(fn))
    med = {n: statistics.median(t) for n, t in times.items()}
    rec = {"tool": "local_sgd_epoch", "device": torch.cuda.get_device_name(0), "devices": D, "samples": NS,
           "steps": STEPS, "batch_stride": STRIDE, "batch_rows": ROWS, "epochs_per_window": a.epochs, "reps": a.reps,
           "one_launch_us": round(med["one_launch"], 2), "chain_us": round(med["chain"], 2),
           "chain_ws_us": round(med["chain_ws"], 2),
           "min_us": {n: round(min(t), 2) for n, t in times.items()},
           "max_us": {n: round(max(t), 2) for n, t in times.items()},
           "chain_over_one_launch": round(med["chain"] / med["one_launch"], 2),
           "chain_ws_over_one_launch": round(med["chain_ws"] / med["one_launch"], 2),
           "models_apart_normwise": apart}
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
