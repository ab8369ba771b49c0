#!/usr/bin/env python3
"""PopulationOptimizer.step timed for the three rules the reference's TF2 drivers construct
(Adam with clipnorm = 1, SGD with momentum 0.9, plain SGD), at two sizes:

* ``headline``: D = 8 devices of P = 25M parameters, cut into layers like a VGG-sized model
  (13 3x3 convolutions with their biases, then dense layers that fill the bucket);
* ``driver``: D = 8 devices of the drivers' MNIST CNN (1 199 882 parameters, 8 layers).

Beside each step, in the same process and alternating window by window:

* ``mix``: the sequential mix of K = 8 neighbours on one bucket of the same P (Engine.mix_seq),
  as the streaming rate this box reaches in this hour;
* ``torch``: what a user has without the library: one torch tensor per (device, layer),
  ``clip_grad_norm_`` per tensor under Adam, then ``torch.optim.Adam`` / ``SGD`` over all of them
  (fused where torch offers it, else foreach).

Every form runs windows of ``--steps`` back-to-back calls between two device events, ending in a
synchronise; ``--warmup`` untimed windows each, then the median over ``--reps``. Reported per
rule: microseconds per step, GB/s of algorithmic bytes (PopulationOptimizer.bytes_per_step: g
counted twice under the clip), that rate over the mix's rate of the same run, and the torch
baseline's time over the step's. Prints one JSON line per size and appends it to ``--out``.
Usage: python tools/population_optim_step.py [--out profiles/population_optim_step.jsonl]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

MNIST = [(3, 3, 1, 32), (32,), (3, 3, 32, 64), (64,), (9216, 128), (128,), (128, 10), (10,)]
RULES = {"adam_clip": ("adam", dict(clipnorm=1.0)), "momentum": ("momentum", dict(momentum=0.9)), "sgd": ("sgd", {})}


def vgg_like(P):
    """VGG16's convolutions with their biases, then two dense layers that fill P."""
    shapes, cin = [], 3
    for cout in (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512):
        shapes += [(3, 3, cin, cout), (cout,)]
        cin = cout
    rows, left = divmod(P - sum(int(np.prod(s)) for s in shapes) - 4096 - 10 - 4096 * 10, 4096)
    assert rows > 0
    return shapes + [(rows, 4096), (4096,), (4096, 10), (10,)] + ([(left,)] if left else [])


def window(fn, steps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / steps  # us per call


def torch_baseline(rule, kw, w, g, table, lr):
    """One tensor per (device, layer), as a user's Keras-like models would hold them."""
    params = []
    for d in range(w.shape[0]):
        for l in range(len(table) - 1):
            p = w[d, table[l]:table[l + 1]].clone().requires_grad_(True)
            p.grad = g[d, table[l]:table[l + 1]].clone()
            params.append(p)
    if rule == "adam":
        try:
            opt, form = torch.optim.Adam(params, lr=lr, eps=1e-7, fused=True), "fused"
        except (RuntimeError, TypeError):
            opt, form = torch.optim.Adam(params, lr=lr, eps=1e-7, foreach=True), "foreach"
    else:
        opt, form = torch.optim.SGD(params, lr=lr, momentum=kw.get("momentum", 0.0), foreach=True), "foreach"

    def step():
        if rule == "adam":
            for p in params:
                torch.nn.utils.clip_grad_norm_(p, 1.0)
        opt.step()
    return step, form


def measure(eng, name, D, shapes, a):
    from federated_amd.local_optim import PopulationOptimizer, layer_offsets
    table = layer_offsets(shapes)
    P = int(table[-1])
    gen = torch.Generator(device="cuda").manual_seed(0)
    w = torch.randn(D, P, device="cuda", generator=gen)
    g = torch.randn(D, P, device="cuda", generator=gen) * 1e-2
    lr = 1e-3
    # the mix of K = 8 neighbours on one bucket of P
    K = 8
    nbrs = [torch.randn(P, device="cuda", generator=gen) for _ in range(K)]
    local, out = torch.randn(P, device="cuda", generator=gen), torch.empty(P, device="cuda")
    forms = {"mix": lambda: eng.mix_seq(out, local, nbrs, [1.0 / (K + 1)] * K)}
    opts, torch_form = {}, {}
    for key, (rule, kw) in RULES.items():
        opts[key] = PopulationOptimizer(eng, D, table, rule, lr, **kw)
        wk = w.clone()
        forms[key] = (lambda o=opts[key], x=wk: o.step(x, g))
        forms["torch_" + key], torch_form[key] = torch_baseline(rule, kw, w, g, table.tolist(), lr)
    for _ in range(a.warmup):
        for fn in forms.values():
            window(fn, a.steps)
    times = {n: [] for n in forms}
    for _ in range(a.reps):
        for n, fn in forms.items():
            times[n].append(window(fn, a.steps))
    med = {n: statistics.median(t) for n, t in times.items()}
    mix_gbps = (K + 2) * P * 4 / med["mix"] / 1e3
    rec = {"tool": "population_optim_step", "size": name, "device": torch.cuda.get_device_name(0), "D": D, "P": P,
           "layers": len(table) - 1, "steps_per_window": a.steps, "reps": a.reps,
           "mix_K8_us": round(med["mix"], 2), "mix_K8_GBps": round(mix_gbps, 1), "rules": {}}
    for key in RULES:
        nbytes = opts[key].bytes_per_step()
        gbps = nbytes / med[key] / 1e3
        rec["rules"][key] = {"us": round(med[key], 2), "min_us": round(min(times[key]), 2),
                             "max_us": round(max(times[key]), 2), "bytes": nbytes, "GBps": round(gbps, 1),
                             "over_mix_rate": round(gbps / mix_gbps, 3), "torch_form": torch_form[key],
                             "torch_us": round(med["torch_" + key], 2),
                             "torch_over_step": round(med["torch_" + key] / med[key], 2)}
    line = json.dumps(rec)
    print(line, flush=True)
    with open(a.out, "a") as fh:
        fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10, help="calls per timed window")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "population_optim_step.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("population_optim_step: no GPU; a timing needs the MI355X")
    from federated_amd.engine import get_engine
    eng = get_engine(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    measure(eng, "headline", 8, vgg_like(25_000_000), a)
    torch.cuda.empty_cache()
    measure(eng, "driver", 8, MNIST, a)


if __name__ == "__main__":
    main()
