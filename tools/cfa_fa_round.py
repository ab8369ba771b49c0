#!/usr/bin/env python3
"""One CFA-FA server epoch (cfa_fa_population_round_f32, Engine.cfa_fa_round) timed at three
shapes: D = 5, P = 1 488 (the driver's), D = 16, P = 16 680, and D = 8, P = 25 000 000.

Beside it, in the same process and alternating window by window:

* ``torch``: the same epoch written in torch fp64 on the device (D chained fold steps on an fp64
  vector, then the client step on the widened stack and one cast): what a resident population had
  before the kernel;
* ``fedavg``: ``cfa_fedavg_population_round_f32`` with ``client="mix"`` on the same D and P: the
  same traffic pattern in fp32 (every row read for the fold, read again and written by the client
  rule, the global model read and written).

Every form runs windows of ``--steps`` back-to-back calls between two device events, ending in a
synchronise; ``--warmup`` untimed windows each, then the median over ``--reps``. Reported per
shape: microseconds per epoch, GB/s of algorithmic bytes (server epoch 2 D P 4 + 16 P; FedAvg round
``bytes_per_round``), the server epoch's rate over the FedAvg round's, the torch form's time over
the kernel's, and the FedAvg round's own spread (min and max window over its median). At the long
shape the launch shapes u = 2 / 4 and batch = 4 / 8 are timed too (``shapes``). Prints one JSON line
per shape and appends it to ``--out``.
Usage: python tools/cfa_fa_round.py [--out profiles/cfa_fa_round.jsonl]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = [("driver", 5, 1488), ("mid", 16, 16680), ("long", 8, 25_000_000)]
EPS, EPS2 = 1.0, 0.5  # the driver's defaults


def window(fn, steps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / steps  # us per call


def torch_epoch(x, out, s, coef, eps2):
    """The server epoch in torch fp64, operation by operation as the driver's numpy."""
    D = x.shape[0]

    def run():
        for d in range(D):
            s.add_((x[d].double() - s).mul_(coef[d]))
        w = x.double()
        out.copy_(w + (s - w).mul_(eps2))
    return run


def env_shape(fn, **env):
    """``fn`` under the launch-shape overrides the library reads at every launch."""
    def run():
        os.environ.update(env)
        try:
            fn()
        finally:
            for k in env:
                del os.environ[k]
    return run


def measure(eng, name, D, P, a):
    from federated_amd import _lib
    from federated_amd.fedavg_population import FedAvgPopulation
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(D, P, device="cuda", generator=gen) * 0.1
    out = torch.empty_like(x)
    s = torch.randn(P, device="cuda", generator=gen, dtype=torch.float64) * 0.1
    bal = np.ones(D) * (1 / D)
    coef = torch.from_numpy(np.asarray([EPS * b for b in bal])).cuda()
    coef_host = [float(c) for c in coef.cpu()]
    kernel = lambda: eng.cfa_fa_round(out, x, s, coef, EPS2, _lib.FA_ROUND)
    fed = FedAvgPopulation(eng, x.clone(), torch.zeros(P, device="cuda"), 1.0)
    fed.set_schedule([list(range(D))], client="mix", client_factor=EPS2, client_divisor=1.0)
    forms = {"kernel": kernel, "fedavg": fed.round, "torch": torch_epoch(x, out, s.clone(), coef_host, EPS2)}
    if name == "long":
        for u in ("2", "4"):
            for b in ("4", "8"):
                forms[f"kernel_u{u}_b{b}"] = env_shape(kernel, CFA_FA_U=u, CFA_FA_BATCH=b)
    for _ in range(a.warmup):
        for fn in forms.values():
            window(fn, a.steps)
    times = {n: [] for n in forms}
    for _ in range(a.reps):
        for n, fn in forms.items():
            times[n].append(window(fn, a.steps))
    med = {n: statistics.median(t) for n, t in times.items()}
    nbytes = 2 * D * P * 4 + 16 * P
    fed_bytes = fed.bytes_per_round()
    gbps, fed_gbps = nbytes / med["kernel"] / 1e3, fed_bytes / med["fedavg"] / 1e3
    rec = {"tool": "cfa_fa_round", "shape": name, "device": torch.cuda.get_device_name(0), "D": D, "P": P,
           "steps_per_window": a.steps, "reps": a.reps,
           "kernel_us": round(med["kernel"], 2), "kernel_min_us": round(min(times["kernel"]), 2),
           "kernel_max_us": round(max(times["kernel"]), 2), "bytes": nbytes, "kernel_GBps": round(gbps, 1),
           "fedavg_mix_us": round(med["fedavg"], 2), "fedavg_bytes": fed_bytes, "fedavg_GBps": round(fed_gbps, 1),
           "fedavg_spread": [round(min(times["fedavg"]) / med["fedavg"], 3), round(max(times["fedavg"]) / med["fedavg"], 3)],
           "kernel_over_fedavg_rate": round(gbps / fed_gbps, 3),
           "torch_fp64_us": round(med["torch"], 2), "torch_over_kernel": round(med["torch"] / med["kernel"], 2)}
    shapes = {n[len("kernel_"):]: round(nbytes / med[n] / 1e3, 1) for n in forms if n.startswith("kernel_")}
    if shapes:
        rec["shapes_GBps"] = shapes
    line = json.dumps(rec)
    print(line, flush=True)
    with open(a.out, "a") as fh:
        fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10, help="calls per timed window")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "cfa_fa_round.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cfa_fa_round: no GPU; a timing needs the MI355X")
    from federated_amd.engine import get_engine
    eng = get_engine(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for name, D, P in SHAPES:
        measure(eng, name, D, P, a)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
