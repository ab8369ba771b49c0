#!/usr/bin/env python3
"""What a FedAvg parameter-server round on a device-resident population costs, three ways:

  a  the composition from Python that was the only route before FedAvgPopulation: the round's
     active list taken from indexes_tx on the host (parameter_server_v2.py:88), one
     Engine.mix_seq_div over the active rows (chained through ``out`` in 16-wide passes), then D
     row copies of the new global model;
  b  FedAvgPopulation.round(), eager: one launch per round, lists and round counter on the device;
  c  FedAvgPopulation.rounds(R): the same rounds replayed from graphs.

Shapes: D = 128 x P = 25M at C = 16 and C = 128; 32 x 1 071 748 at C = 8; 16 x 2 202 (the TF2
lenet-1) at C = 4. E = 16 epochs of active lists, each a draw of C devices without replacement.
Client rule: copy.

All legs of a shape run in one process, alternating: after a warm-up (code objects, graph
capture), PASSES passes, each timing R rounds of every leg in turn with HIP events. A leg's
figure is the median of its passes; ``a_spread`` is (max - min) / median over the passes of (a),
the box's own noise, and "not slower" below means within that spread. Each line carries the bytes
a round moves (FedAvgPopulation.bytes_per_round) and the fraction of the 8 TB/s HBM peak they give
at the measured time. ``--sweep`` adds the launch shapes (float4 per lane, rows per load batch,
workgroups per CU) of leg (b) on the first shape, through the library's CFA_FEDAVG_* overrides.
One JSON line per leg and one of ratios per shape, appended to --out."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

NAME = "tools/probe/fedavg_round.py"
PEAK_BYTES_PER_S = 8e12
SHAPES = {
    "D128_P25M_C16": dict(D=128, P=25_000_000, C=16, R=12),
    "D128_P25M_C128": dict(D=128, P=25_000_000, C=128, R=8),
    "D32_P1071748_C8": dict(D=32, P=1_071_748, C=8, R=200),
    "D16_P2202_C4": dict(D=16, P=2_202, C=4, R=1000),
}
EPOCHS = 16
PASSES = int(os.environ.get("FEDAVG_PASSES", "5"))
U_FACTOR = 0.9


def _time(fn, rounds):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn(rounds)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / rounds


def run_shape(shape: str, sweep: bool):
    import numpy as np
    import torch

    from federated_amd.engine import get_engine
    from federated_amd.fedavg_population import FedAvgPopulation
    s = SHAPES[shape]
    D, P, C, R = s["D"], s["P"], s["C"], s["R"]
    eng = get_engine(0)
    rng = np.random.default_rng(D * 1000 + C)
    tx = np.stack([rng.permutation(D)[:C] for _ in range(EPOCHS)], axis=1)  # indexes_tx [C, E]
    gen = torch.Generator(device="cuda").manual_seed(5)
    pitch = (P + 3) // 4 * 4
    models = torch.empty((D, pitch), dtype=torch.float32, device="cuda").normal_(generator=gen)[:, :P]
    params = torch.empty(P, dtype=torch.float32, device="cuda").normal_(generator=gen)
    pop = FedAvgPopulation(eng, models, params, U_FACTOR)
    pop.set_schedule(tx, client="copy")
    moved = pop.bytes_per_round()

    # leg (a): its own global model and spare bucket, the same stack
    state = {"p": params.clone(), "out": torch.empty_like(params), "epoch": 0}

    def leg_a(n):
        for _ in range(n):
            ids = tx[:, state["epoch"] % EPOCHS]  # the host-built active list of the round
            state["epoch"] += 1
            eng.mix_seq_div(state["out"], state["p"], [models[int(k)] for k in ids], [U_FACTOR] * C, [float(C)] * C)
            state["p"], state["out"] = state["out"], state["p"]
            for d in range(D):
                models[d].copy_(state["p"])

    legs = {"a_composed_eager": leg_a, "b_population_eager": lambda n: pop.rounds(n, graph=False),
            "c_population_graph": lambda n: pop.rounds(n, graph=True)}
    for fn in legs.values():  # warm-up: code objects, and the graphs of 1 and 8 rounds
        fn(max(R, 9))
    torch.cuda.synchronize()
    us = {k: [] for k in legs}
    for _ in range(PASSES):
        for k, fn in legs.items():
            us[k].append(_time(fn, R))
    lines = []
    med = {k: statistics.median(v) for k, v in us.items()}
    for k in legs:
        lines.append({"experiment": NAME, "shape": shape, "leg": k, "devices": D, "P": P, "active": C,
                      "rounds": R, "us_per_round": round(med[k], 3), "us_per_round_passes": [round(u, 3) for u in us[k]],
                      "moved_bytes": moved, "frac_of_8TBps": round(moved / (med[k] * 1e-6) / PEAK_BYTES_PER_S, 4),
                      "device": torch.cuda.get_device_name(0)})
    a = us["a_composed_eager"]
    spread = (max(a) - min(a)) / med["a_composed_eager"]
    lines.append({"experiment": NAME, "shape": shape, "leg": "ratios", "baseline": "a_composed_eager",
                  "a_over_c": round(med["a_composed_eager"] / med["c_population_graph"], 2),
                  "b_over_c": round(med["b_population_eager"] / med["c_population_graph"], 2),
                  "a_over_b": round(med["a_composed_eager"] / med["b_population_eager"], 2),
                  "a_spread": round(spread, 4),
                  "b_not_slower_than_a": bool(med["b_population_eager"] <= med["a_composed_eager"] * (1 + spread)),
                  "c_not_slower_than_b": bool(med["c_population_graph"] <= med["b_population_eager"] * (1 + spread)),
                  "frac_of_8TBps_c": lines[2]["frac_of_8TBps"]})
    if sweep:
        for u in (1, 2, 4):
            for batch in (4, 8):
                for wg in (1, 2, 4, 8):
                    os.environ.update(CFA_FEDAVG_U=str(u), CFA_FEDAVG_BATCH=str(batch), CFA_FEDAVG_WG_PER_CU=str(wg))
                    legs["b_population_eager"](2)
                    t = statistics.median(_time(legs["b_population_eager"], R) for _ in range(3))
                    lines.append({"experiment": NAME, "shape": shape, "leg": "sweep", "u": u, "batch": batch,
                                  "wg_per_cu": wg, "us_per_round": round(t, 3),
                                  "frac_of_8TBps": round(moved / (t * 1e-6) / PEAK_BYTES_PER_S, 4)})
        for k in ("CFA_FEDAVG_U", "CFA_FEDAVG_BATCH", "CFA_FEDAVG_WG_PER_CU"):
            del os.environ[k]
    return lines


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_fedavg_round.jsonl"))
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--sweep", action="store_true", help="launch-shape sweep of leg (b) on the first shape")
    args = ap.parse_args()
    import torch
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as fh:
        for i, shape in enumerate(args.shapes):
            for line in run_shape(shape, args.sweep and i == 0):
                fh.write(json.dumps(line) + "\n")
                fh.flush()
                print(json.dumps(line), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
