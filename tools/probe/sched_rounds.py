#!/usr/bin/env python3
"""What a time-varying topology costs per round, three ways (and one static run for scale), at the
reference's model sizes:

  a  set_topology(lists of the round) + run() per round, eager: the only route before topology
     schedules (CSR rebuilt on the host, three uploads, one launch from Python);
  b  set_schedule once, rounds(R, graph=False): tables and round counter on the device, every
     round launched from Python;
  c  set_schedule once, rounds(R, graph=True): captured periods replayed;
  d  for scale, not a route for these runs: ONE fixed table, set_topology once, rounds(R,
     graph=True). (c) minus (d) is what the table lookup and the counter's own launch cost.

Shapes: D = 16, P = 24 622 (FL_CFA_CNN_tf2 bucket), TF1 numerics, cfa_ongraphs draws of 3
neighbours; D = 8, P = 1 488 (CFA-GE CNN bucket), the TF2 rule. T = S = 111 tables each (the
length of the reference's vGraph.mat), from topology.mobile on a seeded random adjacency tensor.

Every leg runs in a fresh process (this script starts them one after the other and never opens
the GPU itself): warm-up rounds (code objects, graph capture), then HIP events around the whole
loop of R = 2 000 rounds, PASSES times; the median is reported. One JSON line per leg, then one
line of ratios per shape with (a) as the baseline, appended to --out."""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

NAME = "tools/probe/sched_rounds.py"
SHAPES = {
    "D16_P24622_tf1": dict(D=16, P=24_622, T=111, numerics="tf1", max_neighbors=3),
    "D8_P1488_fp32": dict(D=8, P=1_488, T=111, numerics="fp32", max_neighbors=2),
}
LEGS = ("a_set_topology_eager", "b_schedule_eager", "c_schedule_graph", "d_static_graph")
R = int(os.environ.get("SCHED_ROUNDS", "2000"))
PASSES = int(os.environ.get("SCHED_PASSES", "5"))
WARMUP = 96  # rounds: a multiple of both graph blocks (16 rounds of 2, as PopulationRound captures)


def leg(shape: str, which: str) -> dict:
    import numpy as np
    import torch

    from federated_amd import topology as T
    from federated_amd.engine import get_engine
    s = SHAPES[shape]
    D, P, Tn = s["D"], s["P"], s["T"]
    rng = np.random.default_rng(D * 1000 + Tn)
    graph = (rng.random((D, D, Tn)) < 0.5).astype(np.uint8)
    for g in range(Tn):
        np.fill_diagonal(graph[:, :, g], 0)
    draw = random.Random(D)
    tables = [T.mobile(graph, g, max_neighbors=s["max_neighbors"], rng=draw) for g in range(Tn)]
    policy = T.alphas_tf1_ongraphs(1.0) if s["numerics"] == "tf1" else T.alphas_tf2
    models = torch.empty((D, P), dtype=torch.float32, device="cuda").normal_(
        generator=torch.Generator(device="cuda").manual_seed(3))
    pr = T.PopulationRound(get_engine(0), models)
    if which == LEGS[0]:
        def rounds(n, first):
            for r in range(first, first + n):
                pr.set_topology(tables[r % Tn], policy, use_window=False, numerics=s["numerics"])
                pr.run()
    elif which == LEGS[3]:
        pr.set_topology(tables[0], policy, use_window=False, numerics=s["numerics"])

        def rounds(n, first):
            pr.rounds(n, graph=True)
    else:
        pr.set_schedule(tables, policy, numerics=s["numerics"])
        graph_replay = which == LEGS[2]

        def rounds(n, first):
            pr.rounds(n, graph=graph_replay)
    rounds(WARMUP, 0)
    torch.cuda.synchronize()
    us = []
    for p in range(PASSES):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rounds(R, WARMUP + p * R)
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / R)
    out = {"experiment": NAME, "shape": shape, "leg": which, "devices": D, "P": P, "tables": Tn, "slots": Tn,
           "numerics": s["numerics"], "rounds": R, "us_per_round": round(statistics.median(us), 3),
           "us_per_round_passes": [round(u, 3) for u in us], "device": torch.cuda.get_device_name(0)}
    if which in LEGS[1:3]:
        out["round_index"] = pr.round_index
        assert out["round_index"] == WARMUP + PASSES * R
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_sched_rounds.jsonl"))
    ap.add_argument("--leg", nargs=2, metavar=("SHAPE", "LEG"), help="run one leg in this process and print its line")
    args = ap.parse_args()
    if args.leg:
        print(json.dumps(leg(*args.leg)), flush=True)
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as fh:
        for shape in SHAPES:
            us = {}
            for which in LEGS:  # a fresh process per leg, one at a time
                res = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", shape, which],
                                     capture_output=True, text=True, timeout=600)
                if res.returncode != 0:
                    sys.stderr.write(res.stdout + res.stderr)
                    raise SystemExit(f"{shape} {which}: exit status {res.returncode}")
                line = [l for l in res.stdout.splitlines() if l.startswith("{")][-1]
                us[which] = json.loads(line)["us_per_round"]
                fh.write(line + "\n")
                fh.flush()
                print(line, flush=True)
            ratios = {"experiment": NAME, "shape": shape, "leg": "ratios", "baseline": LEGS[0],
                      "a_over_c": round(us[LEGS[0]] / us[LEGS[2]], 2), "b_over_c": round(us[LEGS[1]] / us[LEGS[2]], 2),
                      "a_over_b": round(us[LEGS[0]] / us[LEGS[1]], 2),
                      "c_minus_d_us": round(us[LEGS[2]] - us[LEGS[3]], 3)}
            fh.write(json.dumps(ratios) + "\n")
            fh.flush()
            print(json.dumps(ratios), flush=True)


if __name__ == "__main__":
    main()
