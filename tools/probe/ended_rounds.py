#!/usr/bin/env python3
"""What the training_end rule costs on a device-resident population (PopulationRound with
set_ended_rule("copy"), cfa_mix_population_ended_f32), per round, five ways on the same tables:

  p  the existing round (rule off, cfa_mix_population_f32), replayed from graphs;
  n  the new kernel with every flag clear, replayed from graphs: n / p is what the flag scan costs
     when nobody has ended;
  a  the host-driven form the rule replaces, one quarter of the devices ended: read the flags
     back, truncate the lists on the host (an ended device and one that copies get an empty list,
     which copies their own row), set_topology, one existing round, then a torch row copy for
     every device that takes an ended neighbour's model;
  b  the new round with the same flags, eager: one launch per round, nothing read back;
  c  the same rounds replayed from graphs.

Shapes: 16 x 24 622 (K = 2), 32 x 1 071 748 (K = 4), 128 x 25M (K = 8); kregular_v3 lists, eps =
1/(n+1); every fourth device ended, flags fixed (propagate=False). All legs of a shape share one
pair of [D, P] stacks and run in one process, alternating: after a warm-up (code objects, graph
capture), PASSES passes, each timing R rounds of every leg in turn with HIP events. A leg's figure
is the median of its passes, its ``spread`` (max - min) / median over them: the box's own noise,
and "not slower" below means within the named leg's spread. Legs b and c carry the bytes a round
moves (2 P 4 for an ended or copying device, (m + 2) P 4 for one that folds m rows) and the
fraction of the 8 TB/s HBM peak they give at the measured time. One JSON line per leg and one of
ratios per shape, appended to --out."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

NAME = "tools/probe/ended_rounds.py"
PEAK_BYTES_PER_S = 8e12
SHAPES = {
    "D16_P24622_K2": dict(D=16, P=24_622, K=2, R=400),
    "D32_P1071748_K4": dict(D=32, P=1_071_748, K=4, R=64),
    "D128_P25M_K8": dict(D=128, P=25_000_000, K=8, R=16),
}
PASSES = int(os.environ.get("ENDED_PASSES", "5"))


def _time(fn, rounds):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn(rounds)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / rounds


def run_shape(shape: str):
    import torch

    from federated_amd import topology as T
    from federated_amd.engine import get_engine
    s = SHAPES[shape]
    D, P, K, R = s["D"], s["P"], s["K"], s["R"]
    assert R % 16 == 0  # whole graph blocks, and no odd round's copy back into ``models``
    eng = get_engine(0)
    lists = T.kregular_v3(D, K)
    ended = list(range(0, D, 4))
    gen = torch.Generator(device="cuda").manual_seed(12)
    models = torch.empty((D, P), dtype=torch.float32, device="cuda").normal_(generator=gen)
    out = torch.empty_like(models)

    def population(rule, ids=()):
        pr = T.PopulationRound(eng, models, out)
        pr.set_ended_rule(rule)
        pr.set_topology(lists, T.alphas_tf2, use_window=False)
        pr.set_ended(ids)
        return pr

    plain, clear, flagged = population(None), population("copy"), population("copy", ended)
    # leg (a): one population per direction of the ping-pong, its flags on the device
    host = (T.PopulationRound(eng, models, out), T.PopulationRound(eng, out, models))
    host_flags = flagged.ended

    def leg_a(n):
        for r in range(n):
            flags = host_flags.cpu().numpy()  # the read-back of every round
            trunc, copies = [], []
            for d, nb in enumerate(lists):
                first = None if flags[d] else next((int(j) for j in nb if flags[j]), None)
                trunc.append([] if flags[d] or first is not None else nb)
                if first is not None:
                    copies.append((d, first))
            pr = host[r & 1]
            pr.set_topology(trunc, T.alphas_tf2, use_window=False)
            o = pr.run()
            for d, j in copies:
                o[d].copy_(pr.models[j])

    flags = [d in ended for d in range(D)]
    rows = 0  # rows a round of (b) / (c) reads and writes
    for d, nb in enumerate(lists):
        stops = flags[d] or any(flags[j] for j in nb)
        rows += 2 if stops else len(nb) + 2
    moved = rows * P * 4

    legs = {"p_plain_graph": lambda n: plain.rounds(n), "n_noflags_graph": lambda n: clear.rounds(n),
            "a_host_driven": leg_a, "b_ended_eager": lambda n: flagged.rounds(n, graph=False),
            "c_ended_graph": lambda n: flagged.rounds(n)}
    for fn in legs.values():  # warm-up: code objects, and the graphs of 1 and 8 periods
        fn(18)
    torch.cuda.synchronize()
    us = {k: [] for k in legs}
    for _ in range(PASSES):
        for k, fn in legs.items():
            us[k].append(_time(fn, R))
    med = {k: statistics.median(v) for k, v in us.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in us.items()}
    lines = []
    for k in legs:
        line = {"experiment": NAME, "shape": shape, "leg": k, "devices": D, "P": P, "K": K, "rounds": R,
                "ended": len(ended) if k[0] in "abc" else 0, "us_per_round": round(med[k], 3),
                "us_per_round_passes": [round(u, 3) for u in us[k]], "spread": round(spread[k], 4),
                "device": torch.cuda.get_device_name(0)}
        if k[0] in "bc":
            line.update(moved_bytes=moved, frac_of_8TBps=round(moved / (med[k] * 1e-6) / PEAK_BYTES_PER_S, 4))
        lines.append(line)
    p, n, a, b, c = (med[k] for k in legs)
    lines.append({"experiment": NAME, "shape": shape, "leg": "ratios",
                  "n_over_p": round(n / p, 3), "a_over_c": round(a / c, 2), "b_over_c": round(b / c, 2),
                  "p_spread": round(spread["p_plain_graph"], 4), "a_spread": round(spread["a_host_driven"], 4),
                  "n_within_p_spread": bool(n <= p * (1 + spread["p_plain_graph"])),
                  "b_not_slower_than_a": bool(b <= a * (1 + spread["a_host_driven"])),
                  "c_not_slower_than_b": bool(c <= b * (1 + spread["a_host_driven"])),
                  "frac_of_8TBps_c": lines[4]["frac_of_8TBps"]})
    return lines


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_ended_rounds.jsonl"))
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    args = ap.parse_args()
    import torch
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as fh:
        for shape in args.shapes:
            for line in run_shape(shape):
                fh.write(json.dumps(line) + "\n")
                fh.flush()
                print(json.dumps(line), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
