#!/usr/bin/env python3
"""The sliding ring round (cfa_mix_ring_slide_f32) on the bench's population (128 devices x 25M
fp32, K = 8 by default). The kernel reads its launch shape from the environment at every launch
(CFA_SLIDE_SEGMENTS, CFA_SLIDE_PF, CFA_SLIDE_WG_PER_CU, CFA_SLIDE_SC1, CFA_SLIDE_U, CFA_SLIDE_SEAM;
results identical), so one process compares shapes on the same stacks. One JSON line per record.

  ring_slide.py sweep            every shape, interleaved over passes: median us per round
  ring_slide.py ab [reps]        the slide round (shape from the environment) alternated with
                                 cfa_mix_ring_round_f32, `reps` (10) times each
  ring_slide.py once [launches]  only slide launches (for rocprofv3 --pmc runs, one counter per run)

Environment: RS_DEVICES, RS_P, RS_H (window half-width), RS_SEGMENTS / RS_PF / RS_WG / RS_SC1 /
RS_U / RS_SEAM (comma lists of the sweep; RS_U: float4 per lane and row, 1, 2 or 4; RS_SEAM: 1 the
seam kernel where the launch rule allows it, 0 the plain kernel), RS_PASSES."""
import itertools
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from federated_amd.engine import get_engine  # noqa: E402

NAME = "tools/probe/ring_slide.py"
D = int(os.environ.get("RS_DEVICES", "128"))
P = int(os.environ.get("RS_P", "25000000"))
H = int(os.environ.get("RS_H", "4"))
K = 2 * H
PEAK = 8.0e12  # MI355X HBM3E peak, bytes/s


def ints(name, default):
    return [int(x) for x in os.environ.get(name, default).split(",")]


def moved_bytes(segments, seam=0, u=4):
    s = min(segments, D)
    seg = -(-D // s)
    halo = 0 if seam and s == 1 and K and u in (2, 4) else -(-D // seg) * K  # slide_takes_seam
    return (2 * D + halo) * P * 4


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "sweep"
    eng = get_engine(0)
    models = torch.empty((D, P), dtype=torch.float32, device="cuda").normal_(
        generator=torch.Generator(device="cuda").manual_seed(5))
    out = torch.empty_like(models)
    alphas = torch.full((D,), 1.0 / (K + 1), dtype=torch.float32, device="cuda")

    def slide(shape=None):
        if shape is not None:
            for key, v in zip(("CFA_SLIDE_SEGMENTS", "CFA_SLIDE_PF", "CFA_SLIDE_WG_PER_CU", "CFA_SLIDE_SC1",
                               "CFA_SLIDE_U", "CFA_SLIDE_SEAM"), shape):
                os.environ[key] = str(v)
        eng.ring_slide(out, models, alphas, 0, D, H, H)

    def timed(fn, n=3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()  # warm
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n

    base = {"experiment": NAME, "mode": mode, "devices": D, "P": P, "hl": H, "hr": H}
    if mode == "once":
        for _ in range(int(sys.argv[2]) if len(sys.argv) > 2 else 5):
            slide()
        torch.cuda.synchronize()
        print(json.dumps(dict(base, segments=int(os.environ.get("CFA_SLIDE_SEGMENTS", "0")) or None)), flush=True)
    elif mode == "ab":
        reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
        ring = lambda: eng.ring_round(out, models, alphas, H, H)  # noqa: E731
        for rep in range(reps):
            for name, fn in (("ring_slide", slide), ("ring_round", ring)):
                print(json.dumps(dict(base, kernel=name, rep=rep, us_per_round=round(timed(fn), 2),
                                      slide_env={k: v for k, v in os.environ.items() if k.startswith("CFA_SLIDE_")})),
                      flush=True)
    else:
        shapes = list(itertools.product(ints("RS_SEGMENTS", "1"), ints("RS_PF", "1,2"),
                                        ints("RS_WG", "1,2,4"), ints("RS_SC1", "0"), ints("RS_U", "1,2,4"),
                                        ints("RS_SEAM", "0,1")))
        times = {s: [] for s in shapes}
        for _ in range(int(os.environ.get("RS_PASSES", "3"))):
            for s in shapes:
                times[s].append(timed(lambda: slide(s)))
        for s in sorted(shapes, key=lambda s: statistics.median(times[s])):
            us = statistics.median(times[s])
            mb = moved_bytes(s[0], s[5] and not s[3], s[4])
            print(json.dumps(dict(base, segments=s[0], pf=s[1], wg_per_cu=s[2], sc1=s[3], u=s[4], seam=s[5],
                                  us_per_round=round(us, 2), spread_us=round(max(times[s]) - min(times[s]), 2),
                                  moved_bytes=mb, moved_frac_of_peak=round(mb / (us * 1e-6) / PEAK, 4))), flush=True)


if __name__ == "__main__":
    main()
