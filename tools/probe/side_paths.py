#!/usr/bin/env python3
"""Launch times of the libcfa paths tools/kernel_rooflines.py does not reach: the TF1 population
round, the scalar kernels that take a whole bucket when it is misaligned (sequential mix, fp64 TF1
fold, both MEWMA forms) and the split reduction behind a split gradient launch.

HIP events around `--reps` back-to-back launches after warm-up, on device-resident buffers; one
JSON line per path. Set CFA_LIB to time another build of libcfa on the same script.
Usage: python tools/probe/side_paths.py [--reps 40]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps  # ms


def off1(P, dtype, n, scale=1.0):
    """n buckets of P elements that start one element past a 16-byte boundary."""
    return [(torch.randn(P + 4, device="cuda", dtype=dtype) * scale)[1:P + 1] for _ in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    args = ap.parse_args()
    from federated_amd import topology
    from federated_amd.engine import get_engine
    eng = get_engine(0)
    torch.manual_seed(7)
    rng = np.random.default_rng(7)

    def emit(kernel, case, fn):
        print(json.dumps({"kernel": kernel, "case": case, "reps": args.reps,
                          "avg_launch_ms": round(timed(fn, args.reps), 5)}), flush=True)

    # TF1 population round: 16 devices x 4 random neighbours, 6.25M elements each
    D, K, P = 16, 4, 6_250_000
    src = torch.randn(D, P, device="cuda")
    out = torch.empty(D, P, device="cuda")
    ptr, idx, coef = [0], [], []
    for d in range(D):
        nb = rng.choice([j for j in range(D) if j != d], K, replace=False)
        idx += [d] + [int(j) for j in nb]
        coef += [0.0] + [0.5 / (K + 1)] * K
        ptr.append(len(idx))
    tabs = (torch.tensor([out[d].data_ptr() for d in range(D)], dtype=torch.int64, device="cuda"),
            torch.tensor([src[d].data_ptr() for d in range(D)], dtype=torch.int64, device="cuda"),
            torch.tensor(ptr, dtype=torch.int32, device="cuda"), torch.tensor(idx, dtype=torch.int32, device="cuda"),
            torch.tensor(coef, dtype=torch.float64, device="cuda"))
    emit("population_tf1_kernel", f"{D} devices x {K} neighbours, P = {P}", lambda: eng.population_tf1(*tabs, D, P))
    del src, out

    # misaligned buckets: the scalar kernels take the whole bucket
    P, n = 4_000_000, 4
    a32 = off1(P, torch.float32, n + 1)
    out32 = torch.empty(P + 4, device="cuda")[2:P + 2]  # another misalignment than the inputs': all scalar
    emit("mix_scalar_kernel", f"cfa_mix_seq_f32, n = {n}, P = {P}, out and inputs misaligned differently",
         lambda: eng.mix_seq(out32, a32[0], a32[1:n + 1], [0.2] * n))
    a64 = off1(P, torch.float64, n + 1, 1e-3)
    out64 = torch.empty(P + 4, device="cuda", dtype=torch.float64)[1:P + 1]
    emit("mix_tf1_f64_kernel", f"cfa_mix_tf1_f64, n = {n}, P = {P}, buckets 8 bytes past a 16-byte boundary",
         lambda: eng.mix_tf1_f64(out64, a64[0], a64[1:], [0.1] * n, False))
    W, s0, s1, g0, g1 = off1(P, torch.float32, 5)
    emit("mewma_scalar_kernel", f"cfa_mewma_update_f32, n = 2, P = {P}, misaligned buckets",
         lambda: eng.mewma(W, [s0, s1], [g0, g1], 0.99, 0.01, 0.02, P // 2, False, True))
    Wd, t0, t1, h0, h1 = off1(P, torch.float64, 5, 1e-3)
    emit("mewma_tf1_f64_kernel", f"cfa_mewma_tf1_f64, n = 2, P = {P}, misaligned buckets",
         lambda: eng.mewma_tf1_f64(Wd, [t0, t1], [h0, h1], 0.99, 0.01, 0.02, P // 2, False, True))

    # split gradient launch (2NN, 32 evaluations of 24 samples): grad_2nn_kernel, then reduce_splits_kernel
    D, N, B, L, C, H = 16, 2, 24, 512, 8, 32
    P = L * H + H + H * C + C
    lists = topology.kregular_tf1(D, N)
    x = torch.randn(D, B, L, device="cuda")
    y = torch.eye(C, device="cuda")[torch.randint(0, C, (D, B), device="cuda")].contiguous()
    models = torch.randn(D, P, device="cuda") * 0.1
    mrow = torch.tensor([j for nbs in lists for j in nbs], dtype=torch.int32, device="cuda")
    drow = torch.tensor([i for i, nbs in enumerate(lists) for _ in nbs], dtype=torch.int32, device="cuda")
    M = mrow.numel()
    grads = torch.empty(M, P, device="cuda")
    ws = eng.grad_workspace(M, B, P)
    geom = {"intermediate_nodes": H}
    emit("reduce_splits_kernel", f"cfa_ge_grad_2nn_rows_f32 + reduction, M = {M}, B = {B}, P = {P}, "
         f"{eng.grad_splits(M, B, P)} splits", lambda: eng.grad_rows(2, x, y, models, mrow, drow, grads, geom, workspace=ws))


if __name__ == "__main__":
    main()
