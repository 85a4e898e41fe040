#!/usr/bin/env python3
"""Timing: cg_displaced_ratios (M = S n log Psi evaluations per walker) next to cg_mcmc with mc_steps = M on the same walkers and
parameters -- the same number of evaluations through the same log Psi code -- and cg_momentum_sums (K = the orbital table) next to
them.  Device-pointer mode, HIP-event time per call (cg_timer_start / cg_timer_stop): median of 20 calls after 5 warm-ups, min - max
reported, at (n, B, S) = (13, 8192, 4) and (57, 512, 1).  The chain runs on a copy of the walkers, so every timed call of the ratio
kernel sees the same input.  One JSON line per size.
   python tools/bench_momentum.py [--reps 20] [--warmup 5] [--sizes 13x8192x4,57x512x1]
   rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_momentum.py      (k_displaced_ratios / k_mcmc / k_momentum)"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from coulombgas_amd.engine import Engine, DeviceArray
from coulombgas_amd.synthetic import bench_inputs

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--sizes", default="13x8192x4,57x512x1")
args = ap.parse_args()

for size in args.sizes.split(","):
    n, B, S = (int(v) for v in size.split("x"))
    L, sp, theta, sidx, x = bench_inputs(n, 2, B, 25 if n <= 29 else 49, 0)
    eng = Engine(n, 2, 2, 16, 16, L, sp)
    eng.set_params(theta)
    eng.set_momentum(sp)
    M = S * n
    x_d, s_d = DeviceArray.from_numpy(eng, x), DeviceArray.from_numpy(eng, sidx, np.int32)
    xc_d = DeviceArray.from_numpy(eng, x)
    eng.mcmc_d(xc_d, s_d, 50, 0.1, seed=1, count=False)         # the chain's walkers: thermalised a little, as in a run

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        eng.sync()
        ts = []
        for _ in range(args.reps):
            eng.timer_start(); fn(); ts.append(eng.timer_stop())
        return {"median": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts))}

    eng.axpby_d(1.0, xc_d, 0.0, x_d)                            # both kernels start from the same thermalised walkers
    t_ratio = timed(lambda: eng.displaced_ratios_d(x_d, s_d, S, seed=3))
    t_sums = timed(lambda: eng.momentum_sums_d(x_d, s_d, S, seed=3))
    t_mcmc = timed(lambda: eng.mcmc_d(xc_d, s_d, M, 0.1, seed=3, count=False))
    out = np.asarray(eng.momentum_sums_d(x_d, s_d, S, seed=3))
    nK = sp.shape[0]
    print(json.dumps({"n": n, "B": B, "S": S, "evaluations_per_walker": M, "nK": int(nK), "displaced_ratios_ms": t_ratio, "momentum_sums_ms": t_sums,
                      "mcmc_ms": t_mcmc, "ratio_displaced_over_mcmc": t_ratio["median"] / t_mcmc["median"],
                      "ratio_sums_over_mcmc": t_sums["median"] / t_mcmc["median"], "sum_k_n_k": float(out[0:2 * nK:2].sum() / B),
                      "dropped": float(out[3 * nK]), "reps": args.reps, "warmup": args.warmup}), flush=True)
    eng.close()
