#!/usr/bin/env python3
"""Timing: cg_structure_sums next to cg_ewald with the same k table on the same walkers, device-pointer mode, HIP-event time per call
(cg_timer_start / cg_timer_stop): median of 20 calls after 5 warm-ups, at (n, B) = (13, 8192) and (57, 512), K = kpoints(2, 15),
128 bins.  One JSON line per size.
   python tools/bench_structure.py [--reps 20] [--warmup 5]
   rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_structure.py      (k_structure / k_structure_reduce / k_ewald)"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import coulombgas_amd as cg
from coulombgas_amd.engine import Engine, DeviceArray
from coulombgas_amd.synthetic import box_length

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--sizes", default="13x8192,57x512")
args = ap.parse_args()

K = cg.kpoints(2, 15)
for size in args.sizes.split(","):
    n, B = (int(v) for v in size.split("x"))
    L = box_length(n, 2)
    eng = Engine(n, 2, 2, 16, 16, L)
    eng.set_ewald(10.0, K, 10.0)
    eng.set_structure(K, 128, 0.5)
    x = DeviceArray.from_numpy(eng, np.random.default_rng(0).uniform(0.0, L, (B, n, 2)))

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        eng.sync()
        ts = []
        for _ in range(args.reps):
            eng.timer_start(); fn(); ts.append(eng.timer_stop())
        return float(np.median(ts)), float(min(ts)), float(max(ts))

    ts, te = timed(lambda: eng.structure_sums_d(x)), timed(lambda: eng.ewald_d(x))
    out = np.asarray(eng.structure_sums_d(x))
    print(json.dumps({"n": n, "B": B, "nK": int(K.shape[0]), "nbins": 128, "structure_ms": {"median": ts[0], "min": ts[1], "max": ts[2]},
                      "ewald_ms": {"median": te[0], "min": te[1], "max": te[2]}, "ratio_of_medians": ts[0] / te[0],
                      "pairs_conserved": bool(out[3 * K.shape[0]:-1].sum() == B * n * (n - 1) // 2), "reps": args.reps, "warmup": args.warmup}),
          flush=True)
    eng.close()
