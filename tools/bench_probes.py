#!/usr/bin/env python3
"""Timing: cg_grad_laplacian_probes with K probes next to K back-to-back cg_grad_laplacian calls on the same walkers, device-pointer mode,
HIP-event time (cg_timer_start / cg_timer_stop), mode 2 (Hutchinson-split).  The two are timed interleaved in one process -- rep by rep:
the K-probe call, then the K single calls --, median / min / max of 20 reps after 5 warm-ups, at (n, B) = (13, 8192), (29, 2048),
(57, 512) and K = 1, 2, 4, 8.  Also n = 29, B = 256: the 58 basis probes with weight 1 (the exact Laplacian) next to
cg_grad_laplacian(mode 0) on the same walkers.  One JSON line.
   python tools/bench_probes.py [--reps 20] [--warmup 5] [--sizes 13x8192,29x2048,57x512] [--K 1,2,4,8] [--exact 29x256]
   rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_probes.py      (k_gradlap_big_probes / k_grad_lap2_probes)"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from coulombgas_amd.engine import Engine, DeviceArray
from coulombgas_amd.synthetic import bench_inputs

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--sizes", default="13x8192,29x2048,57x512")
ap.add_argument("--K", default="1,2,4,8")
ap.add_argument("--exact", default="29x256")
args = ap.parse_args()
Ks = [int(k) for k in args.K.split(",")]


def stats(ts):
    return {"median": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts))}


def make(n, B):
    L, sp, theta, sidx, x = bench_inputs(n, 2, B, 25 if n <= 29 else 36 if n <= 49 else 49, 0)
    eng = Engine(n, 2, 2, 16, 16, L, sp)
    eng.set_params(theta)
    return eng, DeviceArray.from_numpy(eng, x), DeviceArray.from_numpy(eng, sidx, np.int32)


def interleaved(eng, fa, fb):
    """fa, fb timed alternately, rep by rep"""
    for _ in range(args.warmup):
        fa(); fb()
    eng.sync()
    ta, tb = [], []
    for _ in range(args.reps):
        eng.timer_start(); fa(); ta.append(eng.timer_stop())
        eng.timer_start(); fb(); tb.append(eng.timer_stop())
    return stats(ta), stats(tb)


out = {"mode": 2, "reps": args.reps, "warmup": args.warmup, "sizes": []}
for size in args.sizes.split(","):
    n, B = (int(v) for v in size.split("x"))
    eng, x, s = make(n, B)
    vall = eng.randn_d("bench_probes", (max(Ks), B, n, 2), 1)
    rows = []
    for K in Ks:
        vK = eng.view(vall, 0, (K, B, n, 2))
        vk = [eng.view(vall, k * B * n * 2, (B, n, 2)) for k in range(K)]

        def single_calls():
            for v in vk:
                eng.grad_laplacian_d(x, s, 2, v)

        tp, ts = interleaved(eng, lambda: eng.grad_laplacian_probes_d(x, s, 2, vK), single_calls)
        rows.append({"K": K, "probes_ms": tp, "K_single_calls_ms": ts, "ratio_of_medians": tp["median"] / ts["median"],
                     "ranges_overlap": not (tp["max"] < ts["min"] or ts["max"] < tp["min"])})
    t1 = rows[0]["probes_ms"]["median"] if Ks[0] == 1 else None
    for r in rows:
        r["t_K_over_t_1"] = r["probes_ms"]["median"] / t1 if t1 else None
    out["sizes"].append({"n": n, "B": B, "rows": rows})
    eng.close()

if args.exact:
    n, B = (int(v) for v in args.exact.split("x"))
    eng, x, s = make(n, B)
    N = n * 2
    basis = DeviceArray.from_numpy(eng, np.ascontiguousarray(np.broadcast_to(np.eye(N).reshape(N, 1, n, 2), (N, B, n, 2))))
    tp, te = interleaved(eng, lambda: eng.grad_laplacian_probes_d(x, s, 2, basis, weight=1.0), lambda: eng.grad_laplacian_d(x, s, 0))
    lp = np.asarray(eng.grad_laplacian_probes_d(x, s, 2, basis, weight=1.0)[1]).copy()
    le = np.asarray(eng.grad_laplacian_d(x, s, 0)[1]).copy()
    out["basis_probes"] = {"n": n, "B": B, "nprobe": N, "probes_ms": tp, "exact_mode_ms": te, "ratio_of_medians": tp["median"] / te["median"],
                           "max_rel_lap_diff": float((np.abs(lp - le) / np.maximum(1.0, np.abs(le))).max())}
    eng.close()
print(json.dumps(out), flush=True)
