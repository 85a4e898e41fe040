// cg_momentum.hpp -- momentum distribution n(k) of a walker batch from displaced wave-function ratios.  The reference has no counterpart
// (it reports the energy and entropy moments of src/VMC.py:44-53 only).  n(k) is the Fourier transform of the one-body density matrix:
// the first observable here that is off-diagonal in position, so it needs Psi at displaced configurations.
//
// Two kernels (cg_momentum_sums runs both; cg_displaced_ratios the first alone):
//   k_displaced_ratios (cg_k_sampler.inc)  per walker b and evaluation m = j n + i (j < S shifts per particle, i < n particles):
//             r_b(m) = Psi_K(x_b with row i moved by s_{b,m} L) / Psi_K(x_b) as (Re, Im), log Psi as cg_logpsi returns it, and
//             s_{b,m} in units of L (supplied, or Philox uniforms in [0, 1): cg_rng.hpp states the counter domain).
//   k_momentum (cg_hip.hip, the pieces below)  thread <-> k, k real in units of 2 pi / L:
//             n_k^(b) = (1/S) sum_{m < S n} e^{-2 pi i k.s_{b,m}} r_b(m),  summed in ascending m from +0, one sincos per term, the
//             factor 1/S applied once to the finished sum.  A term whose ratio is not finite (either component) adds nothing and is
//             counted in `dropped` (the same count for every k: it does not look at the phase).
//
// Packed result, W + 1 = 3 nK + 2 doubles, SUMS over the batch (cg_axpby accumulates over calls, one cg_allreduce_sum over ranks):
//   [0, 2 nK)      sum_b n_k^(b) as (re, im) pairs
//   [2 nK, 3 nK)   sum_b (Re n_k^(b))^2                   (the second moment behind the standard error over walkers)
//   [3 nK]         dropped terms
//   [3 nK + 1]     number of walkers B
//
// Reduction over the batch -- the rule of cg_structure.hpp, which fixes every bit of the result whatever grid was launched:
//   1. R = min(B, CG_STRUCT_ROWS = 1024) rows.  Row r sums its walkers r, r + R, r + 2R, ... in ascending order, starting from +0.
//   2. Column p of the result: group g = 0..CG_STRUCT_GROUPS-1 (16) sums the rows g, g + 16, g + 32, ... in ascending order, starting
//      from +0; the group sums are then added in ascending g, starting from group 0's (k_structure_reduce).
//   A row belongs to one workgroup at a time (a workgroup takes rows blockIdx.x, blockIdx.x + gridDim.x, ...), so the number of
//   workgroups does not enter (CG_MOMENTUM_GRID changes it).  No floating-point atomics; `dropped` is a sum of small integers held
//   exactly in doubles.
#pragma once
#include "cg_structure.hpp"

// width of one row of partial sums: [2 nK (re, im)] [nK re^2] [dropped]
static CG_HD int cg_momentum_width(int nK) { return 3 * nK + 1; }

// n_k^(b) of one walker for one k: ratios (M, 2), shifts (M, D) of that walker
template <int D>
CG_DEVI void cg_momentum_walker(const double* __restrict__ ratios, const double* __restrict__ shifts, int M, double invS,
                                const double (&k)[D], double& nre, double& nim) {
    double sr = 0.0, si = 0.0;
    for (int m = 0; m < M; ++m) {
        const double rr = ratios[2 * m], ri = ratios[2 * m + 1];
        if (!(isfinite(rr) && isfinite(ri))) continue;
        double t = 0.0;
#pragma unroll
        for (int a = 0; a < D; ++a) t += k[a] * shifts[m * D + a];
        double sn, cs; sincos(-2.0 * CG_PI * t, &sn, &cs);
        sr += cs * rr - sn * ri; si += cs * ri + sn * rr;
    }
    nre = sr * invS; nim = si * invS;
}
// the terms of one walker that k_momentum leaves out
CG_DEVI int cg_momentum_dropped(const double* __restrict__ ratios, int M) {
    int d = 0;
    for (int m = 0; m < M; ++m) d += (isfinite(ratios[2 * m]) && isfinite(ratios[2 * m + 1])) ? 0 : 1;
    return d;
}

// One row of partial sums for the k vector `kidx` (the thread's; kidx >= nK: nothing to do): walkers row, row + rows, ... in ascending
// order.  The thread with kidx == 0 also writes the row's dropped count.
template <int D>
CG_DEVI void cg_momentum_row(const double* __restrict__ ratios, const double* __restrict__ shifts, int B, int rows, int row, int M, double invS,
                             const double* __restrict__ K, int nK, int kidx, double* __restrict__ out_row) {
    if (kidx >= nK) return;
    double k[D];
#pragma unroll
    for (int a = 0; a < D; ++a) k[a] = K[(size_t)kidx * D + a];
    double are = 0.0, aim = 0.0, a2 = 0.0, drop = 0.0;
    for (int w = row; w < B; w += rows) {
        const double* rw = ratios + (size_t)w * M * 2;
        double nre, nim;
        cg_momentum_walker<D>(rw, shifts + (size_t)w * M * D, M, invS, k, nre, nim);
        are += nre; aim += nim; a2 += nre * nre;
        if (kidx == 0) drop += (double)cg_momentum_dropped(rw, M);
    }
    out_row[2 * kidx] = are; out_row[2 * kidx + 1] = aim; out_row[2 * nK + kidx] = a2;
    if (kidx == 0) out_row[3 * nK] = drop;
}
