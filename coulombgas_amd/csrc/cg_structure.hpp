// cg_structure.hpp -- structure observables of a walker batch: the density modes rho_k = sum_i exp(2 pi i k.x_i / L) behind the static
// structure factor S(k) = <|rho_k|^2> / n, and the radial pair histogram behind g(r).  The reference has no counterpart (it reports the
// energy and entropy moments of src/VMC.py:44-53 only); the conventions are those of its Ewald sum (src/potential.py:47-48).
//
// Per walker (the pieces below; the kernels that call them are in cg_hip.hip):
//   rho_k     from per-particle power tables e^{2 pi i m x/L}, m = 0..Kmax, held in LDS exactly as in cg_ewald.hpp (one sincos per
//             coordinate, no transcendental per (particle, k)); thread <-> k, CG_STRUCT_KPT vectors per thread and launch slice, the sums
//             of |rho_k|^2, Re rho_k, Im rho_k over the walkers of a row stay in that thread's registers.
//   histogram every pair i < j: r~ = (x_i - x_j)/L - rint(.) (nearest image, cg_ewald.hpp:39-41), d = |r~|, t = d * (nbins / rmax),
//             bin (int)t if t < nbins, else the overflow bin nbins.  The test is written !(t < nbins): a pair with a non-finite
//             distance lands in the overflow bin and the pair count is conserved.  Integer counters in LDS.
//
// Reduction over the batch -- the rule that fixes every bit of the result (two calls on the same input agree bit for bit, whatever
// grid was launched):
//   1. R = min(B, CG_STRUCT_ROWS) rows.  Row r sums its walkers r, r + R, r + 2R, ... in ascending order, starting from +0.
//   2. Column p of the result: group g = 0..CG_STRUCT_GROUPS-1 sums the rows g, g + GROUPS, g + 2 GROUPS, ... in ascending order,
//      starting from +0; the group sums are then added in ascending g, starting from group 0's.
//   A row belongs to one workgroup at a time (a workgroup takes rows blockIdx.x, blockIdx.x + gridDim.x, ...), so the number of
//   workgroups does not enter.  Splitting a batch over two calls and adding the results regroups the walkers into other rows: the
//   histogram (integers, exact in doubles up to 2^53) is unchanged, the rho sums differ by ordinary reassociation error.
//   No floating-point atomics anywhere; the histogram's LDS atomics are integer adds (order-independent).
//
// LDS of one workgroup: [n D padded to even: the walker] [n D (Kmax+1) 2: tables] doubles, then [nbins + 1] 32-bit counters;
// no reduction scratch (the per-k sums never leave their thread).  cg_structure_lds_bytes() is what cg_set_structure checks.
#pragma once
#include "cg_common.hpp"

#define CG_STRUCT_ROWS 1024
#define CG_STRUCT_GROUPS 16
#define CG_STRUCT_KPT 4

static CG_HD int cg_structure_rows(int B) { return B < CG_STRUCT_ROWS ? B : CG_STRUCT_ROWS; }
static CG_HD size_t cg_structure_lds_bytes(int n, int D, int Kmax, int nbins) {
    const size_t N = (size_t)n * D;
    return sizeof(double) * (((N + 1) & ~(size_t)1) + N * (size_t)(Kmax + 1) * 2) + ((sizeof(unsigned) * ((size_t)nbins + 1) + 7) & ~(size_t)7);
}

// tab[(e T + m) 2 + {0,1}] = e^{2 pi i m x_e / L}, e = particle * D + axis, T = Kmax + 1 (the table of cg_ewald_walker)
template <int D>
CG_DEVI void cg_structure_tables(const CgBlk& b, const double* x, int n, double L, int T, double* tab) {
    for (int e = b.tid; e < n * D; e += b.nthr) {
        double s, c; sincos(x[e] * (2.0 * CG_PI / L), &s, &c);
        double* t = tab + (size_t)e * T * 2;
        double pr = 1.0, pi = 0.0;
        t[0] = 1.0; t[1] = 0.0;
        for (int m = 1; m < T; ++m) {
            const double nr = pr * c - pi * s, ni = pr * s + pi * c;
            pr = nr; pi = ni; t[2 * m] = pr; t[2 * m + 1] = pi;
        }
    }
}

// rho_k of the walker whose tables are in tab, for the integer vector kv
template <int D>
CG_DEVI void cg_structure_rho(const double* tab, int n, int T, const int (&kv)[D], double& sr, double& si) {
    sr = 0.0; si = 0.0;
    for (int i = 0; i < n; ++i) {
        double pr = 1.0, pi = 0.0;
#pragma unroll
        for (int a = 0; a < D; ++a) {
            const int m = kv[a] < 0 ? -kv[a] : kv[a];
            const double* t = tab + ((size_t)(i * D + a) * T + m) * 2;
            const double tr = t[0], ti = kv[a] < 0 ? -t[1] : t[1];
            const double nr = pr * tr - pi * ti, ni = pr * ti + pi * tr;
            pr = nr; pi = ni;
        }
        sr += pr; si += pi;
    }
}

// this thread's vectors of the launch slice that starts at k0: k = k0 + j nthr + tid, j < CG_STRUCT_KPT
struct CgStructAcc {
    double s2[CG_STRUCT_KPT], re[CG_STRUCT_KPT], im[CG_STRUCT_KPT];
    CG_DEVI void zero() {
#pragma unroll
        for (int j = 0; j < CG_STRUCT_KPT; ++j) s2[j] = re[j] = im[j] = 0.0;
    }
};
template <int D>
CG_DEVI void cg_structure_load_k(const CgBlk& b, const int* __restrict__ K, int k0, int nK, int (&kv)[CG_STRUCT_KPT][D]) {
#pragma unroll
    for (int j = 0; j < CG_STRUCT_KPT; ++j) {
        const int k = k0 + j * b.nthr + b.tid;
#pragma unroll
        for (int a = 0; a < D; ++a) kv[j][a] = k < nK ? K[(size_t)k * D + a] : 0;
    }
}
template <int D>
CG_DEVI void cg_structure_add_walker(const CgBlk& b, const double* tab, int n, int T, int k0, int nK, const int (&kv)[CG_STRUCT_KPT][D],
                                     CgStructAcc& acc) {
#pragma unroll
    for (int j = 0; j < CG_STRUCT_KPT; ++j) {
        if (k0 + j * b.nthr + b.tid >= nK) continue;
        double sr, si;
        cg_structure_rho<D>(tab, n, T, kv[j], sr, si);
        acc.s2[j] += sr * sr + si * si; acc.re[j] += sr; acc.im[j] += si;
    }
}
// one row of partial sums: [nK: |rho|^2] [2 nK: (re, im)] [nbins + 1: counts]
CG_DEVI void cg_structure_store_k(const CgBlk& b, int k0, int nK, const CgStructAcc& acc, double* __restrict__ row) {
#pragma unroll
    for (int j = 0; j < CG_STRUCT_KPT; ++j) {
        const int k = k0 + j * b.nthr + b.tid;
        if (k >= nK) continue;
        row[k] = acc.s2[j]; row[nK + 2 * k] = acc.re[j]; row[nK + 2 * k + 1] = acc.im[j];
    }
}

CG_DEVI void cg_structure_count(unsigned* slot) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(slot, 1u);            // LDS integer add
#else
    ++*slot;
#endif
}
// scale = nbins / rmax; hist: nbins + 1 counters (the last one: overflow)
template <int D>
CG_DEVI void cg_structure_pairs(const CgBlk& b, const double* x, int n, double L, int nbins, double scale, unsigned* hist) {
    const double rL = 1.0 / L, nb = (double)nbins;
    for (int e = b.tid; e < n * n; e += b.nthr) {
        const int i = e / n, j = e - i * n;
        if (j <= i) continue;
        double d2 = 0.0;
#pragma unroll
        for (int a = 0; a < D; ++a) {
            double r = (x[i * D + a] - x[j * D + a]) * rL;
            r -= rint(r);
            d2 += r * r;
        }
        const double t = sqrt(d2) * scale;
        const int bin = !(t < nb) ? nbins : (int)t;
        cg_structure_count(hist + bin);
    }
}
// the counters of a finished row go out as doubles and start the next row at zero (each counter by one thread: no barrier in between)
CG_DEVI void cg_structure_store_hist(const CgBlk& b, int nbins, unsigned* hist, double* __restrict__ row_hist) {
    for (int e = b.tid; e <= nbins; e += b.nthr) { row_hist[e] = (double)hist[e]; hist[e] = 0u; }
}

// step 2 of the rule above, one group of one column
CG_DEVI double cg_structure_group_sum(const double* __restrict__ partial, int rows, int W, int p, int g) {
    double a = 0.0;
    for (int r = g; r < rows; r += CG_STRUCT_GROUPS) a += partial[(size_t)r * W + p];
    return a;
}
