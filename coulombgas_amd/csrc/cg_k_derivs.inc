// cg_k_derivs.inc -- grad / Laplacian (cg_lap.hpp) and theta-VJP / score (cg_derivs.hpp) kernels and their launches for ONE
// group of (dim, spsize, tpsize) instantiations.  Included by cg_k_derivs_a.hip / cg_k_derivs_b.hip with
//   CG_UNIT_CONFIGS(X) : the instantiations of this unit     CG_UNIT_NAME(f) : its function prefix
// Launch functions return 1 (launched), 0 (configuration not in this unit) or a negative error code.
int cg_big_scores(cg_ctx* c, const CgDev& m, const double* x, const int* sidx, int B, double* score);       // cg_k_big.hip
int cg_big_grad_lap(cg_ctx* c, const CgDev& m, const double* x, const int* sidx, int B, int mode, const double* v, double* grad, double* lap);
#ifndef CG_TH_STATIC_LDS
#define CG_TH_STATIC_LDS 0
#endif
#ifndef CG_LAP_LDS_BYTES
#define CG_LAP_LDS_BYTES (80 * 1024)
#endif

// grad / Laplacian of log Psi w.r.t. x (cg_lap.hpp): ONE walker per workgroup, no persistent loop -- around a loop over walkers
// the compiler hoists every loop-invariant address, offset and weight out of the body and spills them (972 B of scratch per lane,
// measured in round 2).  AL: every array of the kernel lives in LDS (the BASELINE size n = 13: 78 KB, two workgroups of 256 threads
// per CU, grid = batch).  Otherwise (NT = 512, one workgroup per CU): the blocks that do not fit the LDS budget use the HBM workspace
// slot of the workgroup, the batch is launched in chunks of `gridDim.x` walkers (w0 = first walker of the chunk).
template <int D, int HS, int HT, bool AL, int NT>
__global__ void __launch_bounds__(NT, NT <= 256 ? 2 : 1) k_grad_lap2(CgDev m, const double* __restrict__ theta, const double* __restrict__ spk, const double* __restrict__ tab, const double* __restrict__ x, const int* __restrict__ sidx, int B, int w0, int mode,
                           const double* __restrict__ v, double* __restrict__ grad, double* __restrict__ lap,
                           double* ws, typename CgLap<D, HS, HT>::Lay lay) {
    double* lds = cg_dyn_lds + CG_TAB_DOUBLES;
    const CgBlk b{(int)threadIdx.x, (int)blockDim.x};
    for (int e = threadIdx.x; e < CG_TAB_DOUBLES; e += blockDim.x) cg_dyn_lds[e] = tab[e];
    const int n = m.n, N = n * D;
    const double* th = theta;
    if (AL && CG_TH_STATIC_LDS) {        // (host: AL kernels are launched only with theta in LDS) a pointer the compiler KNOWS is LDS:
        double* th_l = lds + lay.th;     // ds_read instead of flat_load for every weight read of the sweeps -- measured 8 % SLOWER
        for (int e = b.tid; e < CgFast<D, HS, HT>::NPARAM; e += b.nthr) th_l[e] = theta[e];   // (flat loads overlap the ds_ queue)
        th = th_l;
    } else if (lay.th_lds) {             // per-lane weight reads from LDS instead of the vector L1
        double* th_l = lds + lay.th;
        for (int e = b.tid; e < CgFast<D, HS, HT>::NPARAM; e += b.nthr) th_l[e] = theta[e];
        th = th_l;
    }
    __syncthreads();
    CG_STAMP_INIT
    const int w = w0 + blockIdx.x;
    if (w < B)
        CgLap<D, HS, HT>::template grad_laplacian<AL>(b, th, x + (size_t)w * N, spk, sidx + (size_t)w * n, n, m.L, mode,
                                                      v ? v + (size_t)w * N : nullptr, grad + (size_t)w * N * 2, lap + 2 * w,
                                                      lds, AL ? ws : ws + (size_t)blockIdx.x * lay.ws_total, lay);
    CG_STAMP_FLUSH
}

// cg_grad_laplacian_probes at the sizes whose every array lives in LDS: k_grad_lap2<AL = true> with the probe loop around its jet pass
// (an instantiation of its own: k_grad_lap2 keeps its code).  v is (nprobe, B, n, dim): probe k of walker w at v + (k B + w) N.
template <int D, int HS, int HT>
__global__ void __launch_bounds__(256, 2) k_grad_lap2_probes(CgDev m, const double* __restrict__ theta, const double* __restrict__ spk, const double* __restrict__ tab, const double* __restrict__ x, const int* __restrict__ sidx, int B, int mode,
                           int nprobe, double weight, const double* __restrict__ v, double* __restrict__ grad, double* __restrict__ lap,
                           double* ws, typename CgLap<D, HS, HT>::Lay lay) {
    double* lds = cg_dyn_lds + CG_TAB_DOUBLES;
    const CgBlk b{(int)threadIdx.x, (int)blockDim.x};
    for (int e = threadIdx.x; e < CG_TAB_DOUBLES; e += blockDim.x) cg_dyn_lds[e] = tab[e];
    const int n = m.n, N = n * D;
    const double* th = theta;
    if (lay.th_lds) {                    // (always, on this path: the branch keeps the pointer generic, as in k_grad_lap2)
        double* th_l = lds + lay.th;
        for (int e = b.tid; e < CgFast<D, HS, HT>::NPARAM; e += b.nthr) th_l[e] = theta[e];
        th = th_l;
    }
    __syncthreads();
    CG_STAMP_INIT
    const int w = blockIdx.x;
    if (w < B)
        CgLap<D, HS, HT>::template grad_laplacian<true, true>(b, th, x + (size_t)w * N, spk, sidx + (size_t)w * n, n, m.L, mode, v + (size_t)w * N,
                                                              grad + (size_t)w * N * 2, lap + 2 * w, lds, ws, lay, nullptr, nullptr,
                                                              nprobe, (size_t)B * N, weight);
    CG_STAMP_FLUSH
}

// Per-sample scores, second generation (cg_score.hpp): one walker per workgroup, every array in LDS, the score row written as
// (re, im) pairs.  Launched for the systems whose layout fits the LDS budget (n <= 16); k_param_vjp below serves the others.
#ifndef CG_SCORE_LDS_BYTES
#define CG_SCORE_LDS_BYTES (80 * 1024)
#endif
template <int D, int HS, int HT>
__global__ void __launch_bounds__(256, 2) k_scores(CgDev m, const double* __restrict__ theta, const double* __restrict__ spk, const double* __restrict__ tab,
                         const double* __restrict__ x, const int* __restrict__ sidx, int B, double* __restrict__ score,
                         typename CgScore<D, HS, HT>::Lay lay) {
    double* lds = cg_dyn_lds + CG_TAB_DOUBLES;
    const CgBlk b{(int)threadIdx.x, (int)blockDim.x};
    for (int e = threadIdx.x; e < CG_TAB_DOUBLES; e += blockDim.x) cg_dyn_lds[e] = tab[e];
    constexpr int NP = CgFast<D, HS, HT>::NPARAM;
    double* th_l = lds + lay.th;
    for (int e = b.tid; e < NP; e += b.nthr) th_l[e] = theta[e];
    const double* th = lay.th >= 0 ? (const double*)th_l : theta;       // (a pointer the compiler treats as generic: flat loads overlap the ds_ queue)
    __syncthreads();
    CG_STAMP_INIT
    const int n = m.n, N = n * D, w = blockIdx.x;
    if (w < B) CgScore<D, HS, HT>::scores(b, th, x + (size_t)w * N, spk, sidx + (size_t)w * n, n, m.L, score + (size_t)w * NP * 2, lds, lay);
    CG_STAMP_FLUSH
}

// First-generation score kernel (cg_derivs.hpp), now the path of the systems that do not fit k_scores' LDS plan: ONE walker per
// workgroup (no persistent loop, see k_grad_lap2), the batch launched in chunks of gridDim.x walkers, each workgroup with its own HBM
// workspace slot; NT = 512 threads with the whole CU's LDS for the staged in-place inverses at large n.
// WPE: waves per SIMD the register allocation is sized for.  1: no constraint (190 VGPRs, nothing spilled, one 512-thread workgroup per CU).
// 4: 128 VGPRs (224 B of spill scratch per lane) so that TWO 512-thread workgroups share a CU: at N > 64 the kernel is a chain of exposed workspace
// latencies (35 cycles per VALU instruction, profiles/r04f_derivs_pmc_*), and the second workgroup fills them -- 2.45 -> 1.97 ms at n = 57, B = 512,
// 2.20 -> 1.55 ms at n = 49; at n = 29 (working set in L2) the spills cost more than the occupancy returns (2.82 -> 3.29 ms): WPE = 1 there.
template <int D, int HS, int HT, int NT, int WPE = 1>
__global__ void __launch_bounds__(NT, NT <= 256 ? 2 : WPE) k_param_vjp(CgDev m, const double* __restrict__ theta, const double* __restrict__ spk, const double* __restrict__ tab, const double* __restrict__ x, const int* __restrict__ sidx, int B, int w0,
                            double* __restrict__ score /* B x P x 2 */,
                            double* ws, size_t ws_per_walker, typename CgDerivs<D, HS, HT>::Layout lay) {
    double* lds = cg_dyn_lds + CG_TAB_DOUBLES;
    const CgBlk b{(int)threadIdx.x, (int)blockDim.x};
    for (int e = threadIdx.x; e < CG_TAB_DOUBLES; e += blockDim.x) cg_dyn_lds[e] = tab[e];
    __syncthreads();
    const int n = m.n, N = n * D;
    constexpr int P = CgFast<D, HS, HT>::NPARAM;
    const int w = w0 + blockIdx.x;
    if (w < B)
        CgDerivs<D, HS, HT>::param_vjp(b, theta, x + (size_t)w * N, spk, sidx + (size_t)w * n, n, m.L, 1.0, 0.0, nullptr,
                                       score + (size_t)w * P * 2, ws + (size_t)blockIdx.x * ws_per_walker, lds, lay);
}

typedef CG_CFG_LIST(CG_UNIT_CONFIGS) CgUnitConfigs;

int CG_UNIT_NAME(grad_lap)(cg_ctx* c, const CgDev& m, const double* x, const int* sidx, int B, int mode, const double* v,
                           double* grad, double* lap) {
    return cg_with_config<CgUnitConfigs>(c->dim, c->hs, c->ht, [&](auto cfg) -> int {
        constexpr int D = cfg.D, HS = cfg.HS, HT = cfg.HT;
        int rc;
        const int n = c->n;
        // everything in LDS at half a CU (two workgroups of 256 threads per CU = 2 waves per SIMD)?
        auto dl = CgLap<D, HS, HT>::layout(n, 256, mode, (size_t)CG_LAP_LDS_BYTES / sizeof(double) - CG_TAB_DOUBLES);
        if (dl.all_lds && dl.th_lds) {
            const size_t lds = sizeof(double) * (CG_TAB_DOUBLES + (size_t)dl.lds_total);
            if ((rc = ensure_ws(c, 64))) return rc;
            if ((rc = set_lds(c, k_grad_lap2<D, HS, HT, true, 256>, lds))) return rc;
            hipLaunchKernelGGL((k_grad_lap2<D, HS, HT, true, 256>), dim3(B), dim3(256), lds, c->stream, m, (const double*)c->d_theta, (const double*)c->d_spk,
                               (const double*)c->d_tab, x, sidx, B, 0, mode, v, grad, lap, (double*)c->ws, dl);
            return 1;
        }
        // larger systems, Hutchinson modes: the planned kernel (cg_k_big.hip)
        if (D == 2 && HS == 16 && HT == 16 && mode != 0 && (rc = cg_big_grad_lap(c, m, x, sidx, B, mode, v, grad, lap)) != 0) return rc;
        // larger systems (exact mode, other configurations): the first generation -- the rest in the workgroup's HBM workspace slot
        const int nt = cg_tune::lap_nt(n, D);
        dl = CgLap<D, HS, HT>::layout(n, nt, mode, (size_t)cg_tune::lap_lds_kb() * 1024 / sizeof(double) - CG_TAB_DOUBLES);
        const size_t lds = sizeof(double) * (CG_TAB_DOUBLES + (size_t)dl.lds_total);
        const int fit = (int)std::max<size_t>(1, (size_t)(160 * 1024) / (lds + 512));
        const int chunk = std::min(B, c->cu_count * cg_tune::lap_per_cu(fit));      // (a slot per walker and ONE launch measured no faster)
        return cg_with_nt_equal<256, 512>(nt, [&](auto ntc) -> int {
            constexpr int NT = ntc;
            return cg_launch_chunked(c, k_grad_lap2<D, HS, HT, false, NT>, lds, dl.ws_total, 8, chunk, B, [&](int grid, int w0) {
                hipLaunchKernelGGL((k_grad_lap2<D, HS, HT, false, NT>), dim3(grid), dim3(NT), lds, c->stream, m, (const double*)c->d_theta, (const double*)c->d_spk,
                                   (const double*)c->d_tab, x, sidx, B, w0, mode, v, grad, lap, (double*)c->ws, dl);
            });
        });
    });
}

// nprobe probes per walker behind one set-up (modes 1 and 2): 1 launched, 0 this unit has no probe-loop kernel for the configuration and
// size (the caller then combines single-probe launches), < 0 error.  Served: everything in LDS (any configuration of the unit), and the
// planned kernel of the (dim 2, 16, 16) flow at n > 16.
int cg_big_grad_lap_probes(cg_ctx* c, const CgDev& m, const double* x, const int* sidx, int B, int mode, int nprobe, const double* v, double weight,
                           double* grad, double* lap);      // cg_k_big.hip
int CG_UNIT_NAME(grad_lap_probes)(cg_ctx* c, const CgDev& m, const double* x, const int* sidx, int B, int mode, int nprobe, const double* v,
                                  double weight, double* grad, double* lap) {
    return cg_with_config<CgUnitConfigs>(c->dim, c->hs, c->ht, [&](auto cfg) -> int {
        constexpr int D = cfg.D, HS = cfg.HS, HT = cfg.HT;
        int rc;
        const auto dl = CgLap<D, HS, HT>::layout(c->n, 256, mode, (size_t)CG_LAP_LDS_BYTES / sizeof(double) - CG_TAB_DOUBLES);
        if (dl.all_lds && dl.th_lds) {
            const size_t lds = sizeof(double) * (CG_TAB_DOUBLES + (size_t)dl.lds_total);
            if ((rc = ensure_ws(c, 64))) return rc;
            if ((rc = set_lds(c, k_grad_lap2_probes<D, HS, HT>, lds))) return rc;
            hipLaunchKernelGGL((k_grad_lap2_probes<D, HS, HT>), dim3(B), dim3(256), lds, c->stream, m, (const double*)c->d_theta, (const double*)c->d_spk,
                               (const double*)c->d_tab, x, sidx, B, mode, nprobe, weight, v, grad, lap, (double*)c->ws, dl);
            return 1;
        }
        if (D == 2 && HS == 16 && HT == 16) return cg_big_grad_lap_probes(c, m, x, sidx, B, mode, nprobe, v, weight, grad, lap);
        return 0;
    });
}

// scores of B walkers into score (B x P x 2) by the first-generation kernel: 1 launched, 0 not this unit, < 0 error
int CG_UNIT_NAME(param_vjp)(cg_ctx* c, const CgDev& m, const double* x, const int* sidx, int B, double* score) {
    return cg_with_config<CgUnitConfigs>(c->dim, c->hs, c->ht, [&](auto cfg) -> int {
        constexpr int D = cfg.D, HS = cfg.HS, HT = cfg.HT;
        typedef CgDerivs<D, HS, HT> Dv;
        const int n = c->n;
        const size_t wsw = Dv::ws_doubles(n);
        auto dl = Dv::layout(n, 256);
        if (dl.vjp_fast) {      // small systems: the arena / the inverses fit a share of the CU's LDS: 256 threads, 2-3 workgroups per CU
            const size_t lds = sizeof(double) * (CG_TAB_DOUBLES + Dv::lds_doubles(n, 256) + Dv::vjp_lds_doubles(dl));
            const int chunk = std::min(B, c->cu_count * 2 * CG_DERIV_WAVES_OF(D));
            return cg_launch_chunked(c, k_param_vjp<D, HS, HT, 256>, lds, wsw, 0, chunk, B, [&](int grid, int w0) {
                hipLaunchKernelGGL((k_param_vjp<D, HS, HT, 256>), dim3(grid), dim3(256), lds, c->stream, m, (const double*)c->d_theta, (const double*)c->d_spk,
                                   (const double*)c->d_tab, x, sidx, B, w0, score, (double*)c->ws, wsw, dl);
            });
        }
        // larger systems: the inverses in place on an LDS copy where it fits, chunked launches
        const int nt = cg_tune::vjp_nt();
        dl = Dv::layout(n, nt, (size_t)cg_tune::vjp_lds_kb() * 1024);
        const size_t lds = sizeof(double) * (CG_TAB_DOUBLES + Dv::lds_doubles(n, nt) + Dv::vjp_lds_doubles(dl));
        const int fit = (int)std::max<size_t>(1, (size_t)(160 * 1024) / (lds + 512));
        const int per_cu = cg_tune::vjp_per_cu(fit);
        const int chunk = std::min(B, c->cu_count * per_cu);
        auto go = [&](auto ntc, auto wpec) -> int {
            constexpr int NT = ntc, WPE = wpec;
            return cg_launch_chunked(c, k_param_vjp<D, HS, HT, NT, WPE>, lds, wsw, 0, chunk, B, [&](int grid, int w0) {
                hipLaunchKernelGGL((k_param_vjp<D, HS, HT, NT, WPE>), dim3(grid), dim3(NT), lds, c->stream, m, (const double*)c->d_theta, (const double*)c->d_spk,
                                   (const double*)c->d_tab, x, sidx, B, w0, score, (double*)c->ws, wsw, dl);
            });
        };
        const bool occ = cg_tune::vjp_occ(n, D) != 0 && nt == 512 && per_cu >= 2;       // two workgroups per CU (128 VGPRs): 512 threads only
        return cg_with_nt_equal<256, 512>(nt, [&](auto ntc) -> int {
            if constexpr (ntc == 512) { if (occ) return go(ntc, std::integral_constant<int, 4>{}); }
            return go(ntc, std::integral_constant<int, 1>{});
        });
    });
}

// scores of B walkers into score (B x P x 2): 1 launched, 0 this unit / this size is served by k_param_vjp, < 0 error
int CG_UNIT_NAME(scores)(cg_ctx* c, const CgDev& m, const double* x, const int* sidx, int B, double* score) {
    return cg_with_config<CgUnitConfigs>(c->dim, c->hs, c->ht, [&](auto cfg) -> int {
        constexpr int D = cfg.D, HS = cfg.HS, HT = cfg.HT, nt = 256;
        if (!(HS == 16 && HT == 16)) return 0;
        const auto dl = CgScore<D, HS, HT>::layout(c->n, nt, (size_t)CG_SCORE_LDS_BYTES / sizeof(double) - CG_TAB_DOUBLES);
        if (!dl.ok) return D == 2 ? cg_big_scores(c, m, x, sidx, B, score) : 0;     // larger systems: the planned kernel (cg_k_big.hip)
        const size_t lds = sizeof(double) * (CG_TAB_DOUBLES + (size_t)dl.total);
        if (int rc = set_lds(c, k_scores<D, HS, HT>, lds)) return rc;
        hipLaunchKernelGGL((k_scores<D, HS, HT>), dim3(B), dim3(nt), lds, c->stream, m, (const double*)c->d_theta, (const double*)c->d_spk,
                           (const double*)c->d_tab, x, sidx, B, score, dl);
        return 1;
    });
}
