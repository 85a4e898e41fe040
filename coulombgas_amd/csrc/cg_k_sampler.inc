// cg_k_sampler.inc -- kernels of the depth-2 fast path (log Psi, fused Metropolis chain) and their launches for ONE group of
// (dim, spsize, tpsize) instantiations.  Included by cg_k_sampler_a.hip / cg_k_sampler_b.hip with
//   CG_UNIT_CONFIGS(X), CG_UNIT_SPECIALS(X) : the instantiations of this unit     CG_UNIT_NAME(f) : its function prefix
// Launch functions return 1 (launched), 0 (configuration not in this unit) or a negative error code.
// With CG_UNIT_DISPLACED defined the unit instantiates k_displaced_ratios alone (cg_k_displaced_a.hip / cg_k_displaced_b.hip: translation units
// of their own, so that the second family of chain-sized kernels compiles next to the first instead of after it); without it, k_logpsi and k_mcmc.
template <int D, int HS, int HT, int MAXT>
__global__ void __launch_bounds__(MAXT, (MAXT <= 256 ? CG_WAVES_PER_EU : 1)) k_logpsi(CgDev m, const double* __restrict__ theta, const double* __restrict__ spk, const double* __restrict__ tab, const double* __restrict__ x, const int* __restrict__ sidx, int B, int mode,
                         double* __restrict__ logphi, double* __restrict__ hld, double* __restrict__ logpsi_out,
                         double* __restrict__ logp_out, double* __restrict__ z_out, double* __restrict__ J_out) {
    using F = CgFast<D, HS, HT>;
    double* lds = cg_dyn_lds + CG_TAB_DOUBLES;
    const CgBlk b{(int)threadIdx.x, (int)blockDim.x};
    for (int e = threadIdx.x; e < CG_TAB_DOUBLES; e += blockDim.x) cg_dyn_lds[e] = tab[e];
    __syncthreads();
    const int n = m.n, N = n * D;
    double* xs = lds + m.lay.total;
    typename F::WFrag wfrag; const typename F::WFrag* wf = nullptr;
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (HS == 16 && HT == 16) { F::load_frags(theta, wfrag); wf = &wfrag; }
#endif
    for (int w = blockIdx.x; w < B; w += gridDim.x) {
        for (int e = b.tid; e < N; e += b.nthr) xs[e] = x[(size_t)w * N + e];
        b.sync();
        if (mode == CG_MODE_LOGPSI) {
            double re, im, h;
            F::logpsi(b, theta, xs, spk, sidx + (size_t)w * n, n, m.L, lds, m.lay, re, im, h, wf);
            if (b.tid == 0) {
                if (logphi) { logphi[2 * w] = re; logphi[2 * w + 1] = im; }
                if (hld) hld[w] = h;
                if (logpsi_out) { logpsi_out[2 * w] = re + h; logpsi_out[2 * w + 1] = im; }
                if (logp_out) logp_out[w] = 2.0 * (re + h);
            }
        } else {
            F::primal(b, theta, xs, n, m.L, lds, m.lay, wf);
            if (z_out)
                for (int e = b.tid; e < N; e += b.nthr) z_out[(size_t)w * N + e] = lds[m.lay.z + e];
            if (mode == CG_MODE_JAC) {
                F::jacobian(b, theta, n, m.L, lds, m.lay, wf);
                for (int e = b.tid; e < N * N; e += b.nthr) J_out[(size_t)w * N * N + e] = lds[m.lay.J + e];
            }
        }
        b.sync();
    }
}

// Batched Metropolis chain: src/MCMC.py:22-39.  One workgroup owns one walker for all mc_steps;
// x is read once and written once, the proposal/accept state never leaves the CU.
// NS > 0: specialised on n = NS and on a workgroup of exactly MAXT threads (CG_MCMC_SPECIALS).
template <int D, int HS, int HT, int MAXT, int NS = 0>
__global__ void __launch_bounds__(MAXT, (MAXT <= 256 ? CG_WAVES_PER_EU : 1)) k_mcmc(CgDev m, const double* __restrict__ theta, const double* __restrict__ spk, const double* __restrict__ tab, double* __restrict__ x, const int* __restrict__ sidx, int B, int steps, double stddev,
                       uint64_t seed, uint64_t walker_offset, const double* __restrict__ noise,
                       const double* __restrict__ unif, double* __restrict__ logp_out,
                       unsigned long long* __restrict__ n_accept) {
    using F = CgFast<D, HS, HT>;
    double* lds = cg_dyn_lds + CG_TAB_DOUBLES;
    const CgBlk b{(int)threadIdx.x, NS > 0 ? MAXT : (int)blockDim.x};
    for (int e = threadIdx.x; e < CG_TAB_DOUBLES; e += blockDim.x) cg_dyn_lds[e] = tab[e];
    __syncthreads();
    const int n = NS > 0 ? NS : m.n, N = n * D;
    CgFastLds lay_s = m.lay;
    if constexpr (NS > 0) lay_s = cg_fast_layout(NS, D, HS, HT, true, HS == 16 && HT == 16);   // folds to constants
    const CgFastLds& lay = lay_s;
    double* xc = lds + lay.total;          // current configuration
    double* xp = xc + ((N + 1) & ~1);        // proposal
    int* flag = (int*)(xp + ((N + 1) & ~1));
    double* kv = xp + ((N + 1) & ~1) + 2;    // the walker's n occupied plane waves k_j (constant along the chain: staged once per walker)
    CG_STAMP_INIT
    typename F::WFrag wfrag; const typename F::WFrag* wf = nullptr;
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (HS == 16 && HT == 16) {
        F::load_frags(theta, wfrag); wf = &wfrag;
        // small n: the weight slot of the LDS layout is not shared with anything -- staged once per workgroup, not per evaluation
        if (lay.wave_lu && !lay.dual) { F::stage_wt(b, theta, lds, lay); wfrag.wt_resident = true; }
    }
#endif
    for (int w = blockIdx.x; w < B; w += gridDim.x) {
        const int* si = sidx + (size_t)w * n;
        for (int e = b.tid; e < N; e += b.nthr) { xc[e] = x[(size_t)w * N + e]; kv[e] = spk[(size_t)si[e / D] * D + e % D]; }
        b.sync();
        double logp = 0.0;
        unsigned int nacc = 0;
        // step -1 evaluates logp of the initial configuration (src/MCMC.py:36) through the SAME call site as the
        // proposals, so that the (large, unrolled) log Psi code exists once in the instruction stream.
        for (int s = -1; s < steps; ++s) {
            CG_STAMP_START(0)
            for (int e = b.tid; e < N; e += b.nthr) {
                double g = 0.0;
                if (s >= 0) g = noise ? noise[((size_t)s * B + w) * N + e]
                                      : cg_philox_normal_ool(seed, walker_offset + w, (uint32_t)s, (uint32_t)e);
                xp[e] = xc[e] + stddev * g;
            }
            b.sync();
            CG_STAMP(0)
            double re, im, h;
#if defined(__HIP_DEVICE_COMPILE__) && !defined(CG_NO_OPAQUE_TID)
            // the lane id is made opaque once per evaluation: everything derived from it (LDS addresses, tile indices)
            // is then recomputed inside the evaluation instead of being hoisted out of the chain loop and spilled
            int tid_o = b.tid; asm volatile("" : "+v"(tid_o));
            const CgBlk be{tid_o, b.nthr};
#else
            const CgBlk& be = b;
#endif
            // (no index table: kv[j] is k_{sidx[j]}; specialised single-wave workgroups: the pair passes share their exponentials)
            F::template logpsi<F::pair_cache_ok(NS, MAXT) ? NS : 0>(be, theta, xp, kv, nullptr, n, m.L, lds, lay, re, im, h, wf);
            const double lp = 2.0 * (re + h);
            if (b.tid == 0) {
                int acc = 1;
                if (s >= 0) {
                    const double u = unif ? unif[(size_t)s * B + w] : cg_philox_uniform_ool(seed, walker_offset + w, (uint32_t)s);
                    const double d = lp - logp;             // ratio = e^d: >= 1 accepts whatever u in [0, 1) is; below, the table exponential
                    acc = (d >= 0.0 || (d > -745.0 && u < cg_exp_nonpos(d))) ? 1 : 0;      // NaN, e^d = 0 -> reject; +inf -> accept (src/MCMC.py:28-29)
                }
                *flag = acc;
            }
            b.sync();
            const int acc = *flag;
            if (acc) {
                for (int e = b.tid; e < N; e += b.nthr) xc[e] = xp[e];
                logp = lp;
                if (s >= 0) ++nacc;
            }
            b.sync();
            CG_STAMP_END(15)
        }
        for (int e = b.tid; e < N; e += b.nthr) x[(size_t)w * N + e] = xc[e];
        if (b.tid == 0) {
            if (logp_out) logp_out[w] = logp;
            if (n_accept && nacc) atomicAdd(n_accept, (unsigned long long)nacc);
        }
        b.sync();
    }
    CG_STAMP_FLUSH
}

// Displaced wave-function ratios for the momentum distribution (cg_momentum.hpp): Psi(x with row i moved by s L) / Psi(x) for M = S n
// single-particle displacements of every walker.  Built like k_mcmc -- one workgroup per walker, the same LDS image (configuration,
// trial configuration, staged plane waves, resident weight fragments; the flag slot stays unused), the same instantiations, and the
// log Psi code once in the instruction stream: evaluation -1 is the base configuration, evaluation m = j n + i moves particle i = m mod n
// by shifts[b, j, i, :] L (supplied), or by Philox uniforms in [0, 1) (cg_rng.hpp: the counter domain), which are then written to
// shifts_out as well.  Lane 0 writes ratios[b, m] = (Re, Im) = exp(dRe log Psi) (cos, sin)(dIm log Psi); a non-finite value is written as is.
template <int D, int HS, int HT, int MAXT, int NS = 0>
__global__ void __launch_bounds__(MAXT, (MAXT <= 256 ? CG_WAVES_PER_EU : 1)) k_displaced_ratios(CgDev m, const double* __restrict__ theta, const double* __restrict__ spk, const double* __restrict__ tab, const double* __restrict__ x, const int* __restrict__ sidx, int B, int M,
                       uint64_t seed, uint64_t walker_offset, const double* __restrict__ shifts,
                       double* __restrict__ shifts_out, double* __restrict__ ratios) {
    using F = CgFast<D, HS, HT>;
    double* lds = cg_dyn_lds + CG_TAB_DOUBLES;
    const CgBlk b{(int)threadIdx.x, NS > 0 ? MAXT : (int)blockDim.x};
    for (int e = threadIdx.x; e < CG_TAB_DOUBLES; e += blockDim.x) cg_dyn_lds[e] = tab[e];
    __syncthreads();
    const int n = NS > 0 ? NS : m.n, N = n * D;
    CgFastLds lay_s = m.lay;
    if constexpr (NS > 0) lay_s = cg_fast_layout(NS, D, HS, HT, true, HS == 16 && HT == 16);   // folds to constants
    const CgFastLds& lay = lay_s;
    double* xc = lds + lay.total;          // base configuration
    double* xp = xc + ((N + 1) & ~1);        // displaced configuration
    double* kv = xp + ((N + 1) & ~1) + 2;    // the walker's n occupied plane waves (the layout of k_mcmc: its flag slot lies in between)
    CG_STAMP_INIT
    typename F::WFrag wfrag; const typename F::WFrag* wf = nullptr;
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (HS == 16 && HT == 16) {
        F::load_frags(theta, wfrag); wf = &wfrag;
        if (lay.wave_lu && !lay.dual) { F::stage_wt(b, theta, lds, lay); wfrag.wt_resident = true; }
    }
#endif
    for (int w = blockIdx.x; w < B; w += gridDim.x) {
        const int* si = sidx + (size_t)w * n;
        for (int e = b.tid; e < N; e += b.nthr) { xc[e] = x[(size_t)w * N + e]; kv[e] = spk[(size_t)si[e / D] * D + e % D]; }
        b.sync();
        double base_re = 0.0, base_im = 0.0;
        int i0 = 0;                            // first coordinate of the particle that evaluation s moves: (s mod n) D
        // evaluation -1 is the base configuration, through the SAME call site as the displaced ones (see k_mcmc)
        for (int s = -1; s < M; ++s) {
            CG_STAMP_START(0)
            for (int e = b.tid; e < N; e += b.nthr) {
                double v = xc[e];
                const int a = e - i0;
                if (s >= 0 && a >= 0 && a < D) {
                    const size_t q = ((size_t)w * M + s) * D + a;
                    const double u = shifts ? shifts[q] : cg_philox_shift_ool(seed, walker_offset + w, (uint32_t)s, (uint32_t)a);
                    if (shifts_out) shifts_out[q] = u;
                    v += u * m.L;
                }
                xp[e] = v;
            }
            b.sync();
            CG_STAMP(0)
            double re, im, h;
#if defined(__HIP_DEVICE_COMPILE__) && !defined(CG_NO_OPAQUE_TID)
            int tid_o = b.tid; asm volatile("" : "+v"(tid_o));      // opaque lane id, once per evaluation (see k_mcmc)
            const CgBlk be{tid_o, b.nthr};
#else
            const CgBlk& be = b;
#endif
            F::template logpsi<F::pair_cache_ok(NS, MAXT) ? NS : 0>(be, theta, xp, kv, nullptr, n, m.L, lds, lay, re, im, h, wf);
            if (s < 0) { base_re = re + h; base_im = im; }
            else {
                if (b.tid == 0) {
                    const double mag = cg_exp_ool((re + h) - base_re);       // NaN / inf in -> NaN / inf out, as is
                    const CgSinCos sc = cg_sincos_ool(im - base_im);
                    ratios[((size_t)w * M + s) * 2] = mag * sc.c; ratios[((size_t)w * M + s) * 2 + 1] = mag * sc.s;
                }
                i0 += D; if (i0 >= N) i0 = 0;
            }
            b.sync();
            CG_STAMP_END(15)
        }
    }
    CG_STAMP_FLUSH
}


typedef CG_CFG_LIST(CG_UNIT_CONFIGS) CgUnitConfigs;
typedef CG_CFG_LIST(CG_UNIT_SPECIALS) CgUnitSpecials;

#if !defined(CG_UNIT_DISPLACED)
int CG_UNIT_NAME(logpsi)(cg_ctx* c, int nt, size_t lds, const CgDev& m, const double* x, const int* sidx, int B, int mode,
                         double* logphi, double* hld, double* logpsi_out, double* logp_out, double* z_out, double* J_out) {
    return cg_with_config<CgUnitConfigs>(c->dim, c->hs, c->ht, [&](auto cfg) -> int {
        return cg_with_nt_upto<256, 1024>(nt, [&](auto ntc) -> int {
            constexpr int D = cfg.D, HS = cfg.HS, HT = cfg.HT, MAXT = ntc;
            if (int rc = set_lds(c, k_logpsi<D, HS, HT, MAXT>, lds)) return rc;
            hipLaunchKernelGGL((k_logpsi<D, HS, HT, MAXT>), dim3(B), dim3(nt), lds, c->stream, m, (const double*)c->d_theta, (const double*)c->d_spk,
                               (const double*)c->d_tab, x, sidx, B, mode, logphi, hld, logpsi_out, logp_out, z_out, J_out);
            return 1;
        });
    });
}

int CG_UNIT_NAME(mcmc)(cg_ctx* c, int nt, size_t lds, const CgDev& m, double* x, const int* sidx, int B, int mc_steps, double mc_stddev,
                       uint64_t seed, uint64_t walker_offset, const double* noise, const double* unif, double* logp_out) {
    // MAXT: the bound the kernel is compiled for, NS: the particle number it is specialised on (0: any)
    auto launch = [&](auto cfg, auto maxt, auto ns) -> int {
        constexpr int D = cfg.D, HS = cfg.HS, HT = cfg.HT, MAXT = maxt, NS = ns;
        if (int rc = set_lds(c, k_mcmc<D, HS, HT, MAXT, NS>, lds)) return rc;
        hipLaunchKernelGGL((k_mcmc<D, HS, HT, MAXT, NS>), dim3(B), dim3(nt), lds, c->stream, m, (const double*)c->d_theta, (const double*)c->d_spk,
                           (const double*)c->d_tab, x, sidx, B, mc_steps, mc_stddev, seed, walker_offset, noise, unif, logp_out, c->d_accept);
        return 1;
    };
    if (int rc = cg_with_special<CgUnitSpecials>(c->dim, c->hs, c->ht, c->n, nt, [&](auto cfg) -> int {
            return launch(cfg, std::integral_constant<int, cfg.NT>{}, std::integral_constant<int, cfg.N>{});
        })) return rc;
    // (512 threads: an instantiation of its own, 256 registers per lane instead of the 128 of the 1024-thread one)
    return cg_with_config<CgUnitConfigs>(c->dim, c->hs, c->ht, [&](auto cfg) -> int {
        return cg_with_nt_upto<256, 512, 1024>(nt, [&](auto ntc) -> int { return launch(cfg, ntc, std::integral_constant<int, 0>{}); });
    });
}
#else
int CG_UNIT_NAME(displaced)(cg_ctx* c, int nt, size_t lds, const CgDev& m, const double* x, const int* sidx, int B, int M,
                            uint64_t seed, uint64_t walker_offset, const double* shifts, double* shifts_out, double* ratios) {
    // the instantiations of k_mcmc: (MAXT, NS) as there
    auto launch = [&](auto cfg, auto maxt, auto ns) -> int {
        constexpr int D = cfg.D, HS = cfg.HS, HT = cfg.HT, MAXT = maxt, NS = ns;
        if (int rc = set_lds(c, k_displaced_ratios<D, HS, HT, MAXT, NS>, lds)) return rc;
        hipLaunchKernelGGL((k_displaced_ratios<D, HS, HT, MAXT, NS>), dim3(B), dim3(nt), lds, c->stream, m, (const double*)c->d_theta, (const double*)c->d_spk,
                           (const double*)c->d_tab, x, sidx, B, M, seed, walker_offset, shifts, shifts_out, ratios);
        return 1;
    };
    if (int rc = cg_with_special<CgUnitSpecials>(c->dim, c->hs, c->ht, c->n, nt, [&](auto cfg) -> int {
            return launch(cfg, std::integral_constant<int, cfg.NT>{}, std::integral_constant<int, cfg.N>{});
        })) return rc;
    return cg_with_config<CgUnitConfigs>(c->dim, c->hs, c->ht, [&](auto cfg) -> int {
        return cg_with_nt_upto<256, 512, 1024>(nt, [&](auto ntc) -> int { return launch(cfg, ntc, std::integral_constant<int, 0>{}); });
    });
}
#endif
