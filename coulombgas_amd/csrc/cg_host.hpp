// cg_host.hpp -- host-side state and launch helpers shared by the translation units of libcoulombgas_hip.so (build.py: HIP_UNITS; the
// library is split so that the units compile in parallel).
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include <vector>
#include <algorithm>
#include <cstring>
#include <cstdio>
#include <cstdlib>
#include <cmath>

#include "../../include/coulombgas.h"
#include "cg_common.hpp"
#include "cg_linalg.hpp"
#include "cg_flow_fast.hpp"
#include "cg_dispatch.hpp"
#include "cg_generic.hpp"
#include "cg_van.hpp"

// ------------------------------------------------------------------------------------------
// device-side model descriptor (passed by value to every kernel)
// ------------------------------------------------------------------------------------------
struct CgDev {
    int n;
    double L;
    CgFastLds lay;
};

// minimum waves per SIMD the sampler kernels are register-allocated for (2 -> <= 256 VGPRs, 4 -> <= 128)
#ifndef CG_WAVES_PER_EU
#define CG_WAVES_PER_EU 2
#endif

enum { CG_MODE_LOGPSI = 0, CG_MODE_FLOW = 1, CG_MODE_JAC = 2 };

// minimum waves per SIMD the derivative kernels are register-allocated for
#ifndef CG_DERIV_WAVES
#define CG_DERIV_WAVES 3
#endif
#define CG_DERIV_WAVES_OF(D) ((D) == 2 ? CG_DERIV_WAVES : (CG_DERIV_WAVES < 2 ? CG_DERIV_WAVES : 2))

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
extern thread_local std::string g_last_error;      // defined in cg_hip.hip

struct Chunk { void* p; size_t cap; };

struct cg_ctx {
    int device = 0, n = 0, dim = 0, depth = 0, hs = 0, ht = 0, M = 0, P = 0;
    double L = 0;
    bool fast = false;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    void* bounce = nullptr; size_t bounce_cap = 0;     // pinned staging buffer for large device-to-host results
    double* d_theta = nullptr;
    double* d_spk = nullptr;
    double* d_tab = nullptr;     // exp / log tables of cg_common.hpp
    bool have_theta = false;
    // ewald
    bool have_ewald = false;
    double kappa = 0, rs = 0, g0 = 0;
    int nG = 0, Gmax = 0;
    int* d_G = nullptr;
    double* d_gk = nullptr;
    // structure observables (cg_set_structure)
    bool have_structure = false;
    int nK = 0, Kmax = 0, nbins = 0;
    double rmax = 0;
    int* d_K = nullptr;
    // momentum distribution (cg_set_momentum): real k vectors in units of 2 pi / L
    bool have_momentum = false;
    int nKm = 0;
    double* d_Km = nullptr;
    int ptr_mode = CG_PTR_HOST;
    int block_threads = 0;
    int cu_count = 256;
    CgFastLds lay;
    CgGenModel gm;               // general-depth path (fast == false)
    CgGenWs gw;
    CgGenWs gwv;      // the same + the reverse-pass arena of the theta-VJP
    unsigned long long* d_accept = nullptr;
    double* d_rate = nullptr;             // device scalar of cg_mcmc_accept_rate
    // staging arena for host-pointer mode + internal workspaces
    std::vector<Chunk> chunks;
    size_t cur = 0, off = 0;
    // persistent workspace (derivative kernels)
    void* ws = nullptr; size_t ws_cap = 0;
    double* d_scores = nullptr; size_t scores_cap = 0; int scores_B = 0;     // resident per-sample scores (cg_scores_*)
    void* d_lay = nullptr; int lay_tag = 0;     // small device copy of a kernel's layout struct (k_grad_lap2_scores: read where used instead of
                                                // living in scalar registers through the whole kernel); lay_tag says whose
    CgVanModel van; double* d_van = nullptr; double* d_van_sp = nullptr; bool have_van = false;   // density-matrix Transformer (cg_van_*)
    double* d_van_scores = nullptr; size_t van_scores_cap = 0; int van_scores_B = 0;              // resident classical scores
    std::string err;
    hipStream_t stream2 = nullptr;                     // look-ahead stream of the blocked Cholesky (bulk trailing updates)
    hipEvent_t ev_a = nullptr, ev_b = nullptr;
};

#define CG_FAIL(ctx, code, ...)                                         \
    do {                                                                \
        char _b[512]; snprintf(_b, sizeof(_b), __VA_ARGS__);            \
        if (ctx) (ctx)->err = _b;                                       \
        g_last_error = _b;                                              \
        return (code);                                                  \
    } while (0)

#define CG_HIP(ctx, call)                                                                         \
    do {                                                                                          \
        hipError_t _e = (call);                                                                   \
        if (_e != hipSuccess) CG_FAIL(ctx, CG_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

static int arena_reset(cg_ctx* c) {
    if (c->chunks.size() > 1) {
        size_t tot = 0;
        for (auto& ch : c->chunks) { tot += ch.cap; (void)hipFree(ch.p); }
        c->chunks.clear();
        void* p = nullptr;
        if (hipMalloc(&p, tot) != hipSuccess) return CG_ERR_HIP;
        c->chunks.push_back({p, tot});
    }
    c->cur = 0; c->off = 0;
    return CG_OK;
}
static void* arena_take(cg_ctx* c, size_t bytes) {
    bytes = (bytes + 255) & ~(size_t)255;
    if (bytes == 0) bytes = 256;
    while (c->cur < c->chunks.size()) {
        if (c->off + bytes <= c->chunks[c->cur].cap) { void* p = (char*)c->chunks[c->cur].p + c->off; c->off += bytes; return p; }
        ++c->cur; c->off = 0;
    }
    size_t cap = std::max(bytes, (size_t)(c->chunks.empty() ? (1u << 20) : 2 * c->chunks.back().cap));
    void* p = nullptr;
    if (hipMalloc(&p, cap) != hipSuccess) return nullptr;
    c->chunks.push_back({p, cap});
    c->cur = c->chunks.size() - 1; c->off = bytes;
    return p;
}

// An argument that is an input and/or output array in either pointer mode.
struct Arg {
    void* user; void* dev; size_t bytes; bool in, out;
};
static int stage(cg_ctx* c, Arg& a) {
    if (!a.user) { a.dev = nullptr; return CG_OK; }
    if (c->ptr_mode == CG_PTR_DEVICE) { a.dev = a.user; return CG_OK; }
    a.dev = arena_take(c, a.bytes);
    if (!a.dev) CG_FAIL(c, CG_ERR_HIP, "device staging allocation of %zu bytes failed", a.bytes);
    if (a.in) CG_HIP(c, hipMemcpyAsync(a.dev, a.user, a.bytes, hipMemcpyHostToDevice, c->stream));
    return CG_OK;
}
static int unstage(cg_ctx* c, Arg& a) {
    if (!a.user || c->ptr_mode == CG_PTR_DEVICE || !a.out) return CG_OK;
    if (a.bytes >= ((size_t)1 << 20)) {
        // Large results (Fisher matrices, score blocks) go through a pinned buffer: a device-to-host copy into pageable
        // memory ran at ~1 GB/s on part of the pool (9 MB Fisher matrix: 10 ms), DMA into pinned memory + memcpy does not.
        if (c->bounce_cap < a.bytes) {
            if (c->bounce) { (void)hipHostFree(c->bounce); c->bounce = nullptr; c->bounce_cap = 0; }
            if (hipHostMalloc(&c->bounce, a.bytes, hipHostMallocDefault) == hipSuccess) c->bounce_cap = a.bytes;
            else { c->bounce = nullptr; (void)hipGetLastError(); }
        }
        if (c->bounce) {
            CG_HIP(c, hipMemcpyAsync(c->bounce, a.dev, a.bytes, hipMemcpyDeviceToHost, c->stream));
            CG_HIP(c, hipStreamSynchronize(c->stream));
            memcpy(a.user, c->bounce, a.bytes);
            return CG_OK;
        }
    }
    CG_HIP(c, hipMemcpyAsync(a.user, a.dev, a.bytes, hipMemcpyDeviceToHost, c->stream));
    return CG_OK;
}
static int finish(cg_ctx* c) {
    CG_HIP(c, hipGetLastError());
    if (c->ptr_mode == CG_PTR_HOST) CG_HIP(c, hipStreamSynchronize(c->stream));
    return CG_OK;
}

// workgroup size of the sampler kernels (tools/sampler_threads_sweep.py, round 4, walker-steps/s at the production batch sizes): n = 22: 128 threads
// 8.53 M against 8.37 M with 256, n = 23: 6.19 M against 7.81 M (the concurrent LU pair wants its helper waves); n = 41 ... 56: 512 threads on
// the 512-thread instantiation (256 registers per lane; these sizes used to run the 1024-thread one with 128: n = 45 1.95 -> 2.58 M, n = 53
// 1.60 -> 2.00 M; 768 threads on the latter: 2.02 / 1.63 M); n = 29, 49, 57 run kernels specialised on the size as well
static int auto_threads(int n) {
    if (n <= 16) return 64;
    if (n <= 22) return 128;
    if (n <= 40) return 256;
    if (n <= 64) return 512;
    return 1024;
}
static int threads_of(const cg_ctx* c) { return c->block_threads > 0 ? c->block_threads : auto_threads(c->n); }

static CgDev make_dev(const cg_ctx* c) {
    CgDev m; m.n = c->n; m.L = c->L; m.lay = c->lay;
    return m;
}

// Tuning table: every CG_* environment variable the library reads -- name, built-in choice, meaning -- and the only place that reads
// one (INTEGRATION.md section 5 lists the same names).  Each is read at every call that uses it (tests and the sweeps under tools/ change
// them between calls on a live context); CG_CHOL_QUADRANT_BLOCKS alone is kept in a function-local static by its user (cg_solve.inc).
// Not here: CG_PLAN_DEBUG (prints the placement plan), read with getenv in cg_big.hpp, which the host-side tools compile without HIP.
static inline int cg_env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return v && *v ? atoi(v) : dflt;
}
namespace cg_tune {
// planned kernels of the larger systems (cg_k_big.hip: n > 16, (dim 2, 16, 16) flow)
inline int big()                     { return cg_env_int("CG_BIG", 1); }                             // 0: the first-generation kernels instead
inline int big_lap()                 { return cg_env_int("CG_BIG_LAP", 1); }                         // 0: ... for grad / Laplacian only
inline int big_fused()               { return cg_env_int("CG_BIG_FUSED", 1); }                       // 0: cg_grad_laplacian_scores runs the two kernels one after the other
inline int big_nt(int n, int D)      { return cg_env_int("CG_BIG_NT", n * D <= 64 ? 256 : 512); }    // threads per workgroup (256 / 512)
inline int big_per_cu()              { return cg_env_int("CG_BIG_PER_CU", 2); }                      // workgroups per CU (read for 256 threads; 512: always 1)
inline int big_lds_kb(int per_cu)    { return cg_env_int("CG_BIG_LDS_KB", per_cu == 2 ? 79 : 159); } // LDS the plan may use
inline int big_rounds()              { return cg_env_int("CG_BIG_ROUNDS", 4); }                      // rounds of workgroups per launch of a chunked batch
inline int big_debug()               { return cg_env_int("CG_BIG_DEBUG", 0); }                       // 1: print the layout to stderr at every call
// first-generation derivative kernels where a system does not fit LDS (cg_k_derivs.inc); fit: workgroups whose LDS fits a CU
inline int lap_nt(int n, int D)      { return cg_env_int("CG_LAP_NT", n * D <= 64 ? 256 : 512); }    // k_grad_lap2: threads per workgroup (256 / 512)
inline int lap_lds_kb()              { return cg_env_int("CG_LAP_LDS_KB", 156); }                         // its LDS budget
inline int lap_per_cu(int fit)       { return cg_env_int("CG_LAP_PER_CU", std::min(fit, 2)); }       // workgroups per CU of a launch
inline int vjp_nt()                  { return cg_env_int("CG_VJP_NT", 512); }                        // k_param_vjp: the same three
inline int vjp_lds_kb()              { return cg_env_int("CG_VJP_LDS_KB", 156); }
inline int vjp_per_cu(int fit)       { return cg_env_int("CG_VJP_PER_CU", std::min(fit, 2)); }
inline int vjp_occ(int n, int D)     { return cg_env_int("CG_VJP_OCC", n * D > 64 ? 1 : 0); }        // 1: the 128-register instantiation, two 512-thread workgroups per CU
// fused grad / Laplacian + scores at n <= 16 (cg_k_derivs_a.hip)
inline int small_fused()             { return cg_env_int("CG_SMALL_FUSED", 1); }                     // 0: the two calls one after the other
inline int small_fused_chunk()       { return cg_env_int("CG_SMALL_FUSED_CHUNK", 16384); }           // walkers per launch (77 KB of stash each: 1.2 GB at most)
// Transformer density matrix (cg_k_van.hip, cg_hip.hip)
// CG_VAN_PAR, positions in parallel (0 / 1), has two built-in choices: the several-samples-per-wave kernel of short sequences is on at every
// size it serves, the one-sample-per-wave kernel only from n = 20 (below it most lanes have no position and the sequential kernel wins)
inline int van_par(bool packed, int n) { return cg_env_int("CG_VAN_PAR", packed || n >= 20 ? 1 : 0); }
inline int van_packed()              { return cg_env_int("CG_VAN_PACKED", 1); }                      // 0: never several samples per wave
inline int van_packed_maxn()         { return cg_env_int("CG_VAN_PACKED_MAXN", 33); }                // ... up to this many particles
inline int van_par_waves()           { return cg_env_int("CG_VAN_PAR_WAVES", 0); }                   // waves per workgroup of both (0: as many as LDS allows, <= 4)
inline int van_grad_reg()            { return cg_env_int("CG_VAN_GRAD_REG", 1); }                    // sequential score kernel: -1 runtime dimensions, 0 compile-time
                                       // dimensions, 1 (> 0) + the gradient row in registers where the workgroup has <= 4 waves, 2 also holds it to <= 4 waves
inline int van_static(int B, int cu) { return cg_env_int("CG_VAN_STATIC", B <= 16 * cu ? 1 : 0); }   // sampler / log-probability with compile-time model dimensions
// structure observables (cg_hip.hip)
inline int struct_grid()             { return cg_env_int("CG_STRUCT_GRID", 0); }                     // workgroups of cg_structure_sums along the rows (0: one per row; same bits at any value)
inline int momentum_grid()           { return cg_env_int("CG_MOMENTUM_GRID", 0); }                   // the same for the reduction kernel of cg_momentum_sums
// solver (cg_solve.inc)
inline int fisher_slices()           { return cg_env_int("CG_FISHER_SLICES", 0); }                   // batch slices of cg_fisher_real (0: by occupancy)
inline int chol_quadrant_blocks()    { return cg_env_int("CG_CHOL_QUADRANT_BLOCKS", 1024); }         // fewer 64 x 64 blocks than this: a wave per quadrant (once per process)
inline int chol_no_lookahead()       { return cg_env_int("CG_CHOL_NO_LOOKAHEAD", 0); }               // 1: the whole trailing update on the context's stream
inline int chol_block_nt()           { return cg_env_int("CG_CHOL_BLOCK_NT", 1024); }                // threads of the diagonal-block kernel (256 / 512 / 1024)
}  // namespace cg_tune

template <class K>
static int set_lds(cg_ctx* c, K kernel, size_t bytes) {
    if (bytes > 160 * 1024) CG_FAIL(c, CG_ERR_UNSUPPORTED, "workgroup needs %zu bytes of LDS (> 160 KiB): n too large for the LDS-resident path", bytes);
    if (bytes > 48 * 1024) CG_HIP(c, hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return CG_OK;
}

static int check_ready(cg_ctx* c, const char* fn, int B) {
    if (!c) return CG_ERR_ARG;
    if (B < 0) CG_FAIL(c, CG_ERR_ARG, "%s: negative batch", fn);
    if (!c->have_theta) CG_FAIL(c, CG_ERR_STATE, "%s: cg_set_flow_params has not been called", fn);
    CG_HIP(c, hipSetDevice(c->device));
    return CG_OK;
}

static int ensure_ws(cg_ctx* c, size_t bytes) {
    if (bytes <= c->ws_cap) return CG_OK;
    CG_HIP(c, hipStreamSynchronize(c->stream));
    if (c->ws) { (void)hipFree(c->ws); c->ws = nullptr; c->ws_cap = 0; }
    CG_HIP(c, hipMalloc(&c->ws, bytes));
    c->ws_cap = bytes;
    return CG_OK;
}

// A batch of B walkers, one per workgroup, in launches of `chunk`: the workspace holds a slot of per_wg doubles for each workgroup of a launch
// (+ the pad doubles that caller has always allocated after the last one); launch(grid, w0) issues the kernel for the walkers [w0, w0 + grid).  Returns 1 (launched) or an error.
template <class K, class L>
static int cg_launch_chunked(cg_ctx* c, K kernel, size_t lds, size_t per_wg, size_t pad, int chunk, int B, L&& launch) {
    if (int rc = ensure_ws(c, sizeof(double) * (per_wg * chunk + pad))) return rc;
    if (int rc = set_lds(c, kernel, lds)) return rc;
    for (int w0 = 0; w0 < B; w0 += chunk) launch(std::min(chunk, B - w0), w0);
    return 1;
}

// general-depth launches (cg_k_generic.hip); every array argument is a device pointer
int cg_gen_run_logpsi(cg_ctx* c, const double* x, const int* sidx, int B, int mode, double* logphi, double* hld, double* logpsi_out,
                      double* logp_out, double* z_out, double* J_out);
int cg_gen_run_mcmc(cg_ctx* c, double* x, const int* sidx, int B, int steps, double stddev, uint64_t seed, uint64_t walker_offset,
                    const double* noise, const double* unif, double* logp_out);
int cg_gen_run_param_vjp(cg_ctx* c, int grid, const double* x, const int* sidx, int B, const double* w_re, const double* w_im,
                         double* partial, double* score);
int cg_gen_run_grad_lap(cg_ctx* c, int grid, const double* x, const int* sidx, int B, int mode, const double* v, double* grad, double* lap);
// displaced ratios on device pointers (cg_k_sampler_a.hip): what cg_momentum_sums (cg_hip.hip) runs before its reduction
int cg_displaced_launch(cg_ctx* c, const char* fn, const double* x, const int* sidx, int B, int S, const double* shifts, uint64_t seed,
                        uint64_t walker_offset, double* ratios, double* shifts_out);
extern "C" int cg_fisher_real_nr(cg_ctx* c, const double* S_dev, int B, int P, double* F_dev);
