// tests/host_emul/cg_pathmap.cpp -- TEST INFRASTRUCTURE ONLY.
// Which kernel path a depth-2 fast configuration (dim, spsize, tpsize) takes at a particle number n, computed from the project's own
// layout functions (cg_fast_layout, CgLap::layout, CgDerivs::layout, CgScore::layout) compiled for the host, as cg_emul.cpp compiles
// them.  tests/test_path_coverage.py asserts with it that every distinct path of the second translation unit's configurations has a
// shape in tests/config_shapes.py, so that a changed threshold fails on the CPU instead of leaving a GPU test that covers nothing.
//
// The launch conditions themselves live in files that need HIP (.inc / .hip, cg_host.hpp) and are RESTATED here; each restatement
// names the lines it mirrors.  tests/test_gpu_configs.py cross-checks `threads` and `fast` with cg_get_launch_info on the device.
#include <cstring>
#include <algorithm>
#include "../../coulombgas_amd/csrc/cg_common.hpp"
#include "../../coulombgas_amd/csrc/cg_linalg.hpp"
#include "../../coulombgas_amd/csrc/cg_flow_fast.hpp"
#include "../../coulombgas_amd/csrc/cg_dispatch.hpp"
#include "../../coulombgas_amd/csrc/cg_derivs.hpp"
#include "../../coulombgas_amd/csrc/cg_lap.hpp"
#include "../../coulombgas_amd/csrc/cg_score.hpp"

// cg_host.hpp:183-189 auto_threads
static int pm_auto_threads(int n) {
    if (n <= 16) return 64;
    if (n <= 22) return 128;
    if (n <= 40) return 256;
    if (n <= 64) return 512;
    return 1024;
}

enum { PM_LU_WAVE_BOTH_26_13 = 0, PM_LU_WAVE_TWO_PHASE = 1, PM_LU_DUAL2 = 2, PM_LU_DUAL = 3, PM_LU_SEQUENTIAL = 4, PM_LU_WAVE_BOTH_32_16 = 5 };
enum { PM_SCORE_K_SCORES = 0, PM_SCORE_VJP_256 = 1, PM_SCORE_VJP_512_WPE1 = 2, PM_SCORE_VJP_512_WPE4 = 3 };
enum { PM_FIELDS = 26 };

// out[0..6]   sampler: threads, fast, wave_lu, dual, Dm == J, U != J, LU branch
// out[7+5m..] grad / Laplacian in mode m = 0, 1, 2: all-LDS, threads, P_lds, A_lds, B_lds (the last four 0 when all-LDS)
// out[22..25] scores: kernel variant, vjp_da, inverses in LDS (vjp_fast > 0), panels staged in LDS (stage > 0)
template <int D, int HS, int HT>
static void pathmap_t(int n, int* out) {
    const int N = n * D;
    // ---- sampler ----
    const int nthr = pm_auto_threads(n);
    // cg_hip.hip:345-353 (cg_create): the layout of the sampler kernels and the 160 KiB test of the LDS-resident path
    const CgFastLds o = cg_fast_layout(n, D, HS, HT, true, HS == 16 && HT == 16);
    const size_t NN = (size_t)N;
    const int fast = sizeof(double) * (CG_TAB_DOUBLES + (size_t)o.total + 3 * ((NN + 1) & ~(size_t)1) + 2) > 160 * 1024 ? 0 : 1;
    // cg_flow_fast.hpp:1425-1487 (CgFast::logpsi, device branch): which LU code factors J and the Slater matrix
    int lu;
    if (o.wave_lu) lu = (nthr == 64 && (n == 13 || n == 16) && N == 2 * n) ? (n == 13 ? PM_LU_WAVE_BOTH_26_13 : PM_LU_WAVE_BOTH_32_16) : PM_LU_WAVE_TWO_PHASE;
    else if (o.dual && nthr >= 192 && nthr <= 1024 && N <= 128 && n <= 64) lu = ((N & 1) == 0 && n >= 8) ? PM_LU_DUAL2 : PM_LU_DUAL;
    else lu = PM_LU_SEQUENTIAL;
    out[0] = nthr; out[1] = fast; out[2] = o.wave_lu; out[3] = o.dual; out[4] = o.Dm == o.J ? 1 : 0; out[5] = o.U != o.J ? 1 : 0; out[6] = lu;
    // ---- grad / Laplacian: cg_k_derivs.inc:128-151 (grad_lap), cg_host.hpp:216-217 (lap_nt, lap_lds_kb) ----
    for (int mode = 0; mode < 3; ++mode) {
        int* q = out + 7 + 5 * mode;
        auto dl = CgLap<D, HS, HT>::layout(n, 256, mode, (size_t)(80 * 1024) / sizeof(double) - CG_TAB_DOUBLES);
        if (dl.all_lds && dl.th_lds) { q[0] = 1; q[1] = q[2] = q[3] = q[4] = 0; continue; }
        const int nt = N <= 64 ? 256 : 512;
        dl = CgLap<D, HS, HT>::layout(n, nt, mode, (size_t)156 * 1024 / sizeof(double) - CG_TAB_DOUBLES);
        q[0] = 0; q[1] = nt; q[2] = dl.P_lds; q[3] = dl.A_lds; q[4] = dl.B_lds;
    }
    // ---- scores: cg_k_derivs.inc:218-230 (scores), :180-215 (param_vjp), cg_host.hpp:219-222 (vjp_nt, vjp_lds_kb, vjp_per_cu, vjp_occ) ----
    int* s = out + 22;
    typedef CgDerivs<D, HS, HT> Dv;
    bool k_scores = false;
    if (HS == 16 && HT == 16) k_scores = CgScore<D, HS, HT>::layout(n, 256, (size_t)(80 * 1024) / sizeof(double) - CG_TAB_DOUBLES).ok != 0;
    auto vl = Dv::layout(n, 256);
    if (k_scores) { s[0] = PM_SCORE_K_SCORES; s[1] = s[2] = s[3] = 0; return; }
    if (vl.vjp_fast) { s[0] = PM_SCORE_VJP_256; }
    else {
        const int nt = 512;
        vl = Dv::layout(n, nt, (size_t)156 * 1024);
        const size_t lds = sizeof(double) * (CG_TAB_DOUBLES + Dv::lds_doubles(n, nt) + Dv::vjp_lds_doubles(vl));
        const int fit = (int)std::max<size_t>(1, (size_t)(160 * 1024) / (lds + 512));
        const int per_cu = std::min(fit, 2);
        const bool occ = N > 64 && per_cu >= 2;
        s[0] = occ ? PM_SCORE_VJP_512_WPE4 : PM_SCORE_VJP_512_WPE1;
    }
    s[1] = vl.vjp_da; s[2] = vl.vjp_fast > 0 ? 1 : 0; s[3] = vl.stage > 0 ? 1 : 0;
}

extern "C" int cg_pathmap_fields(void) { return PM_FIELDS; }

// 0: filled; -1: (dim, spsize, tpsize) is not a compiled configuration of the fast path
extern "C" int cg_pathmap(int dim, int hs, int ht, int n, int* out) {
    if (n < 1) return -2;
#define CG_X(D, HS, HT) if (dim == D && hs == HS && ht == HT) { pathmap_t<D, HS, HT>(n, out); return 0; }
    CG_FAST_CONFIGS(CG_X)
#undef CG_X
    return -1;
}

// the configurations of the second translation unit (CG_FAST_CONFIGS_B), three ints each; returns how many
extern "C" int cg_pathmap_unit_b(int* out, int cap) {
    int k = 0;
#define CG_X(D, HS, HT) if (k < cap) { out[3 * k] = D; out[3 * k + 1] = HS; out[3 * k + 2] = HT; } ++k;
    CG_FAST_CONFIGS_B(CG_X)
#undef CG_X
    return k;
}
