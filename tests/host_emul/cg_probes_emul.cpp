// tests/host_emul/cg_probes_emul.cpp -- TEST INFRASTRUCTURE ONLY.
// The probe loop of cg_grad_laplacian_probes compiled for the host with the 1-thread workgroup shim of cg_common.hpp:
//   emu_grad_laplacian_probes  CgLap::grad_laplacian<AL, MP = true> (coulombgas_amd/csrc/cg_lap.hpp), the loop of k_grad_lap2_probes;
//                              lds_budget selects the all-in-LDS or the block-wise layout as in cg_emul.cpp
//   emu_probe_combine          cg_probe_add / cg_probe_fold on given per-pass partial sums: the combination rule that the loop of
//                              CgBig::grad_laplacian<MP = true> (cg_big.hpp; its passes are DPP / MFMA code, device only) shares with CgLap
// Built by tests/test_probes_host.py; never loaded by the coulombgas_amd package.
#include <vector>
#include <cstring>
#include "../../coulombgas_amd/csrc/cg_common.hpp"
#include "../../coulombgas_amd/csrc/cg_linalg.hpp"
#include "../../coulombgas_amd/csrc/cg_flow_fast.hpp"
#include "../../coulombgas_amd/csrc/cg_dispatch.hpp"
#include "../../coulombgas_amd/csrc/cg_lap.hpp"

template <int D, int HS, int HT>
static void emu_probes_t(int n, double L, const double* theta, const double* sp_indices, int M, const int* sidx, const double* x, int B, int mode,
                         int nprobe, const double* v, double weight, double* grad, double* lap, long lds_budget) {
    using G = CgLap<D, HS, HT>;
    const auto lay = G::layout(n, 1, mode, (size_t)lds_budget);
    std::vector<double> ws(lay.ws_total + 8), lds(lay.lds_total + 8), spk((size_t)M * D);
    for (size_t i = 0; i < spk.size(); ++i) spk[i] = sp_indices[i] * (2.0 * CG_PI / L);
    CgBlk b{0, 1};
    const double* th = theta;
    if (lay.th_lds) { memcpy(lds.data() + lay.th, theta, sizeof(double) * G::NP); th = lds.data() + lay.th; }
    const size_t N = (size_t)n * D;
    for (int w = 0; w < B; ++w) {
        if (lay.all_lds)
            G::template grad_laplacian<true, true>(b, th, x + w * N, spk.data(), sidx + (size_t)w * n, n, L, mode, v + w * N, grad + w * N * 2, lap + 2 * w,
                                                   lds.data(), ws.data(), lay, nullptr, nullptr, nprobe, (size_t)B * N, weight);
        else
            G::template grad_laplacian<false, true>(b, th, x + w * N, spk.data(), sidx + (size_t)w * n, n, L, mode, v + w * N, grad + w * N * 2, lap + 2 * w,
                                                    lds.data(), ws.data(), lay, nullptr, nullptr, nprobe, (size_t)B * N, weight);
    }
}

extern "C" int emu_grad_laplacian_probes(int n, int dim, int hs, int ht, double L, const double* theta, const double* sp_indices, int M, const int* sidx,
                                         const double* x, int B, int mode, int nprobe, const double* v, double weight, double* grad, double* lap,
                                         long lds_budget) {
    if ((mode != 1 && mode != 2) || nprobe < 1 || !v) return -1;
#define CG_X(D, HS, HT) if (dim == D && hs == HS && ht == HT) { emu_probes_t<D, HS, HT>(n, L, theta, sp_indices, M, sidx, x, B, mode, nprobe, v, weight, grad, lap, lds_budget); return 0; }
    CG_FAST_CONFIGS(CG_X)
#undef CG_X
    return -1;
}

// tot (4, in / out): a thread's probe-free partials; r (nprobe, 4): its partial sums of the passes
extern "C" void emu_probe_combine(int nprobe, const double* r, double weight, double* tot) {
    double acc[4] = {0, 0, 0, 0}, t[4] = {tot[0], tot[1], tot[2], tot[3]};
    for (int k = 0; k < nprobe; ++k) {
        const double rk[4] = {r[4 * k], r[4 * k + 1], r[4 * k + 2], r[4 * k + 3]};
        cg_probe_add(acc, rk, k);
    }
    cg_probe_fold(t, acc, weight);
    for (int i = 0; i < 4; ++i) tot[i] = t[i];
}
