// tests/host_emul/cg_structure_emul.cpp -- TEST INFRASTRUCTURE ONLY.
// The structure-observable device code (coulombgas_amd/csrc/cg_structure.hpp) compiled for the host with the 1-thread workgroup shim
// of cg_common.hpp, rows and row groups summed by the rule the header states.  Built by tests/test_structure_host.py; never loaded by
// the coulombgas_amd package.
#include <vector>
#include "../../coulombgas_amd/csrc/cg_structure.hpp"

template <int D>
static void emu_structure_t(int n, double L, const int* K, int nK, int Kmax, int nbins, double rmax, const double* x, int B, double* out) {
    const int T = Kmax + 1, W = 3 * nK + nbins + 1, rows = cg_structure_rows(B);
    const CgBlk b{0, 1};
    const int per = CG_STRUCT_KPT * b.nthr, slices = (nK + per - 1) / per;       // what blockIdx.y walks on the GPU
    const double scale = (double)nbins / rmax;
    std::vector<double> tab((size_t)n * D * T * 2), partial((size_t)rows * W, 0.0);
    std::vector<unsigned> hist(nbins + 1, 0u);
    std::vector<CgStructAcc> acc(slices);
    for (int row = 0; row < rows; ++row) {
        for (auto& a : acc) a.zero();
        for (int w = row; w < B; w += rows) {
            const double* xs = x + (size_t)w * n * D;
            cg_structure_tables<D>(b, xs, n, L, T, tab.data());
            for (int s = 0; s < slices; ++s) {
                int kv[CG_STRUCT_KPT][D];
                cg_structure_load_k<D>(b, K, s * per, nK, kv);
                cg_structure_add_walker<D>(b, tab.data(), n, T, s * per, nK, kv, acc[s]);
            }
            cg_structure_pairs<D>(b, xs, n, L, nbins, scale, hist.data());
        }
        double* prow = partial.data() + (size_t)row * W;
        for (int s = 0; s < slices; ++s) cg_structure_store_k(b, s * per, nK, acc[s], prow);
        cg_structure_store_hist(b, nbins, hist.data(), prow + 3 * nK);
    }
    for (int p = 0; p < W; ++p) {
        double a = cg_structure_group_sum(partial.data(), rows, W, p, 0);
        for (int g = 1; g < CG_STRUCT_GROUPS; ++g) a += cg_structure_group_sum(partial.data(), rows, W, p, g);
        out[p] = a;
    }
    out[W] = (double)B;
}

extern "C" int emu_structure_sums(int n, int dim, double L, const int* K, int nK, int nbins, double rmax, const double* x, int B, double* out) {
    int Kmax = 0;
    for (int e = 0; e < nK * dim; ++e) Kmax = K[e] < 0 ? (-K[e] > Kmax ? -K[e] : Kmax) : (K[e] > Kmax ? K[e] : Kmax);
    if (dim == 2) emu_structure_t<2>(n, L, K, nK, Kmax, nbins, rmax, x, B, out);
    else if (dim == 3) emu_structure_t<3>(n, L, K, nK, Kmax, nbins, rmax, x, B, out);
    else return -1;
    return 0;
}
