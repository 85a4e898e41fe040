// tests/host_emul/cg_momentum_emul.cpp -- TEST INFRASTRUCTURE ONLY.
// The momentum-distribution reduction (coulombgas_amd/csrc/cg_momentum.hpp) compiled for the host with the 1-thread workgroup shim of
// cg_common.hpp, rows and row groups summed by the rule the header states.  Built by tests/test_momentum_host.py; never loaded by the
// coulombgas_amd package.
#include <vector>
#include "../../coulombgas_amd/csrc/cg_momentum.hpp"

template <int D>
static void emu_momentum_t(const double* K, int nK, const double* ratios, const double* shifts, int B, int S, int n, double* out) {
    const int W = cg_momentum_width(nK), rows = cg_structure_rows(B), M = S * n;
    std::vector<double> partial((size_t)rows * W, 0.0);
    for (int row = 0; row < rows; ++row)
        for (int k = 0; k < nK; ++k)                  // what threadIdx.x and blockIdx.y walk on the GPU
            cg_momentum_row<D>(ratios, shifts, B, rows, row, M, 1.0 / (double)S, K, nK, k, partial.data() + (size_t)row * W);
    for (int p = 0; p < W; ++p) {
        double a = cg_structure_group_sum(partial.data(), rows, W, p, 0);
        for (int g = 1; g < CG_STRUCT_GROUPS; ++g) a += cg_structure_group_sum(partial.data(), rows, W, p, g);
        out[p] = a;
    }
    out[W] = (double)B;
}

extern "C" int emu_momentum_sums(int n, int dim, const double* K, int nK, const double* ratios, const double* shifts, int B, int S, double* out) {
    if (dim == 2) emu_momentum_t<2>(K, nK, ratios, shifts, B, S, n, out);
    else if (dim == 3) emu_momentum_t<3>(K, nK, ratios, shifts, B, S, n, out);
    else return -1;
    return 0;
}
