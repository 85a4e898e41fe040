// cg_solve.inc -- classical Fisher matrix of the SR optimizer on the device (src/sr.py:36, 74): real SYRK with f64 MFMA.
// The damped solve (src/sr.py:38-45, 102-117) uses cg_cholesky below: a right-looking blocked Cholesky written here
// (64-column panels: diagonal block in LDS, panel by forward substitution one thread per row, trailing update as
// 16 x 16 f64 MFMA tiles with K = 64) -- rocSOLVER's first call stalled for minutes on fresh boxes while the rocBLAS
// kernel library paged in.  cg_spd_solve adds the damping, factors and runs both triangular solves on the device.
// Included at the end of cg_hip.hip.

// F[p][q] = (scale) sum_{b in slice} S[b][p] S[b][q] for a real (B x P) score matrix (classical Fisher matrix, src/sr.py:74 / :36).
// One wave owns a 64 x 64 block of F as 4 x 4 MFMA tiles (16 accumulators, 8 operand loads per 16 MFMAs); the four waves of a
// workgroup form a 128 x 128 block.  MFMA row i of tile a is parameter p0 + 4 i + a, so that a lane's four operands are 32
// contiguous bytes of a row of S and its 4 x 4 results 32 contiguous bytes of a row of F.  blockIdx.z slices the batch
// (partial matrices, summed in fixed order by k_rows_sum) when P alone gives too few workgroups.
#define CG_MFMA_4X4(acc, av, bv)                                                                                          \
    _Pragma("unroll") for (int a_ = 0; a_ < 4; ++a_)                                                                      \
        _Pragma("unroll") for (int c_ = 0; c_ < 4; ++c_)(acc)[a_][c_] = __builtin_amdgcn_mfma_f64_16x16x4f64((av)[a_], (bv)[c_], (acc)[a_][c_], 0, 0, 0)
__global__ void __launch_bounds__(256, 2) k_fisher_real(const double* __restrict__ S, int B, int P, int chunk, double scale, double* __restrict__ F) {
    typedef double d4_t __attribute__((ext_vector_type(4)));
    if (blockIdx.x < blockIdx.y) return;                                  // upper block-triangle only; mirrored on the way out
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p0 = 128 * blockIdx.y + 64 * (wave >> 1), q0 = 128 * blockIdx.x + 64 * (wave & 1);
    if (p0 >= P || q0 >= P || q0 + 64 <= p0) return;
    const int col = lane & 15, kq = lane >> 4;
    const int b0 = blockIdx.z * chunk, b1 = min(B, b0 + chunk);
    F += (size_t)blockIdx.z * P * P;
    d4_t acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = d4_t{0, 0, 0, 0};
    const int pl = p0 + 4 * col, ql = q0 + 4 * col;
    int bb = b0;
    if (p0 + 64 <= P && q0 + 64 <= P && b1 - b0 >= 8) {                   // interior block (wave-uniform): operands of step
        const double* pa = S + (size_t)(b0 + kq) * P + pl;                // t + 1 are in flight while step t multiplies
        const double* pb = S + (size_t)(b0 + kq) * P + ql;
        const size_t step = (size_t)4 * P;
        double av[4], bv[4], an[4], bn[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) { av[a] = pa[a]; bv[a] = pb[a]; }
        const int steps = (b1 - b0) >> 2;
        for (int t = 1; t < steps; ++t) {
            pa += step; pb += step;
#pragma unroll
            for (int a = 0; a < 4; ++a) { an[a] = pa[a]; bn[a] = pb[a]; }
            CG_MFMA_4X4(acc, av, bv);
#pragma unroll
            for (int a = 0; a < 4; ++a) { av[a] = an[a]; bv[a] = bn[a]; }
        }
        CG_MFMA_4X4(acc, av, bv);
        bb = b0 + 4 * steps;
    }
    for (; bb < b1; bb += 4) {                                            // ragged blocks and the last rows of the batch
        const int b = bb + kq;
        double av[4], bv[4];
        const double* rowp = S + (size_t)min(b, B - 1) * P;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            av[a] = (b < b1 && pl + a < P) ? rowp[pl + a] : 0.0;
            bv[a] = (b < b1 && ql + a < P) ? rowp[ql + a] : 0.0;
        }
        CG_MFMA_4X4(acc, av, bv);
    }
    const bool mirror = q0 != p0;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int pr = p0 + 4 * (kq + 4 * r) + a;
            if (pr >= P) continue;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int q = ql + c;
                if (q < P) {
                    const double v = acc[a][c][r] * scale;
                    F[(size_t)pr * P + q] = v;
                    if (mirror) F[(size_t)q * P + pr] = v;
                }
            }
        }
}
// launch of the above on device pointers; partial matrices from the arena when the batch is sliced
static int fisher_real_launch(cg_ctx* c, const double* S, int B, int P, double* F) {
    const int nbt = (P + 127) / 128, blocks = nbt * (nbt + 1) / 2;
    int nsl = 1;
    while (nsl < 16 && blocks * nsl < c->cu_count && B / (2 * nsl) >= 64) nsl *= 2;
    // a few rounds of workgroups per CU (P = 5907: 1128 blocks on 256 CUs = 4.4 -> 5 rounds, one of them 40 % full): four batch slices give
    // 17.6 rounds of quarter-length blocks; 6.9 -> 5.9 ms at B = 8192 with the fixed-order sum of the partial matrices included
    if (nsl == 1 && blocks >= c->cu_count && blocks < 8 * c->cu_count && B >= 4096) nsl = 4;
    { const int f = cg_tune::fisher_slices(); if (f > 0) nsl = f; }
    const int chunk = (((B + nsl - 1) / nsl) + 3) & ~3;
    if (nsl == 1) {
        hipLaunchKernelGGL(k_fisher_real, dim3(nbt, nbt, 1), dim3(256), 0, c->stream, S, B, P, chunk, 1.0 / (double)B, F);
    } else {
        double* part = (double*)arena_take(c, sizeof(double) * (size_t)nsl * P * P);
        if (!part) CG_FAIL(c, CG_ERR_HIP, "Fisher matrix: workspace allocation failed");
        hipLaunchKernelGGL(k_fisher_real, dim3(nbt, nbt, nsl), dim3(256), 0, c->stream, S, B, P, chunk, 1.0, part);
        hipLaunchKernelGGL(k_rows_sum, dim3((P * P + 255) / 256), dim3(256), 0, c->stream, (const double*)part, nsl, P * P, 1.0 / (double)B, F);
    }
    CG_HIP(c, hipGetLastError());
    return CG_OK;
}
#define CG_CHOL_NB 64
#define CG_CHOL_OUTER 256
// Blocked right-looking factorisation in 256-column outer blocks, THREE launches per outer block:
//  k_chol_block  the 256 x 256 diagonal block, one workgroup, 64 columns at a time: (a) the 64 x 64 diagonal block by FOUR waves in
//                16 x 16 tiles through LDS: per tile column the diagonal tile is factored and inverted by 16 lanes in registers
//                (16 dependent columns instead of 64; DPP row broadcasts), the tiles below it are L_it = A_it X_tt^T and the
//                trailing tiles A_ij -= L_it L_jt^T on the matrix cores; then X = L^-1 block column by block column (X_ij =
//                -X_ii sum_k L_ik X_kj, one wave per block column); L_kk and X are stored (the panels and the triangular solves
//                multiply by X instead of substituting); (b) the (at most three) 64-row panels below it inside the outer block,
//                L = A X^T, stored and kept in LDS; (c) their update of the rest of the outer block, A_ij -= L_i L_j^T.
//                info = first non-positive pivot + 1; rows / columns >= nb of the last block are padded with the identity.
//  k_chol_trsm   every 64-row block BELOW the outer block: its four 64-column panels in one pass, L_j = (A_j - sum_{i<j} L_i
//                L_ji^T) X_jj^T, the earlier L_i of the rows kept in LDS (no workgroup depends on another);
//  k_chol_update the trailing matrix, K = 256.
// Round 2 / early round 3 launched diagonal block, panel and inner update per 64 columns (3 x 93 + 23 launches at P = 5907, 24 + 13
// + 21 us per step with the GPU all but idle): the chain is now ~55 + 15 us per 256 columns.
#define CG_CHOL_LD 66                      /* LDS row stride (doubles): 64 would put a tile's 16 rows on one bank */
#if defined(__HIP_DEVICE_COMPILE__)
// lane LANE of every 16-lane DPP row to the whole row (row_newbcast): the broadcasts of the 16 x 16 tile sweeps without the
// VALU -> SGPR -> VALU round trip of v_readlane
template <int LANE>
static __device__ __forceinline__ double cg_bcast16(double v) {
    const long long u = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)u, 0x150 + LANE, 0xf, 0xf, true);      // (bound_ctrl: no zero-initialised destination,
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(u >> 32), 0x150 + LANE, 0xf, 0xf, true); //  two moves fewer per broadcast; every lane has a source)
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
template <int J, int C>
static __device__ __forceinline__ void cg_chol16_upd(double (&a)[16], double l) {
    if constexpr (C < 16) { a[C] = fma(-l, cg_bcast16<C>(l), a[C]); cg_chol16_upd<J, C + 1>(a, l); }
}
// X = L^-1 of the 16 x 16 tile, lane = column i: x[R] = (delta_Ri - sum_{K<R} L[R][K] x[K]) / L[R][R].  Column-oriented: as soon as x[K]
// is final every later row takes its term (s[R] -= L[R][K] x[K], independent of one another), so the dependent path of row R is one
// multiply-add and one multiply instead of R multiply-adds in sequence; the order of the terms of a row is unchanged (same bits).
template <int K, int R>
static __device__ __forceinline__ void cg_chol16_inv_upd(const double (&a)[16], double (&sacc)[16], double xk) {
    if constexpr (R < 16) { sacc[R] = fma(-cg_bcast16<R>(a[K]), xk, sacc[R]); cg_chol16_inv_upd<K, R + 1>(a, sacc, xk); }
}
template <int K>
static __device__ __forceinline__ void cg_chol16_inv(const double (&a)[16], double (&x)[16], double (&sacc)[16], double rdiag) {
    if constexpr (K < 16) {
        x[K] = sacc[K] * cg_bcast16<K>(rdiag);
        cg_chol16_inv_upd<K, K + 1>(a, sacc, x[K]);
        __builtin_amdgcn_sched_barrier(0);            // (the scheduler otherwise hoists all 120 broadcasts: 240 live VGPRs, spills)
        cg_chol16_inv<K + 1>(a, x, sacc, rdiag);
    }
}
template <int J>
static __device__ __forceinline__ void cg_chol16_col(double (&a)[16], int i, double& rdiag, int& bad, int gcol) {
    if constexpr (J < 16) {
        const double d = cg_bcast16<J>(a[J]);
        if (!(d > 0.0)) { if (bad == 0) bad = gcol + J + 1; }
        double rs = __builtin_amdgcn_rsq(d);
        const double hd = 0.5 * d;
        rs = rs * fma(-hd * rs, rs, 1.5);
        rs = rs * fma(-hd * rs, rs, 1.5);
        double sd = d * rs;
        sd = fma(0.5 * rs, fma(-sd, sd, d), sd);
        const double l = (i == J) ? sd : a[J] * rs;
        if (i == J) rdiag = rs;
        a[J] = l;
        cg_chol16_upd<J, J + 1>(a, l);
        __builtin_amdgcn_sched_barrier(0);
        cg_chol16_col<J + 1>(a, i, rdiag, bad, gcol);
    }
}
#endif
#define CG_CHOL_BLOCK_LDS (sizeof(double) * (4 * 64 * CG_CHOL_LD + 4 * 16 * 18) + 16)
#define CG_CHOL_XINV_LDS (sizeof(double) * (4 * 64 * CG_CHOL_LD))
#define CG_CHOL_TRSM_LDS (sizeof(double) * (2 * 64 * CG_CHOL_LD))
#if defined(__HIP_DEVICE_COMPILE__)
// rows [r0, r0 + 64) of a 64-column panel into dst (LDS, 64 x CG_CHOL_LD): L = A[rows, k0:k0+nb] X^T, X (= L_kk^-1) in LDS (xs_ld) or
// global (ld 64); one wave per 16 rows, K = 64
template <bool XLDS>
static __device__ __forceinline__ void cg_chol_panel_rows(double* __restrict__ A, int P, int k0, int nb, const double* X, int r0, double* dst, int strip, int col, int kq) {
    typedef double d4_t __attribute__((ext_vector_type(4)));
    constexpr int XLD = XLDS ? CG_CHOL_LD : CG_CHOL_NB;
    const int ra = r0 + 16 * strip + col;
    const double* pa = A + (size_t)min(ra, P - 1) * P + k0;
    double av[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) { const int k = 4 * s + kq; av[s] = (ra < P && k < nb) ? pa[k] : 0.0; }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        d4_t acc = {0, 0, 0, 0};
#pragma unroll
        for (int s = 0; s < 16; ++s)                                     // B operand [k][j] = X[16 c + j][k]
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], X[(16 * c + col) * XLD + 4 * s + kq], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int lr = 16 * strip + kq + 4 * r, j = 16 * c + col;
            dst[lr * CG_CHOL_LD + j] = acc[r];
            if (r0 + lr < P && j < nb) A[(size_t)(r0 + lr) * P + k0 + j] = acc[r];
        }
    }
}
#endif
__global__ void __launch_bounds__(1024) k_chol_block(double* __restrict__ A, int P, int o0, int oe, int* __restrict__ info, double* __restrict__ Linv_all,
                                                      double* __restrict__ Xo /* 256 x 256: receives the diagonal blocks of L_oo^-1 */) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef double d4_t __attribute__((ext_vector_type(4)));
    extern __shared__ double cg_chol_lds[];
#ifdef CG_CHOL_STAMPS                      /* diagnostic build: cycles per phase of the first outer block, printed by thread 0 */
    unsigned long long st_acc[7] = {0, 0, 0, 0, 0, 0, 0}, st_t = __builtin_amdgcn_s_memtime();
#define CG_CST(i) { const unsigned long long st_n = __builtin_amdgcn_s_memtime(); st_acc[i] += st_n - st_t; st_t = st_n; }
#else
#define CG_CST(i)
#endif
#pragma unroll 1
    for (int k0 = o0; k0 < oe; k0 += CG_CHOL_NB) {
    int lds0 = 0;
    asm volatile("" : "+v"(lds0));          // (opaque per step: otherwise every LDS address of the step is hoisted out of the loop and spilled)
    double* Ls = cg_chol_lds + lds0; double* Xs = Ls + 64 * CG_CHOL_LD; double* Qs = Xs + 64 * CG_CHOL_LD;      // Qs: two panel buffers
    double (*Ts)[16 * 18] = (double (*)[16 * 18])(Qs + 2 * 64 * CG_CHOL_LD);
    int& bad_s = *(int*)(Qs + 2 * 64 * CG_CHOL_LD + 4 * 16 * 18);
    const int nb = min(CG_CHOL_NB, P - k0);
    double* Linv = Linv_all + (size_t)(k0 / CG_CHOL_NB) * CG_CHOL_NB * CG_CHOL_NB;
    __syncthreads();
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));          // (likewise: nothing derived from the lane index is hoisted out of the step)
    const int nthr = blockDim.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), col = lane & 15, kq = lane >> 4;
    for (int e = tid; e < 64 * 64; e += nthr) {
        const int i = e >> 6, j = e & 63;
        Ls[i * CG_CHOL_LD + j] = (i < nb && j < nb) ? (j <= i ? A[(size_t)(k0 + i) * P + k0 + j] : 0.0) : (i == j ? 1.0 : 0.0);
        Xs[i * CG_CHOL_LD + j] = 0.0;
    }
    if (tid == 0) bad_s = 0;
    __syncthreads();
    CG_CST(0)
    auto tile_mm = [&](const double* Am, const double* Bm, bool bt, d4_t c) {     // c += A (16 x 16) * (bt ? B^T : B), operands in LDS
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int k = 4 * ks + kq;
            const double av = Am[col * CG_CHOL_LD + k];
            const double bv = bt ? Bm[col * CG_CHOL_LD + k] : Bm[k * CG_CHOL_LD + col];
            c = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, c, 0, 0, 0);
        }
        return c;
    };
#pragma unroll 1
    for (int t = 0; t < 4; ++t) {
        double* Ltt = Ls + (16 * t) * CG_CHOL_LD + 16 * t; double* Xtt = Xs + (16 * t) * CG_CHOL_LD + 16 * t;
        if (wave == 0) {                          // diagonal tile: unblocked Cholesky + inverse, lane = row, the row in registers
            int i = lane & 15;
            asm volatile("" : "+v"(i));
            double a[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) a[j] = Ltt[i * CG_CHOL_LD + j];
            int bad = 0;
            double rdiag = 1.0;
            cg_chol16_col<0>(a, i, rdiag, bad, k0 + 16 * t);      // (a non-positive pivot gives NaNs; the block is then abandoned below)
#pragma unroll
            for (int j = 0; j < 16; ++j) asm volatile("" : "+v"(a[j]));      // (or the 120 broadcasts of the sweep are kept alive for the inverse: spills)
            double x[16], sacc[16];               // X_tt = L_tt^-1, lane = column
#pragma unroll
            for (int r = 0; r < 16; ++r) sacc[r] = (r == i) ? 1.0 : 0.0;
            cg_chol16_inv<0>(a, x, sacc, rdiag);
#pragma unroll
            for (int r = 0; r < 16; ++r) asm volatile("" : "+v"(x[r]));      // (or the products are sunk into the branch below, the convergent broadcasts are not, and all 120 stay live)
            bad = __builtin_amdgcn_readfirstlane(bad);
            if (lane < 16) {
#pragma unroll
                for (int j = 0; j < 16; ++j) Ltt[i * CG_CHOL_LD + j] = j <= i ? a[j] : 0.0;
#pragma unroll
                for (int r = 0; r < 16; ++r) Xtt[r * CG_CHOL_LD + i] = i <= r ? x[r] : 0.0;
            }
            if (lane == 0 && bad) bad_s = bad;
        }
        __syncthreads();
        if (bad_s) { if (tid == 0 && *info == 0) *info = bad_s; return; }
        for (int i = t + 1 + wave; i < 4; i += 4) {           // tiles below: L_it = A_it X_tt^T
            double* Ait = Ls + (16 * i) * CG_CHOL_LD + 16 * t;
            d4_t c = {0, 0, 0, 0};
            c = tile_mm(Ait, Xtt, true, c);
            asm volatile("" ::: "memory");                     // (the wave's own reads of A_it are complete: in-order LDS)
#pragma unroll
            for (int r = 0; r < 4; ++r) Ait[(kq + 4 * r) * CG_CHOL_LD + col] = c[r];
        }
        __syncthreads();
        {   // trailing tiles (i, j), t < j <= i: A_ij -= L_it L_jt^T
            int q = 0;
            for (int i = t + 1; i < 4; ++i)
                for (int j = t + 1; j <= i; ++j, ++q) {
                    if ((q & 3) != wave) continue;
                    double* Aij = Ls + (16 * i) * CG_CHOL_LD + 16 * j;
                    d4_t c = {0, 0, 0, 0};
                    c = tile_mm(Ls + (16 * i) * CG_CHOL_LD + 16 * t, Ls + (16 * j) * CG_CHOL_LD + 16 * t, true, c);
#pragma unroll
                    for (int r = 0; r < 4; ++r) Aij[(kq + 4 * r) * CG_CHOL_LD + col] -= c[r];
                }
        }
        __syncthreads();
    }
    // X = L^-1: block column j by wave j; X_ij = -X_ii (sum_{k = j}^{i-1} L_ik X_kj), i = j + 1 ... 3 in order
    CG_CST(1)
    if (wave < 4) {
        const int j = wave;
        double* T = Ts[wave];
        for (int i = j + 1; i < 4; ++i) {
            d4_t c = {0, 0, 0, 0};
            for (int k = j; k < i; ++k) c = tile_mm(Ls + (16 * i) * CG_CHOL_LD + 16 * k, Xs + (16 * k) * CG_CHOL_LD + 16 * j, false, c);
#pragma unroll
            for (int r = 0; r < 4; ++r) T[(kq + 4 * r) * 18 + col] = c[r];
            asm volatile("" ::: "memory");
            d4_t x = {0, 0, 0, 0};
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const int k = 4 * ks + kq;
                x = __builtin_amdgcn_mfma_f64_16x16x4f64(Xs[(16 * i + col) * CG_CHOL_LD + 16 * i + k], T[k * 18 + col], x, 0, 0, 0);
            }
            asm volatile("" ::: "memory");
#pragma unroll
            for (int r = 0; r < 4; ++r) Xs[(16 * i + kq + 4 * r) * CG_CHOL_LD + 16 * j + col] = -x[r];
            asm volatile("" ::: "memory");
        }
    }
    __syncthreads();
    CG_CST(2)
    for (int e = tid; e < 64 * 64; e += nthr) {
        const int i = e >> 6, j = e & 63;
        const double xv = j <= i ? Xs[i * CG_CHOL_LD + j] : 0.0;
        if (i < nb && j <= i) A[(size_t)(k0 + i) * P + k0 + j] = Ls[i * CG_CHOL_LD + j];
        Linv[i * CG_CHOL_NB + j] = xv;
        Xo[(size_t)(k0 - o0 + i) * CG_CHOL_OUTER + (k0 - o0 + j)] = xv;
    }
    const int cb = k0 + nb, nq = (oe - cb + 63) / 64;                // row blocks left in the outer block (<= 3)
    if (nq <= 0) break;
    __syncthreads();                                        // (L_kk is stored: its LDS copy becomes the first panel buffer)
    CG_CST(3)
    for (int task = wave; task < 4 * nq; task += nthr >> 6) {  // (b): one wave per 16 rows of the (at most three) panels
        const int ib = task >> 2;
        cg_chol_panel_rows<true>(A, P, k0, nb, Xs, cb + 64 * ib, ib == 0 ? Ls : Qs + (ib - 1) * 64 * CG_CHOL_LD, task & 3, col, kq);
    }
    __syncthreads();
    CG_CST(4)
    for (int task = wave; task < 2 * nq * (nq + 1); task += nthr >> 6) {     // (c): 16 rows of block (ib, tj <= ib): C -= L_ib L_tj^T
        const int pair = task >> 2, strip = task & 3;
        const int ib = pair < 1 ? 0 : (pair < 3 ? 1 : 2), tj = pair - (ib * (ib + 1)) / 2;
        const double* Li = ib == 0 ? Ls : Qs + (ib - 1) * 64 * CG_CHOL_LD;
        const double* Lj = tj == 0 ? Ls : Qs + (tj - 1) * 64 * CG_CHOL_LD;
        const int p0 = cb + 64 * ib + 16 * strip, q0 = cb + 64 * tj;
        double cv[4][4];
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int pr = p0 + kq + 4 * r, qc = q0 + 16 * c + col;
                cv[c][r] = (pr < P && qc < oe && qc <= pr) ? A[(size_t)pr * P + qc] : 0.0;
            }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            d4_t acc = {0, 0, 0, 0};
#pragma unroll
            for (int ks = 0; ks < 16; ++ks)
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Li[(16 * strip + col) * CG_CHOL_LD + 4 * ks + kq], Lj[(16 * c + col) * CG_CHOL_LD + 4 * ks + kq], acc, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int pr = p0 + kq + 4 * r, qc = q0 + 16 * c + col;
                if (pr < P && qc < oe && qc <= pr) A[(size_t)pr * P + qc] = cv[c][r] - acc[r];
            }
        }
    }
    __threadfence_block();
    __syncthreads();
    CG_CST(5)
    }
#ifdef CG_CHOL_STAMPS
    if (threadIdx.x == 0 && o0 == 0) printf("k_chol_block cycles: load %llu  factor %llu  X %llu  writeback %llu  panels %llu  update %llu\n", st_acc[0], st_acc[1], st_acc[2], st_acc[3], st_acc[4], st_acc[5]);
#endif
#endif
}
// the blocks below the diagonal of X_oo = L_oo^-1 (256 x 256), block column j = blockIdx.x: X_ij = -X_ii sum_{k=j}^{i-1} L_ik X_kj for
// i = j + 1 ... in order, the column's finished blocks kept in LDS.  With X_oo the panel below the outer block is ONE product.
__global__ void __launch_bounds__(256) k_chol_xinv(const double* __restrict__ A, int P, int o0, int oe, const double* __restrict__ Linv_all, double* __restrict__ Xo) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef double d4_t __attribute__((ext_vector_type(4)));
    extern __shared__ double cg_chol_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, kq = lane >> 4;
    const int j = blockIdx.x, nblk = (oe - o0) / 64;                   // (launched on full outer blocks only)
    double* Xb = cg_chol_lds;                                          // X_jj, X_{j+1,j}, X_{j+2,j}
    double* W = Xb + 3 * 64 * CG_CHOL_LD;
    const double* Xjj = Linv_all + (size_t)(o0 / CG_CHOL_NB + j) * CG_CHOL_NB * CG_CHOL_NB;
    for (int e = tid; e < 64 * 64; e += 256) Xb[(e >> 6) * CG_CHOL_LD + (e & 63)] = Xjj[e];
    __syncthreads();
    // Round 4, measured and dropped (P = 5907): (1) this kernel folded into the waves k_chol_block's panels and updates leave idle -- 6.85 ms
    // against 6.25: there the operands (L panels, earlier X blocks) cannot be staged (LDS full, 128 registers per lane) and come back from
    // L2 / HBM at ~7 k cycles per dependent round trip, 143 k cycles per outer block; (2) every operand load of the three block rows issued
    // before the first product (144 doubles per lane, 322 registers with the accumulator file): 38.5 us per launch against 37.3.
    for (int i = j + 1; i < nblk; ++i) {
        // one round trip per block row: the rows' L_ik (k = j ... i - 1) and X_ii together
        double av[3][16], xv[16];
        const double* Xii = Linv_all + (size_t)(o0 / CG_CHOL_NB + i) * CG_CHOL_NB * CG_CHOL_NB;
#pragma unroll
        for (int kk = 0; kk < 3; ++kk) {
            const double* pa = A + (size_t)(o0 + 64 * i + 16 * wave + col) * P + o0 + 64 * (j + kk);
#pragma unroll
            for (int ks = 0; ks < 16; ++ks) av[kk][ks] = j + kk < i ? pa[4 * ks + kq] : 0.0;
        }
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) xv[ks] = Xii[(16 * wave + col) * CG_CHOL_NB + 4 * ks + kq];
#pragma unroll
        for (int c = 0; c < 4; ++c) {                                   // W = sum_k L_ik X_kj, rows 16 wave ...
            d4_t acc = {0, 0, 0, 0};
#pragma unroll
            for (int kk = 0; kk < 3; ++kk) {
                if (j + kk >= i) break;
                const double* Xk = Xb + kk * 64 * CG_CHOL_LD;
#pragma unroll
                for (int ks = 0; ks < 16; ++ks)
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[kk][ks], Xk[(4 * ks + kq) * CG_CHOL_LD + 16 * c + col], acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) W[(16 * wave + kq + 4 * r) * CG_CHOL_LD + 16 * c + col] = acc[r];
        }
        __syncthreads();
        double* Xi = Xb + (i - j) * 64 * CG_CHOL_LD;
#pragma unroll
        for (int c = 0; c < 4; ++c) {                                   // X_ij = -X_ii W
            d4_t acc = {0, 0, 0, 0};
#pragma unroll
            for (int ks = 0; ks < 16; ++ks)
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xv[ks], W[(4 * ks + kq) * CG_CHOL_LD + 16 * c + col], acc, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int lr = 16 * wave + kq + 4 * r, lc = 16 * c + col;
                if (i - j < 3) Xi[lr * CG_CHOL_LD + lc] = -acc[r];
                Xo[(size_t)(64 * i + lr) * CG_CHOL_OUTER + 64 * j + lc] = -acc[r];
            }
        }
        __syncthreads();
    }
#endif
}
// rows [oe + 64 blockIdx.x, +64) of the outer block's column panel in one product, L = A[rows, o0:oe] X_oo^T (X_oo lower triangular:
// output block j sums the input blocks k <= j): the rows' A operands in registers (loaded once, so the in-place store is safe), the
// 64 x 64 blocks of X_oo staged through LDS by the whole workgroup, the next block's loads in flight during the products
__global__ void __launch_bounds__(256) k_chol_trsm(double* __restrict__ A, int P, int o0, int oe, const double* __restrict__ Xo) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef double d4_t __attribute__((ext_vector_type(4)));
    typedef double d2_t __attribute__((ext_vector_type(2)));
    extern __shared__ double cg_chol_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, kq = lane >> 4;
    const int r0 = oe + 64 * blockIdx.x, ra = r0 + 16 * wave + col;
    double av[4][16];
    {
        const double* pa = A + (size_t)min(ra, P - 1) * P + o0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int s = 0; s < 16; ++s) av[k][s] = ra < P ? pa[64 * k + 4 * s + kq] : 0.0;
    }
    // staging: thread -> row tid >> 2 of the block, 16 consecutive doubles from column 16 (tid & 3)
    const int srow = tid >> 2, scol = 16 * (tid & 3);
    d2_t st[8];
    auto fetch = [&](int j, int k) {
        const d2_t* src = (const d2_t*)(Xo + (size_t)(64 * j + srow) * CG_CHOL_OUTER + 64 * k + scol);
#pragma unroll
        for (int u = 0; u < 8; ++u) st[u] = src[u];
    };
    auto stash = [&](double* buf) {
#pragma unroll
        for (int u = 0; u < 8; ++u) { buf[srow * CG_CHOL_LD + scol + 2 * u] = st[u][0]; buf[srow * CG_CHOL_LD + scol + 2 * u + 1] = st[u][1]; }
    };
    int cur = 0;
    fetch(0, 0);
    stash(cg_chol_lds);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        d4_t acc[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = d4_t{0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k <= j; ++k) {
            const bool last = j == 3 && k == 3;
            if (!last) { if (k < j) fetch(j, k + 1); else fetch(j + 1, 0); }          // the next block's loads fly during the products
            const double* Xb = cg_chol_lds + cur * 64 * CG_CHOL_LD;
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int s = 0; s < 16; ++s)                                           // B operand [kk][n] = X[64 j + 16 c + n][64 k + kk]
                    acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[k][s], Xb[(16 * c + col) * CG_CHOL_LD + 4 * s + kq], acc[c], 0, 0, 0);
            if (!last) { stash(cg_chol_lds + (cur ^ 1) * 64 * CG_CHOL_LD); __syncthreads(); cur ^= 1; }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int rr = r0 + 16 * wave + kq + 4 * r;
                if (rr < P) A[(size_t)rr * P + o0 + 64 * j + 16 * c + col] = acc[c][r];
            }
    }
#endif
}
// trailing update of the lower triangle: A[r][c] -= sum_{k in [kb, kb + kl)} A[r][k] A[c][k] for columns c in [cb, ce), rows
// r >= max(c, cb).  One wave per 64 x 64 block (4 x 4 MFMA tiles); MFMA row i of tile a is matrix row 4 i + a (32 contiguous
// bytes of C per lane); a lane holds two K entries per stage (K index 8 h + 2 kq + s: 16 contiguous bytes of each of its 8
// operand rows; KS = 2), stage h + 1 in flight while stage h multiplies; the K = 64 calls are latency-bound and run with KS = 4.  Called with kl = 64 on the rest of a 256-column outer block
// after each 64-column panel and with kl = 256 on everything right of the outer block once it is finished: the trailing
// matrix is read and written once per 256 columns (the K = 64 update of the whole trailing matrix was HBM-bound).
template <int KS, int OCC>
__global__ void __launch_bounds__(256, OCC) k_chol_update(double* __restrict__ A, int P, int kb, int kl, int cb, int ce) {
    typedef double d4_t __attribute__((ext_vector_type(4)));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ti = blockIdx.y, tj = blockIdx.x * 4 + wave;
    const int p0 = cb + 64 * ti, q0 = cb + 64 * tj;
    if (q0 > p0 || q0 >= ce || p0 >= P) return;
    const int col = lane & 15, kq = lane >> 4;
    const int pl = p0 + 4 * col, ql = q0 + 4 * col;
    d4_t acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = d4_t{0, 0, 0, 0};
    if (OCC == 1) {                        // latency-bound calls: C is fetched up front (acc = -C, stored back as -acc)
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int pr = p0 + 4 * (kq + 4 * r) + a;
#pragma unroll
                for (int c = 0; c < 4; ++c) if (pr < P && ql + c <= pr && ql + c < ce) acc[a][c][r] = -A[(size_t)pr * P + ql + c];
            }
    }
    if (p0 + 64 <= P && q0 + 64 <= ce && kl % (4 * KS) == 0) {                 // interior block (wave-uniform; q0 <= p0)
        const double* ra = A + (size_t)pl * P + kb + KS * kq;
        const double* rb = A + (size_t)ql * P + kb + KS * kq;
        double av[KS][4], bv[KS][4], an[KS][4], bn[KS][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int s = 0; s < KS; ++s) { av[s][a] = ra[(size_t)a * P + s]; bv[s][a] = rb[(size_t)a * P + s]; }
        for (int h = 4 * KS; h < kl; h += 4 * KS) {
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int s = 0; s < KS; ++s) { an[s][a] = ra[(size_t)a * P + h + s]; bn[s][a] = rb[(size_t)a * P + h + s]; }
#pragma unroll
            for (int s = 0; s < KS; ++s) CG_MFMA_4X4(acc, av[s], bv[s]);
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int s = 0; s < KS; ++s) { av[s][a] = an[s][a]; bv[s][a] = bn[s][a]; }
        }
#pragma unroll
        for (int s = 0; s < KS; ++s) CG_MFMA_4X4(acc, av[s], bv[s]);
    } else {
        for (int h = 0; h < kl; h += 4) {
            double av[4], bv[4];
            const int k = h + kq;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                av[a] = (k < kl && pl + a < P) ? A[(size_t)(pl + a) * P + kb + k] : 0.0;
                bv[a] = (k < kl && ql + a < ce) ? A[(size_t)(ql + a) * P + kb + k] : 0.0;
            }
            CG_MFMA_4X4(acc, av, bv);
        }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int pr = p0 + 4 * (kq + 4 * r) + a;
            if (pr >= P) continue;
            double* crow = A + (size_t)pr * P;
#pragma unroll
            for (int c = 0; c < 4; ++c) if (ql + c <= pr && ql + c < ce) { if (OCC == 1) crow[ql + c] = -acc[a][c][r]; else crow[ql + c] -= acc[a][c][r]; }
        }
}
// the same update with a 32 x 32 quadrant of the 64 x 64 block per wave (2 x 2 MFMA tiles, one K-stage of 8 in flight, four waves per
// SIMD): for the calls with too few blocks to give every SIMD a 4 x 4-tile wave -- the narrow update of the next outer block's 256
// columns on the dependent chain (a 64 x 64 x 256 block is 27 us of MFMA issue for ONE wave) and the last trailing updates
__global__ void __launch_bounds__(256, 4) k_chol_update_q(double* __restrict__ A, int P, int kb, int kl, int cb, int ce) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef double d4_t __attribute__((ext_vector_type(4)));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, kq = lane >> 4;
    const int pb = cb + 64 * blockIdx.y, qb = cb + 64 * blockIdx.x;
    if (qb > pb || qb >= ce || pb >= P) return;
    const int p0 = pb + 32 * (wave >> 1), q0 = qb + 32 * (wave & 1);
    if (q0 > p0 + 31 || q0 >= ce || p0 >= P) return;                   // (the quadrant above the diagonal of a diagonal block)
    d4_t acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[a][c] = d4_t{0, 0, 0, 0};
    const double* ra[2]; const double* rb[2];          // (P may be odd: 8-byte loads)
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        ra[a] = A + (size_t)min(p0 + 16 * a + col, P - 1) * P + kb + 2 * kq;
        rb[a] = A + (size_t)min(q0 + 16 * a + col, P - 1) * P + kb + 2 * kq;
    }
    double av[2][2], bv[2][2], an[2][2], bn[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int s = 0; s < 2; ++s) { av[a][s] = ra[a][s]; bv[a][s] = rb[a][s]; }
    for (int h = 8; h < kl; h += 8) {                                   // (kl is a multiple of 8: 256, or 64 k)
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int s = 0; s < 2; ++s) { an[a][s] = ra[a][h + s]; bn[a][s] = rb[a][h + s]; }
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int c = 0; c < 2; ++c) acc[a][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a][s], bv[c][s], acc[a][c], 0, 0, 0);
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int s = 0; s < 2; ++s) { av[a][s] = an[a][s]; bv[a][s] = bn[a][s]; }
    }
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int c = 0; c < 2; ++c) acc[a][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a][s], bv[c][s], acc[a][c], 0, 0, 0);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int pr = p0 + 16 * a + kq + 4 * r, qc = q0 + 16 * c + col;
                if (pr < P && qc < ce && qc <= pr) A[(size_t)pr * P + qc] -= acc[a][c][r];
            }
#endif
}
extern "C" {

/* In-place Cholesky factor of a symmetric positive definite matrix: on return the lower triangle of A (P x P, row-major)
 * holds L with A = L L^T (the strict upper triangle is left as it was).  CG_ERR_STATE if A is not positive definite. */
// the factorisation proper on a device matrix; *dinfo (device, zeroed by the caller) receives the first bad pivot + 1
// dinv: (P + 63) / 64 blocks of 64 x 64 doubles, receives the inverses of the diagonal blocks of L
// trailing update of the columns [cb, P) (T row blocks) with the K = kl panel at column kb: a wave per 64 x 64 block when that fills the
// GPU, a wave per quadrant when it does not
static void chol_trailing_update(cg_ctx* c, hipStream_t st, double* dA, int P, int kb, int kl, int cb, int T) {
    static const int qmax = cg_tune::chol_quadrant_blocks();
    if (T * (T + 1) / 2 < qmax) hipLaunchKernelGGL(k_chol_update_q, dim3(T, T), dim3(256), 0, st, dA, P, kb, kl, cb, P);
    else hipLaunchKernelGGL((k_chol_update<2, 2>), dim3((T + 3) / 4, T), dim3(256), 0, st, dA, P, kb, kl, cb, P);
}
// Stream A (the context's stream) carries the dependent chain of an outer block -- k_chol_block, k_chol_xinv, k_chol_trsm and the
// update of the NEXT outer block's 256 columns --, stream B the rest of the trailing update, which the next outer block's chain does
// not need (look-ahead): B waits for A's panel, A waits for B before it touches the columns B was updating.
static int chol_factor_dev(cg_ctx* c, double* dA, int P, int* dinfo, double* dinv, double** Xo_out = nullptr) {
    int rc;
    if ((rc = set_lds(c, k_chol_block, CG_CHOL_BLOCK_LDS)) || (rc = set_lds(c, k_chol_xinv, CG_CHOL_XINV_LDS)) || (rc = set_lds(c, k_chol_trsm, CG_CHOL_TRSM_LDS))) return rc;
    const int nouter = (P + CG_CHOL_OUTER - 1) / CG_CHOL_OUTER;
    double* Xo_all = (double*)arena_take(c, sizeof(double) * (size_t)nouter * CG_CHOL_OUTER * CG_CHOL_OUTER);      // L_oo^-1 of every outer block
    if (Xo_out) *Xo_out = Xo_all;
    if (!Xo_all) CG_FAIL(c, CG_ERR_HIP, "Cholesky: workspace allocation failed");
    const bool ahead = nouter > 2 && !cg_tune::chol_no_lookahead();
    if (ahead && !c->stream2) {
        CG_HIP(c, hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
        CG_HIP(c, hipEventCreateWithFlags(&c->ev_a, hipEventDisableTiming));
        CG_HIP(c, hipEventCreateWithFlags(&c->ev_b, hipEventDisableTiming));
    }
    bool b_busy = false;
    // an early return (a failing event / stream call) must not leave stream B writing into dA behind the caller's back: the next API call
    // resets the arena and reuses it
    struct BGuard { cg_ctx* c; bool* busy; ~BGuard() { if (*busy && c->stream2) (void)hipStreamSynchronize(c->stream2); } } guard{c, &b_busy};
    for (int o0 = 0; o0 < P; o0 += CG_CHOL_OUTER) {
        const int oe = std::min(P, o0 + CG_CHOL_OUTER);
        double* Xo = Xo_all + (size_t)(o0 / CG_CHOL_OUTER) * CG_CHOL_OUTER * CG_CHOL_OUTER;
        hipLaunchKernelGGL(k_chol_block, dim3(1), dim3(cg_tune::chol_block_nt()), CG_CHOL_BLOCK_LDS, c->stream, dA, P, o0, oe, dinfo, dinv, Xo);
        if (oe >= P) break;
        const int T = (P - oe + 63) / 64;
        hipLaunchKernelGGL(k_chol_xinv, dim3(3), dim3(256), CG_CHOL_XINV_LDS, c->stream, (const double*)dA, P, o0, oe, (const double*)dinv, Xo);
        hipLaunchKernelGGL(k_chol_trsm, dim3(T), dim3(256), CG_CHOL_TRSM_LDS, c->stream, dA, P, o0, oe, (const double*)Xo);
        const int ne = std::min(P, oe + CG_CHOL_OUTER);                 // the next outer block's columns [oe, ne)
        if (!ahead || ne >= P) {
            if (b_busy) { CG_HIP(c, hipStreamWaitEvent(c->stream, c->ev_b, 0)); b_busy = false; }
            chol_trailing_update(c, c->stream, dA, P, o0, oe - o0, oe, T);
            continue;
        }
        if (b_busy) CG_HIP(c, hipStreamWaitEvent(c->stream, c->ev_b, 0));     // (B's previous update wrote into [oe, ne) too)
        hipLaunchKernelGGL(k_chol_update_q, dim3(4, T), dim3(256), 0, c->stream, dA, P, o0, oe - o0, oe, ne);
        CG_HIP(c, hipEventRecord(c->ev_a, c->stream));                  // the panel is complete and the narrow update has had the GPU to itself
        CG_HIP(c, hipStreamWaitEvent(c->stream2, c->ev_a, 0));
        const int T2 = (P - ne + 63) / 64;
        chol_trailing_update(c, c->stream2, dA, P, o0, oe - o0, ne, T2);
        CG_HIP(c, hipEventRecord(c->ev_b, c->stream2));
        b_busy = true;
    }
    if (b_busy) { CG_HIP(c, hipStreamWaitEvent(c->stream, c->ev_b, 0)); b_busy = false; }
    CG_HIP(c, hipGetLastError());                                       // a launch that failed on either stream
    return CG_OK;
}
static double* chol_inverse_blocks(cg_ctx* c, int P) {
    return (double*)arena_take(c, sizeof(double) * (size_t)((P + CG_CHOL_NB - 1) / CG_CHOL_NB) * CG_CHOL_NB * CG_CHOL_NB);
}

int cg_cholesky(cg_ctx* c, double* A, int P) {
    if (!c) return CG_ERR_ARG;
    if (!A || P <= 0) CG_FAIL(c, CG_ERR_ARG, "cg_cholesky: bad argument");
    CG_HIP(c, hipSetDevice(c->device));
    int rc;
    if ((rc = arena_reset(c))) CG_FAIL(c, rc, "cg_cholesky: arena");
    Arg aa{A, nullptr, sizeof(double) * (size_t)P * P, true, true};
    if ((rc = stage(c, aa))) return rc;
    int* dinfo = (int*)arena_take(c, sizeof(int));
    double* dinv = chol_inverse_blocks(c, P);
    if (!dinfo || !dinv) CG_FAIL(c, CG_ERR_HIP, "cg_cholesky: workspace allocation failed");
    CG_HIP(c, hipMemsetAsync(dinfo, 0, sizeof(int), c->stream));
    if ((rc = chol_factor_dev(c, (double*)aa.dev, P, dinfo, dinv))) return rc;
    int info = 0;
    CG_HIP(c, hipMemcpyAsync(&info, dinfo, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    CG_HIP(c, hipStreamSynchronize(c->stream));
    if (info != 0) CG_FAIL(c, CG_ERR_STATE, "cg_cholesky: the matrix is not positive definite (pivot %d)", info);
    if ((rc = unstage(c, aa))) return rc;
    return finish(c);
}

// ---- damped SPD solve (src/sr.py:38-41 / 102-112): x = (A + damping I)^-1 b, everything on the device --------------
__global__ void k_add_diag(double* __restrict__ A, int P, double v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < P) A[(size_t)i * P + i] += v;
}
// Triangular solves with the inverse diagonal blocks X_k = L_kk^-1 (k_chol_diag).  y is the running right-hand side, z the
// solution; ONE launch per 64-wide block: every workgroup forms z_k = X_k y_k (lower) or X_k^T y_k (transposed) in LDS,
// workgroup 0 stores it, and the rest of y is updated with it.  y_k itself is not written, so no workgroup races another.
__device__ __forceinline__ void trsv_block_solution(const double* __restrict__ X, const double* __restrict__ y, int k0, int nb, int transposed,
                                                    double* ys, double* zs) {
    const int t = threadIdx.x;
    if (t < CG_CHOL_NB) ys[t] = t < nb ? y[k0 + t] : 0.0;
    __syncthreads();
    const int r = t >> 2, part = t & 3;                                  // 4 threads per entry of z_k
    double a = 0.0;
    if (!transposed) { for (int k = part; k <= r; k += 4) a += X[r * CG_CHOL_NB + k] * ys[k]; }
    else             { for (int k = r + ((part - r) & 3); k < CG_CHOL_NB; k += 4) a += X[k * CG_CHOL_NB + r] * ys[k]; }
    a += __shfl_xor(a, 1); a += __shfl_xor(a, 2);
    if (part == 0) zs[r] = a;
    __syncthreads();
}
// lower: y[i] -= sum_j L[i][k0+j] z[k0+j] for the rows below the block: 16 lanes per row, 32 B per lane
__global__ void __launch_bounds__(256) k_trsv_lower(const double* __restrict__ L, const double* __restrict__ Xall, int P, int k0, int nb,
                                                    double* __restrict__ y, double* __restrict__ z) {
    __shared__ double ys[CG_CHOL_NB], zs[CG_CHOL_NB];
    trsv_block_solution(Xall + (size_t)(k0 / CG_CHOL_NB) * CG_CHOL_NB * CG_CHOL_NB, y, k0, nb, 0, ys, zs);
    if (blockIdx.x == 0 && threadIdx.x < nb) z[k0 + threadIdx.x] = zs[threadIdx.x];
    const int sub = threadIdx.x & 15, row = k0 + nb + blockIdx.x * 16 + (threadIdx.x >> 4);
    double acc = 0.0;
    if (row < P) {
        const double* r = L + (size_t)row * P + k0;
#pragma unroll
        for (int u = 0; u < 4; ++u) { const int j = 4 * sub + u; if (j < nb) acc += r[j] * zs[j]; }
    }
    acc += __shfl_xor(acc, 1); acc += __shfl_xor(acc, 2); acc += __shfl_xor(acc, 4); acc += __shfl_xor(acc, 8);
    if (row < P && sub == 0) y[row] -= acc;
}
// transposed: y[i] -= sum_j L[k0+j][i] z[k0+j] for the entries before the block: one thread per i, coalesced over i
__global__ void __launch_bounds__(256) k_trsv_upper(const double* __restrict__ L, const double* __restrict__ Xall, int P, int k0, int nb,
                                                    double* __restrict__ y, double* __restrict__ z) {
    __shared__ double ys[CG_CHOL_NB], zs[CG_CHOL_NB];
    trsv_block_solution(Xall + (size_t)(k0 / CG_CHOL_NB) * CG_CHOL_NB * CG_CHOL_NB, y, k0, nb, 1, ys, zs);
    if (blockIdx.x == 0 && threadIdx.x < nb) z[k0 + threadIdx.x] = zs[threadIdx.x];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= k0) return;
    double acc = 0.0;
    for (int j = 0; j < nb; ++j) acc += L[(size_t)(k0 + j) * P + i] * zs[j];
    y[i] -= acc;
}

// ---- 256-wide substitution steps with X_oo = L_oo^-1 of the outer blocks (k_chol_block / k_chol_xinv): two launches per 256 columns
// instead of four one-launch 64-column steps.  z_K = X_oo y_K (or X_oo^T y_K) by four workgroups, then the rest of y by many.
__global__ void __launch_bounds__(1024) k_trsv_z256(const double* __restrict__ X, const double* __restrict__ y, double* __restrict__ z, int transposed) {
    __shared__ double ys[256], part[16][64];
    const int t = threadIdx.x, g = blockIdx.x;          // four workgroups, 64 entries of z each: 16 loads per thread, one round trip
    if (t < 256) ys[t] = y[t];
    __syncthreads();
    if (!transposed) {                      // 16 lanes per row: z[r] = sum_{c <= r} X[r][c] y[c]
        const int sub = t & 15, r = 64 * g + (t >> 4);
        const double* xr = X + (size_t)r * 256;
        double a = 0.0;
#pragma unroll
        for (int m = 0; m < 16; ++m) { const int c = 16 * m + sub; if (c <= r) a += xr[c] * ys[c]; }
        a += __shfl_xor(a, 1); a += __shfl_xor(a, 2); a += __shfl_xor(a, 4); a += __shfl_xor(a, 8);
        if (sub == 0) z[r] = a;
    } else {                                // thread (c, part): z[c] = sum_{r >= c} X[r][c] y[r], r = part mod 16
        const int cl = t & 63, c = 64 * g + cl, pt = t >> 6;
        double a = 0.0;
#pragma unroll
        for (int m = 0; m < 16; ++m) { const int r = pt + 16 * m; if (r >= c) a += X[(size_t)r * 256 + c] * ys[r]; }
        part[pt][cl] = a;
        __syncthreads();
        if (t < 64) {
            double v = 0.0;
#pragma unroll
            for (int q = 0; q < 16; ++q) v += part[q][t];
            z[64 * g + t] = v;
        }
    }
}
// y[row] -= sum_{j < 256} L[row][k0 + j] z[k0 + j] for the rows from k0 + 256: 16 lanes per row, 128-byte segments
__global__ void __launch_bounds__(256) k_trsv_lower256(const double* __restrict__ L, int P, int k0, double* __restrict__ y, const double* __restrict__ z) {
    __shared__ double zs[256];
    zs[threadIdx.x] = z[k0 + threadIdx.x];
    __syncthreads();
    const int sub = threadIdx.x & 15, row = k0 + 256 + blockIdx.x * 16 + (threadIdx.x >> 4);
    double acc = 0.0;
    if (row < P) {
        const double* r = L + (size_t)row * P + k0;
#pragma unroll
        for (int u = 0; u < 16; ++u) acc += r[16 * u + sub] * zs[16 * u + sub];
    }
    acc += __shfl_xor(acc, 1); acc += __shfl_xor(acc, 2); acc += __shfl_xor(acc, 4); acc += __shfl_xor(acc, 8);
    if (row < P && sub == 0) y[row] -= acc;
}
// transposed: y[i] -= sum_{j < 256} L[k0 + j][i] x[k0 + j] for i < k0: 64 entries per workgroup, the 256 rows split over the four waves
__global__ void __launch_bounds__(256) k_trsv_upper256(const double* __restrict__ L, int P, int k0, double* __restrict__ y, const double* __restrict__ x) {
    __shared__ double xs[256], part[4][64];
    xs[threadIdx.x] = x[k0 + threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = blockIdx.x * 64 + lane;
    double acc = 0.0;
    if (i < k0) {
        const double* col = L + (size_t)(k0 + 64 * wave) * P + i;
#pragma unroll 16
        for (int j = 0; j < 64; ++j) acc += col[(size_t)j * P] * xs[64 * wave + j];
    }
    part[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && i < k0) y[i] -= part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane];
}

// A -= u u^T + v v^T (centring of the quantum Fisher matrix, src/sr.py:88: Re(conj(m) m^T) with m = u + i v)
__global__ void __launch_bounds__(256) k_rank2_downdate(double* __restrict__ A, int P, const double* __restrict__ u, const double* __restrict__ v) {
    const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (j < P) A[(size_t)i * P + j] -= u[i] * u[j] + v[i] * v[j];
}

int cg_spd_solve(cg_ctx* c, double* A, int P, double damping, const double* center_re, const double* center_im,
                 const double* b, double* x) {
    if (!c) return CG_ERR_ARG;
    if (!A || !b || !x || P <= 0) CG_FAIL(c, CG_ERR_ARG, "cg_spd_solve: bad argument");
    CG_HIP(c, hipSetDevice(c->device));
    int rc;
    if ((rc = arena_reset(c))) CG_FAIL(c, rc, "cg_spd_solve: arena");
    Arg aa{A, nullptr, sizeof(double) * (size_t)P * P, true, false};       // host mode: the caller's matrix is left intact
    Arg ax{x, nullptr, sizeof(double) * (size_t)P, false, true};
    Arg au{(void*)center_re, nullptr, sizeof(double) * (size_t)P, true, false}, av{(void*)center_im, nullptr, sizeof(double) * (size_t)P, true, false};
    if ((center_re == nullptr) != (center_im == nullptr)) CG_FAIL(c, CG_ERR_ARG, "cg_spd_solve: centre needs both parts");
    if ((rc = stage(c, aa)) || (rc = stage(c, ax)) || (rc = stage(c, au)) || (rc = stage(c, av))) return rc;
    int* dinfo = (int*)arena_take(c, sizeof(int));
    double* dinv = chol_inverse_blocks(c, P);
    double* z = (double*)arena_take(c, sizeof(double) * (size_t)P);
    if (!dinfo || !dinv || !z) CG_FAIL(c, CG_ERR_HIP, "cg_spd_solve: workspace allocation failed");
    CG_HIP(c, hipMemsetAsync(dinfo, 0, sizeof(int), c->stream));
    double* dA = (double*)aa.dev; double* y = (double*)ax.dev;
    CG_HIP(c, hipMemcpyAsync(y, b, sizeof(double) * (size_t)P, hipMemcpyDefault, c->stream));
    if (center_re) hipLaunchKernelGGL(k_rank2_downdate, dim3((P + 255) / 256, P), dim3(256), 0, c->stream, dA, P, (const double*)au.dev, (const double*)av.dev);
    if (damping != 0.0) hipLaunchKernelGGL(k_add_diag, dim3((P + 255) / 256), dim3(256), 0, c->stream, dA, P, damping);
    double* Xo = nullptr;
    if ((rc = chol_factor_dev(c, dA, P, dinfo, dinv, &Xo))) return rc;
    // substitutions: 256 columns at a time with X_oo where an outer block is followed by rows (every outer block but the last),
    // 64 columns at a time with the inverse diagonal blocks in the last one.  (A failed factorisation leaves NaNs: reported below.)
    const int last0 = ((P - 1) / CG_CHOL_OUTER) * CG_CHOL_OUTER;
    for (int o0 = 0; o0 < last0; o0 += CG_CHOL_OUTER) {                    // L z = b   (y: running right-hand side)
        const double* X = Xo + (size_t)(o0 / CG_CHOL_OUTER) * CG_CHOL_OUTER * CG_CHOL_OUTER;
        hipLaunchKernelGGL(k_trsv_z256, dim3(4), dim3(1024), 0, c->stream, X, (const double*)(y + o0), z + o0, 0);
        hipLaunchKernelGGL(k_trsv_lower256, dim3((P - o0 - CG_CHOL_OUTER + 15) / 16), dim3(256), 0, c->stream, (const double*)dA, P, o0, y, (const double*)z);
    }
    for (int k0 = last0; k0 < P; k0 += CG_CHOL_NB) {
        const int nb = std::min(CG_CHOL_NB, P - k0), m = P - k0 - nb;
        hipLaunchKernelGGL(k_trsv_lower, dim3(std::max(1, (m + 15) / 16)), dim3(256), 0, c->stream, (const double*)dA, (const double*)dinv, P, k0, nb, y, z);
    }
    for (int k0 = ((P - 1) / CG_CHOL_NB) * CG_CHOL_NB; k0 >= last0; k0 -= CG_CHOL_NB) {   // L^T x = z, x into y's storage
        const int nb = std::min(CG_CHOL_NB, P - k0);
        hipLaunchKernelGGL(k_trsv_upper, dim3(std::max(1, (k0 + 255) / 256)), dim3(256), 0, c->stream, (const double*)dA, (const double*)dinv, P, k0, nb, z, y);
    }
    for (int o0 = last0 - CG_CHOL_OUTER; o0 >= 0; o0 -= CG_CHOL_OUTER) {
        const double* X = Xo + (size_t)(o0 / CG_CHOL_OUTER) * CG_CHOL_OUTER * CG_CHOL_OUTER;
        hipLaunchKernelGGL(k_trsv_z256, dim3(4), dim3(1024), 0, c->stream, X, (const double*)(z + o0), y + o0, 1);
        if (o0 > 0) hipLaunchKernelGGL(k_trsv_upper256, dim3((o0 + 63) / 64), dim3(256), 0, c->stream, (const double*)dA, P, o0, z, (const double*)y);
    }
    int info = 0;
    CG_HIP(c, hipMemcpyAsync(&info, dinfo, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    CG_HIP(c, hipStreamSynchronize(c->stream));
    if (info != 0) CG_FAIL(c, CG_ERR_STATE, "cg_spd_solve: the matrix is not positive definite (pivot %d)", info);
    if ((rc = unstage(c, ax))) return rc;
    return finish(c);
}

/* device-pointer form without an arena reset (callers that hold arena workspace) */
int cg_fisher_real_nr(cg_ctx* c, const double* S_dev, int B, int P, double* F_dev) {
    return fisher_real_launch(c, S_dev, B, P, F_dev);
}
int cg_fisher_real(cg_ctx* c, const double* S, int B, int P, double* F) {
    if (!c) return CG_ERR_ARG;
    if (!S || !F || B <= 0 || P <= 0) CG_FAIL(c, CG_ERR_ARG, "cg_fisher_real: bad argument");
    CG_HIP(c, hipSetDevice(c->device));
    int rc;
    if ((rc = arena_reset(c))) CG_FAIL(c, rc, "cg_fisher_real: arena");
    Arg as{(void*)S, nullptr, sizeof(double) * (size_t)B * P, true, false};
    Arg af{F, nullptr, sizeof(double) * (size_t)P * P, false, true};
    if ((rc = stage(c, as)) || (rc = stage(c, af))) return rc;
    if ((rc = fisher_real_launch(c, (const double*)as.dev, B, P, (double*)af.dev))) return rc;
    if ((rc = unstage(c, af))) return rc;
    return finish(c);
}

}  // extern "C"
