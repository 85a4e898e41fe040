// cg_dispatch.hpp -- compile-time (dim, spsize, tpsize) instantiations of the depth-2 fast path.
#pragma once
#include <type_traits>
// X(D, HS, HT)
#if defined(CG_ONLY_2_16_16)      /* diagnostic builds: one configuration, a fifth of the compile time */
#define CG_FAST_CONFIGS(X) X(2, 16, 16)
#elif defined(CG_ONLY_3_4_4)
#define CG_FAST_CONFIGS(X) X(3, 4, 4)
#else
// two groups = two translation units per kernel family (compiled in parallel): A is the shape of every shipped run
#define CG_FAST_CONFIGS_A(X) X(2, 16, 16)
#define CG_FAST_CONFIGS_B(X) X(3, 16, 16) X(2, 4, 4) X(3, 4, 4) X(2, 8, 8) X(3, 8, 8) X(2, 32, 32)
#define CG_FAST_CONFIGS(X) CG_FAST_CONFIGS_A(X) CG_FAST_CONFIGS_B(X)
#endif
#if !defined(CG_FAST_CONFIGS_A)
#define CG_FAST_CONFIGS_A(X) CG_FAST_CONFIGS(X)
#define CG_FAST_CONFIGS_B(X)
#endif

// Sampler kernels additionally specialised on the particle number and the workgroup size: X(D, HS, HT, N, THREADS).
// With n a compile-time constant every LDS offset, trip count and tile count of the chain folds away (the runtime-n
// kernel keeps ~100 scalar registers of layout state alive across the Metropolis loop and spills them).
#if defined(CG_NO_SPECIALS) || defined(CG_ONLY_3_4_4)
#define CG_MCMC_SPECIALS(X)
#else
#define CG_MCMC_SPECIALS(X) X(2, 16, 16, 13, 64) X(2, 16, 16, 29, 256) X(2, 16, 16, 49, 512) X(2, 16, 16, 57, 512)     /* the sizes of the reference's production runs (data/n_29, n_49, n_57) and of its n = 13 benchmark */
#endif

// The lists as types, and the run-time -> compile-time step of every launch function: cg_with_config<List>(dim, hs, ht, f) calls the generic
// lambda f with the entry of List that matches as an (empty) object -- constexpr int D = cfg.D, HS = cfg.HS, HT = cfg.HT; -- and returns what
// it returns, or 0 when the list has no such entry (the convention of the launch functions: 1 launched, 0 not in this unit, < 0 error).
template <int D_, int HS_, int HT_, int N_ = 0, int NT_ = 0>
struct CgCfg { static constexpr int D = D_, HS = HS_, HT = HT_, N = N_, NT = NT_; };
template <class... C> struct CgCfgList {};
#define CG_CFG_ENTRY(...) , CgCfg<__VA_ARGS__>
#define CG_CFG_LIST(LIST) CgCfgList<void LIST(CG_CFG_ENTRY)>        /* (void: the head that the leading commas hang on) */
typedef CG_CFG_LIST(CG_FAST_CONFIGS) CgFastConfigs;

template <class... C, class F>
static inline int cg_with_entry(CgCfgList<void, C...>, int dim, int hs, int ht, int n, int nt, F&& f) {
    int r = 0;
    (void)(... || (dim == C::D && hs == C::HS && ht == C::HT && n == C::N && nt == C::NT && ((r = f(C{})), true)));
    return r;
}
template <class List, class F>
static inline int cg_with_config(int dim, int hs, int ht, F&& f) { return cg_with_entry(List{}, dim, hs, ht, 0, 0, f); }
// the same over a list of X(D, HS, HT, N, THREADS): the entry specialised on this particle number and workgroup size (cfg.N, cfg.NT)
template <class List, class F>
static inline int cg_with_special(int dim, int hs, int ht, int n, int nt, F&& f) { return cg_with_entry(List{}, dim, hs, ht, n, nt, f); }

// Kernels instantiated for a few workgroup sizes NTS...: f is called with the size that serves the run-time thread count nt, as a
// std::integral_constant.  cg_with_nt_upto: the first listed size >= nt (the workgroup may be smaller than the instantiation's bound),
// cg_with_nt_equal: the listed size == nt (the kernel runs with exactly that many threads); both: the last one when none matches.
template <bool EQUAL, int NT0, int... NTS, class F>
static inline int cg_with_nt(int nt, F&& f) {
    if constexpr (sizeof...(NTS) == 0) return f(std::integral_constant<int, NT0>{});
    else return (EQUAL ? nt == NT0 : nt <= NT0) ? f(std::integral_constant<int, NT0>{}) : cg_with_nt<EQUAL, NTS...>(nt, f);
}
template <int... NTS, class F> static inline int cg_with_nt_upto(int nt, F&& f) { return cg_with_nt<false, NTS...>(nt, f); }
template <int... NTS, class F> static inline int cg_with_nt_equal(int nt, F&& f) { return cg_with_nt<true, NTS...>(nt, f); }

static inline bool cg_fast_supported(int depth, int dim, int hs, int ht) {
    return depth == 2 && cg_with_config<CgFastConfigs>(dim, hs, ht, [](auto) { return 1; }) == 1;
}
