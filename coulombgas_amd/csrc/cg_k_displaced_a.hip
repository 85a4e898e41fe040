// cg_k_displaced_a.hip -- displaced-ratio kernels (momentum distribution) of the (2, 16, 16) flow: the instantiations of k_mcmc in
// cg_k_sampler_a.hip, in a translation unit of their own (they cost as much to compile as the chain kernels).  Entry point: cg_k_sampler_a.hip.
#include "cg_host.hpp"
#include "cg_rng.hpp"

#define CG_UNIT_DISPLACED
#define CG_UNIT_CONFIGS(X) CG_FAST_CONFIGS_A(X)
#define CG_UNIT_SPECIALS(X) CG_MCMC_SPECIALS(X)
#define CG_UNIT_NAME(f) cg_sampler_a_##f
#include "cg_k_sampler.inc"
