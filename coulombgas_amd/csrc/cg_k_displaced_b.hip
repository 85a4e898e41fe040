// cg_k_displaced_b.hip -- displaced-ratio kernels (momentum distribution) of the remaining (dim, spsize, tpsize) instantiations.
#include "cg_host.hpp"
#include "cg_rng.hpp"

#define CG_UNIT_DISPLACED
#define CG_UNIT_CONFIGS(X) CG_FAST_CONFIGS_B(X)
#define CG_UNIT_SPECIALS(X)
#define CG_UNIT_NAME(f) cg_sampler_b_##f
#include "cg_k_sampler.inc"
