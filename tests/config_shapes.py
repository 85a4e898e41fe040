"""The shapes of the GPU tests of the second translation unit's flow configurations (csrc/cg_dispatch.hpp: CG_FAST_CONFIGS_B), and the
kernel path each of them takes.

A path is described per kernel FAMILY by a signature string computed by tests/host_emul/cg_pathmap.cpp from the project's layout
functions:

  S    sampler (log Psi, flow, Jacobian, Metropolis chain, displaced ratios): "<threads>:<LU branch>:w<wave_lu>d<dual>j<Dm == J>u<U != J>"
       LU branch: wave-both<26,13> / wave-both<32,16> (cg_wave_lu2_both), wave-two-phase, dual2 (cg_blocked_lu_dual2),
       dual (cg_blocked_lu_dual), sequential (cg_blocked_lu_logabsdet, then cg_blocked_lu_logdet_complex)
  L0, L1, L2   grad / Laplacian in mode 0 (exact), 1 (Hutchinson), 2 (Hutchinson, split): "lds" (k_grad_lap2<AL = true>) or
       "ws<threads>:<P_lds><A_lds><B_lds>" (k_grad_lap2<AL = false>: the blocks that are not in LDS live in the HBM workspace)
  Q    per-sample scores: "k_scores", or "vjp256" / "vjp512w1" / "vjp512w4" (k_param_vjp, threads and waves per SIMD) +
       ":da<vjp_da>i<inverses in LDS>s<panels staged in LDS>"

SHAPES maps (dim, spsize, tpsize, n) to the families that shape stands for, each with the signature recorded when the shape was chosen.
tests/test_path_coverage.py (CPU) asserts that the recorded signatures are still the computed ones and that every signature any of these
configurations takes at any n of the fast path has a shape here; tests/test_gpu_configs.py runs the shapes.  Shapes were chosen as the
smallest n of each signature, one n serving as many families as it can; the entries marked "+" are there in addition (the last n of
the fast path of each configuration, closed shells in three dimensions, ragged last panels).
"""
import ctypes as C

import numpy as np

FAMILIES = ("S", "L0", "L1", "L2", "Q")
LU_BRANCH = ("wave-both<26,13>", "wave-two-phase", "dual2", "dual", "sequential", "wave-both<32,16>")
SCORE_KERNEL = ("k_scores", "vjp256", "vjp512w1", "vjp512w4")
_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        from coulombgas_amd.build import build_pathmap
        _LIB = C.CDLL(build_pathmap())
    return _LIB


def unit_b_configs():
    """the (dim, spsize, tpsize) of CG_FAST_CONFIGS_B, read from the header through the path map"""
    buf = (C.c_int * 96)()
    k = _lib().cg_pathmap_unit_b(buf, 32)
    assert 0 < k <= 32
    return [tuple(buf[3 * i:3 * i + 3]) for i in range(k)]


def paths(dim, hs, ht, n):
    """-> dict(threads, fast, S, L0, L1, L2, Q) of the configuration at n particles"""
    out = (C.c_int * _lib().cg_pathmap_fields())()
    rc = _lib().cg_pathmap(dim, hs, ht, n, out)
    assert rc == 0, "cg_pathmap(%d, %d, %d, %d) -> %d" % (dim, hs, ht, n, rc)
    o = list(out)
    p = dict(threads=o[0], fast=o[1])
    p["S"] = "%d:%s:w%dd%dj%du%d" % (o[0], LU_BRANCH[o[6]], o[2], o[3], o[4], o[5])
    for m in range(3):
        q = o[7 + 5 * m:12 + 5 * m]
        p["L%d" % m] = "lds" if q[0] else "ws%d:%d%d%d" % (q[1], q[2], q[3], q[4])
    s = o[22:26]
    p["Q"] = SCORE_KERNEL[s[0]] if s[0] == 0 else "%s:da%di%ds%d" % (SCORE_KERNEL[s[0]], s[1], s[2], s[3])
    return p


def last_fast_n(dim, hs, ht, limit=4096):
    """largest n of the LDS-resident path (cg_create sends larger systems to the general path)"""
    n = 0
    while n < limit and paths(dim, hs, ht, n + 1)["fast"]:
        n += 1
    return n


SHAPES = {
    # (3, 16, 16): fast path up to n = 38
    (3, 16, 16, 5): {"S": "64:wave-two-phase:w1d0j0u1", "L0": "lds", "L1": "lds", "L2": "lds", "Q": "vjp256:da1i1s0"},
    (3, 16, 16, 9): {"L0": "ws256:111", "L1": "ws256:111", "L2": "ws256:111", "Q": "k_scores"},
    (3, 16, 16, 10): {"S": "64:wave-two-phase:w1d0j0u0"},
    (3, 16, 16, 11): {"S": "64:sequential:w0d1j0u0"},
    (3, 16, 16, 15): {"L1": "ws256:110"},
    (3, 16, 16, 16): {"S": "64:sequential:w0d1j0u0", "L0": "ws256:110", "L1": "ws256:100", "L2": "ws256:110", "Q": "vjp256:da0i1s0"},    # +
    (3, 16, 16, 17): {"S": "128:sequential:w0d1j0u0", "L0": "ws256:100", "L2": "ws256:100"},
    (3, 16, 16, 22): {"Q": "vjp512w1:da1i1s0"},
    (3, 16, 16, 23): {"S": "256:dual:w0d1j0u0", "L0": "ws512:100", "L1": "ws512:100", "L2": "ws512:100", "Q": "vjp512w1:da0i1s0"},
    (3, 16, 16, 24): {"S": "256:dual2:w0d1j0u0"},
    (3, 16, 16, 27): {"S": "256:dual:w0d1j0u0"},    # +
    (3, 16, 16, 33): {"S": "256:dual:w0d1j0u0", "L1": "ws512:000", "Q": "vjp512w4:da0i0s1"},    # +
    (3, 16, 16, 38): {"S": "256:dual2:w0d1j0u0"},    # +
    # (2, 4, 4): fast path up to n = 63
    (2, 4, 4, 1): {"S": "64:sequential:w0d0j0u1"},
    (2, 4, 4, 13): {"S": "64:wave-both<26,13>:w1d0j0u0", "L0": "lds", "L1": "lds", "L2": "lds", "Q": "vjp256:da1i1s0"},
    (2, 4, 4, 15): {"S": "64:wave-two-phase:w1d0j0u0"},
    (2, 4, 4, 16): {"S": "64:wave-both<32,16>:w1d0j0u0"},
    (2, 4, 4, 17): {"S": "128:sequential:w0d1j0u0"},
    (2, 4, 4, 19): {"Q": "vjp256:da0i1s0"},
    (2, 4, 4, 23): {"S": "256:dual2:w0d1j0u0", "L0": "ws256:111", "L1": "ws256:111", "L2": "ws256:111", "Q": "vjp512w1:da1i1s0"},
    (2, 4, 4, 25): {"L1": "ws256:101"},
    (2, 4, 4, 27): {"S": "256:sequential:w0d0j1u0", "L0": "ws256:101", "L1": "ws256:100", "L2": "ws256:101"},
    (2, 4, 4, 30): {"L0": "ws256:100", "L2": "ws256:100"},
    (2, 4, 4, 35): {"Q": "vjp512w1:da0i1s0"},
    (2, 4, 4, 41): {"S": "512:sequential:w0d0j1u0", "L0": "ws512:100", "L1": "ws512:100", "L2": "ws512:100", "Q": "vjp512w4:da0i0s1"},
    (2, 4, 4, 63): {"S": "512:sequential:w0d0j1u0", "L1": "ws512:000"},    # +
    # (3, 4, 4): fast path up to n = 42
    (3, 4, 4, 1): {"S": "64:sequential:w0d0j0u1"},
    (3, 4, 4, 10): {"S": "64:wave-two-phase:w1d0j0u0", "L0": "lds", "L1": "lds", "L2": "lds", "Q": "vjp256:da1i1s0"},
    (3, 4, 4, 11): {"S": "64:sequential:w0d1j0u0"},
    (3, 4, 4, 17): {"S": "128:sequential:w0d1j0u0"},
    (3, 4, 4, 18): {"L0": "ws256:111", "L1": "ws256:111", "L2": "ws256:111", "Q": "vjp256:da0i1s0"},
    (3, 4, 4, 19): {"L0": "ws256:101", "L1": "ws256:100", "L2": "ws256:101"},
    (3, 4, 4, 20): {"L0": "ws256:100", "L2": "ws256:100"},
    (3, 4, 4, 23): {"S": "256:dual:w0d1j0u0", "L0": "ws512:100", "L1": "ws512:100", "L2": "ws512:100", "Q": "vjp512w1:da1i1s0"},
    (3, 4, 4, 24): {"S": "256:dual2:w0d1j0u0"},
    (3, 4, 4, 26): {"Q": "vjp512w1:da0i1s0"},
    (3, 4, 4, 39): {"S": "256:dual:w0d1j0u0", "L1": "ws512:000", "Q": "vjp512w4:da0i0s1"},    # +
    (3, 4, 4, 40): {"S": "256:sequential:w0d0j1u0"},
    (3, 4, 4, 41): {"S": "512:sequential:w0d0j1u0"},
    (3, 4, 4, 42): {"S": "512:sequential:w0d0j1u0"},    # +
    # (2, 8, 8): fast path up to n = 60
    (2, 8, 8, 1): {"S": "64:sequential:w0d0j0u1"},
    (2, 8, 8, 3): {"S": "64:wave-two-phase:w1d0j0u1"},
    (2, 8, 8, 13): {"S": "64:wave-both<26,13>:w1d0j0u0", "L0": "lds", "L1": "lds", "L2": "lds", "Q": "vjp256:da1i1s0"},
    (2, 8, 8, 15): {"S": "64:wave-two-phase:w1d0j0u0"},
    (2, 8, 8, 16): {"S": "64:wave-both<32,16>:w1d0j0u0"},
    (2, 8, 8, 17): {"S": "128:sequential:w0d1j0u0", "L0": "ws256:111", "L1": "ws256:111", "L2": "ws256:111", "Q": "vjp256:da0i1s0"},
    (2, 8, 8, 23): {"S": "256:dual2:w0d1j0u0"},
    (2, 8, 8, 24): {"L0": "ws256:101", "L1": "ws256:101", "L2": "ws256:101", "Q": "vjp512w1:da1i1s0"},
    (2, 8, 8, 27): {"L0": "ws256:100", "L1": "ws256:100", "L2": "ws256:100"},
    (2, 8, 8, 33): {"Q": "vjp512w1:da0i1s0"},
    (2, 8, 8, 41): {"S": "512:dual2:w0d1j0u0", "L0": "ws512:100", "L1": "ws512:100", "L2": "ws512:100", "Q": "vjp512w4:da0i0s1"},
    (2, 8, 8, 43): {"S": "512:sequential:w0d0j1u0"},
    (2, 8, 8, 60): {"S": "512:sequential:w0d0j1u0", "L1": "ws512:000"},    # +
    # (3, 8, 8): fast path up to n = 40
    (3, 8, 8, 2): {"S": "64:wave-two-phase:w1d0j0u1"},
    (3, 8, 8, 10): {"S": "64:wave-two-phase:w1d0j0u0", "L0": "lds", "L1": "lds", "L2": "lds", "Q": "vjp256:da1i1s0"},
    (3, 8, 8, 11): {"S": "64:sequential:w0d1j0u0", "L1": "ws256:111"},
    (3, 8, 8, 17): {"S": "128:sequential:w0d1j0u0", "L0": "ws256:111", "L1": "ws256:110", "L2": "ws256:111", "Q": "vjp256:da0i1s0"},
    (3, 8, 8, 18): {"L0": "ws256:101", "L1": "ws256:100", "L2": "ws256:101"},
    (3, 8, 8, 19): {"L0": "ws256:100", "L2": "ws256:100"},
    (3, 8, 8, 23): {"S": "256:dual:w0d1j0u0", "L0": "ws512:100", "L1": "ws512:100", "L2": "ws512:100", "Q": "vjp512w1:da1i1s0"},
    (3, 8, 8, 24): {"S": "256:dual2:w0d1j0u0"},
    (3, 8, 8, 25): {"Q": "vjp512w1:da0i1s0"},
    (3, 8, 8, 33): {"S": "256:dual:w0d1j0u0", "L1": "ws512:000", "Q": "vjp512w4:da0i0s1"},    # +
    (3, 8, 8, 40): {"S": "256:dual2:w0d1j0u0"},    # +
    # (2, 32, 32): fast path up to n = 43
    (2, 32, 32, 5): {"L0": "lds", "L1": "lds", "L2": "lds", "Q": "vjp256:da1i1s0"},
    (2, 32, 32, 13): {"S": "64:wave-both<26,13>:w1d0j0u1", "L0": "ws256:111", "L1": "ws256:111", "L2": "ws256:111", "Q": "vjp256:da0i1s0"},
    (2, 32, 32, 15): {"S": "64:wave-two-phase:w1d0j0u1", "L1": "ws256:110"},
    (2, 32, 32, 16): {"S": "64:wave-both<32,16>:w1d0j0u0"},
    (2, 32, 32, 17): {"S": "128:sequential:w0d1j0u0", "L0": "ws256:101", "L2": "ws256:101"},
    (2, 32, 32, 23): {"S": "256:dual2:w0d1j0u0", "L0": "ws256:100", "L1": "ws256:100", "L2": "ws256:100", "Q": "vjp512w1:da1i1s0"},
    (2, 32, 32, 25): {"Q": "vjp512w1:da0i1s0"},
    (2, 32, 32, 41): {"S": "512:dual2:w0d1j0u0", "L0": "ws512:100", "L1": "ws512:100", "L2": "ws512:100", "Q": "vjp512w4:da0i0s1"},
    (2, 32, 32, 43): {"S": "512:dual2:w0d1j0u0"},    # +
}


def shapes_of(family):
    """[(dim, hs, ht, n)] of the shapes that stand for a signature of this family, sorted"""
    return sorted(k for k, v in SHAPES.items() if family in v)


DERIV_WS = 0.3          # weight scale of the derivative-family inputs (a flow near the identity; the sampler family also runs 1.5)
EXACT_GOLDEN = "golden_configs_exact.npz"     # tests/golden: one walker per exact-mode shape above n = 7 (make_golden_vectors.py --configs-exact)
EXACT_LIVE_MAX_N = 7    # up to here the exact mode is compared with the oracle at test time (seconds); above it the oracle takes too long


def key_of(shape):
    return "d%d_s%d_t%d_n%d" % shape


def inputs(shape, B, ws):
    """seeded inputs of a shape from the package's generators: dict(L, sp, theta, x, sidx, rng)"""
    from tests.common import orbitals, box_length, flow_theta, state_indices, walkers
    dim, hs, ht, n = shape
    L = box_length(n, dim)
    sp = orbitals(dim, 49 if dim == 2 and n > 40 else 25)
    rng = np.random.default_rng(1000 * n + 10 * dim + hs)
    theta = flow_theta(rng, 2, hs, ht, dim, ws, 0.1)
    x = walkers(rng, B, n, dim, L)
    sidx = state_indices(rng, B, n, sp.shape[0])
    return dict(L=L, sp=sp, theta=theta, x=x, sidx=sidx, rng=rng)
