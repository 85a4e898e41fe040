"""The rarely taken branch of the wave-level LUs -- the full pivot search behind the threshold test -- and the determinism of the
single-wave sampler.

The register-resident factorisations of the n <= 16 sampler (csrc/cg_linalg.hpp) take the first unfinished row as the pivot of a column
unless a live candidate is more than 4x larger (16x in squared modulus for the complex Slater matrix); only then the full search runs.
The benchmark inputs (a flow near the identity) never leave the short path, so this file feeds the three routines inputs on which the
search does run, in the real factorisation and in the complex one:

  n = 13, 16   cg_wave_lu2_both<26, 13> / <32, 16>                       (both matrices in one instruction stream)
  n = 12       cg_wave_lu2_logabsdet<32> + cg_wave_lu2_logdet_complex<16>  (the separate single-wave routines)

each with the (2, 16, 16) flow, eight walkers, 64 threads.  THAT the search runs is established by replaying the threshold rule in numpy
(threshold_lu_replay below: the device algorithm column by column, the same pivot choice including the comparison of the candidates by
the high word of their modulus) on J from cg_flow_jacobian and on the Slater matrix built from cg_flow_forward's z: the search must
fire in at least one real and one complex column step for at least half of the walkers.

CASES records the seed and weight scale of each n.  They were picked on the CPU with the C oracle's J and z alone: the weight scale
1.5 is the one at which tests/test_gpu_configs.py sees row exchanges in every LU, and already the first seed tried, 0, meets the
condition above on the oracle's matrices (6, 7 and 7 of the 8 walkers at n = 12, 13, 16); test_reference_inputs_take_the_search
re-checks that without a GPU.

Checks: log phi, 1/2 log|det J|, log p and a 6-step chain with supplied draws against oracle/cg_oracle.c, with the tolerances
tests/test_gpu_configs.py uses for its wave-level-LU shapes at the weight scale 1.5 (1e-9 relative; chain positions 1e-12).
Every figure is printed before it is asserted (pytest -s).

Determinism (n = 13): the same chain call twice, and once more as two half-batch calls with walker_offset: walkers and log p bitwise
equal."""
import ctypes as C

import numpy as np
import pytest

from tests.common import orbitals, box_length, flow_theta, state_indices, walkers

DIM, HS, HT, B = 2, 16, 16, 8
# n: (seed, weight scale), chosen with the oracle alone (see the module docstring)
CASES = {12: (0, 1.5), 13: (0, 1.5), 16: (0, 1.5)}
CHAIN_STEPS, CHAIN_STD = 6, 0.1

_ORACLE = None
_REF = {}


def _c_oracle():
    global _ORACLE
    if _ORACLE is None:
        from coulombgas_amd.build import build_oracle
        _ORACLE = C.CDLL(build_oracle())
        _ORACLE.cgo_mcmc.restype = C.c_double
    return _ORACLE


def _p(a):
    return np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)


def _check(what, err, bound):
    print("  %-34s %.3e (bound %.3e)" % (what, err, bound))
    assert err < bound, (what, err, bound)


def _high_word(v):
    return (np.ascontiguousarray(v, dtype=np.float64).view(np.uint64) >> np.uint64(32)).astype(np.int64)


def threshold_lu_replay(A, factor):
    """Column steps of the wave-level LU on one matrix (real or complex): the pivot of column k is the first unfinished row unless
    a live candidate's size is more than `factor` times larger -- size = |a| (real, factor 4) or |a|^2 (complex, factor 16) -- and then
    the live row whose size has the largest high word (the first such row).  Rows never move.  -> (steps at which the search ran,
    log|det|)."""
    A = np.array(A)
    n = A.shape[0]
    live = np.ones(n, bool)
    fired, logdet = [], 0.0
    for k in range(n):
        col = A[:, k]
        size = np.abs(col) if np.isrealobj(A) else col.real * col.real + col.imag * col.imag
        p = int(np.flatnonzero(live)[0])
        if (live & (size * (1.0 / factor) > size[p])).any():
            fired.append(k)
            key = np.where(live, _high_word(size) + 1, 0)
            p = int(np.flatnonzero(key == key.max())[0])
        logdet += np.log(np.abs(A[p, k]))
        live[p] = False
        mult = np.where(live, col / A[p, k], 0.0)
        A = A - np.outer(mult, A[p])
    return fired, logdet


def slater(z, sp, sidx, L):
    """D_ij = exp(i k_j . z_i), k_j = 2 pi / L sp[sidx[j]]"""
    k = 2.0 * np.pi / L * sp[sidx]
    return np.exp(1j * (z @ k.T))


def searches(J, z, sp, sidx, L):
    """-> per walker: (real column steps with a search, complex column steps with a search)"""
    out = []
    for w in range(J.shape[0]):
        fr, ld = threshold_lu_replay(J[w], 4.0)
        assert abs(ld - np.linalg.slogdet(J[w])[1]) < 1e-8 * max(1.0, abs(ld))          # the replay is an LU of this matrix
        fc, _ = threshold_lu_replay(slater(z[w], sp, sidx[w], L), 16.0)
        out.append((len(fr), len(fc)))
    return out


def _reference(n):
    """inputs of case n and everything the oracle says about them, computed once per session"""
    if n not in _REF:
        seed, ws = CASES[n]
        L, sp = box_length(n, DIM), orbitals(DIM, 25)
        rng = np.random.default_rng(seed)
        theta = flow_theta(rng, 2, HS, HT, DIM, ws, 0.1)
        x = walkers(rng, B, n, DIM, L)
        sidx = state_indices(rng, B, n, sp.shape[0])
        noise = rng.standard_normal((CHAIN_STEPS, B, n, DIM)); unif = rng.uniform(size=(CHAIN_STEPS, B))
        lib = _c_oracle()
        N = n * DIM
        out = np.zeros((B, 3)); zr = np.zeros((B, n, DIM)); Jr = np.zeros((B, N, N))
        lib.cgo_logpsi(n, DIM, 2, HS, HT, C.c_double(L), _p(theta), _p(sp), sp.shape[0], _p(sidx), _p(x), B, _p(out))
        lib.cgo_flow(n, DIM, 2, HS, HT, C.c_double(L), _p(theta), _p(x), B, _p(zr), _p(Jr))
        xc = x.copy(); lpc = np.zeros(B)
        rate = lib.cgo_mcmc(n, DIM, 2, HS, HT, C.c_double(L), _p(theta), _p(sp), sp.shape[0], _p(sidx), _p(xc), B, CHAIN_STEPS,
                            C.c_double(CHAIN_STD), _p(noise), _p(unif), _p(lpc))
        _REF[n] = dict(L=L, sp=sp, theta=theta, x=x, sidx=sidx, noise=noise, unif=unif, out=out, z=zr, J=Jr, chain_x=xc, chain_lp=lpc,
                       chain_rate=rate)
        for v in _REF[n].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _REF[n]


def _engine(n, r):
    from coulombgas_amd.engine import Engine
    eng = Engine(n, DIM, 2, HS, HT, r["L"], r["sp"])
    eng.set_params(r["theta"])
    info = eng.launch_info()
    assert info["threads"] == 64 and info["fast"] == 1, info
    return eng


def _assert_search_runs(tag, cnt):
    both = sum(1 for a, c in cnt if a >= 1 and c >= 1)
    print("  %s: column steps with a full search per walker (real, complex): %s -> %d of %d walkers with both" % (tag, cnt, both, len(cnt)))
    assert 2 * both >= len(cnt), (tag, cnt)


@pytest.mark.parametrize("n", sorted(CASES))
def test_reference_inputs_take_the_search(n):
    """the recorded seed and scale meet the condition on the oracle's matrices alone (no GPU)"""
    r = _reference(n)
    _assert_search_runs("oracle n=%d" % n, searches(r["J"], r["z"], r["sp"], r["sidx"], r["L"]))


@pytest.mark.gpu
@pytest.mark.parametrize("n", sorted(CASES))
def test_full_search_against_c_oracle(n):
    r = _reference(n)
    L, sp, x, sidx, out = r["L"], r["sp"], r["x"], r["sidx"], r["out"]
    N = n * DIM
    eng = _engine(n, r)
    print("n = %d, seed %d, weight scale %.1f" % ((n,) + CASES[n]))
    # the search runs on the matrices the device factorises
    z = eng.flow_forward(x)
    J = np.asarray(eng.flow_jacobian(x)).reshape(B, N, N)
    _check("flow", np.abs(z - r["z"]).max(), 1e-12 * max(1.0, np.abs(r["z"]).max()))
    _check("Jacobian", np.abs(J - r["J"]).max(), 1e-12 * max(1.0, np.abs(r["J"]).max()))
    _assert_search_runs("device n=%d" % n, searches(J, z, sp, sidx, L))
    # log phi, 1/2 log|det J|, log p
    tol = 1e-9
    lphi, hld = eng.logphi_logjacdet(x, sidx)
    b_re, b_h = tol * np.abs(out[:, 0]).max(), tol * max(1.0, np.abs(out[:, 2]).max())
    _check("Re log phi", np.abs(lphi[:, 0] - out[:, 0]).max(), b_re)
    _check("Im log phi (mod 2 pi)", np.abs(np.angle(np.exp(1j * (lphi[:, 1] - out[:, 1])))).max(), tol)
    _check("1/2 log|det J|", np.abs(hld - out[:, 2]).max(), b_h)
    _check("log p", np.abs(eng.logp(x, sidx) - 2.0 * (out[:, 0] + out[:, 2])).max(), 2.0 * (b_re + b_h))      # log p = 2 (Re log phi + 1/2 log|det J|)
    # 6 steps with supplied draws
    xg, lpg, nacc = eng.mcmc(x, sidx, CHAIN_STEPS, CHAIN_STD, noise=r["noise"], unif=r["unif"])
    print("  accepted %d of %d (oracle rate %.4f)" % (nacc, CHAIN_STEPS * B, r["chain_rate"]))
    assert nacc / (CHAIN_STEPS * B) == pytest.approx(r["chain_rate"], abs=1e-15)
    _check("chain positions", np.abs(xg - r["chain_x"]).max(), 1e-12)
    _check("chain log p against the oracle", np.abs(lpg - r["chain_lp"]).max(), tol * max(1.0, np.abs(r["chain_lp"]).max()))
    _check("chain log p against the log Psi kernel", np.abs(lpg - eng.logp(xg, sidx)).max(), tol * max(1.0, np.abs(lpg).max()))
    eng.close()


@pytest.mark.gpu
def test_single_wave_chain_is_deterministic():
    """n = 13: the same call twice, and split into two half-batch calls with walker_offset -- bitwise the same walkers and log p"""
    n = 13
    r = _reference(n)
    eng = _engine(n, r)
    x, sidx, noise, unif = r["x"], r["sidx"], r["noise"], r["unif"]
    x1, lp1, n1 = eng.mcmc(x, sidx, CHAIN_STEPS, CHAIN_STD, noise=noise, unif=unif)
    x2, lp2, n2 = eng.mcmc(x, sidx, CHAIN_STEPS, CHAIN_STD, noise=noise, unif=unif)
    assert np.isfinite(x1).all() and np.isfinite(lp1).all()
    assert x1.tobytes() == x2.tobytes() and lp1.tobytes() == lp2.tobytes() and n1 == n2
    h = B // 2
    xa, lpa, na = eng.mcmc(x[:h], sidx[:h], CHAIN_STEPS, CHAIN_STD, walker_offset=0, noise=noise[:, :h], unif=unif[:, :h])
    xb, lpb, nb = eng.mcmc(x[h:], sidx[h:], CHAIN_STEPS, CHAIN_STD, walker_offset=h, noise=noise[:, h:], unif=unif[:, h:])
    assert np.concatenate([xa, xb]).tobytes() == x1.tobytes()
    assert np.concatenate([lpa, lpb]).tobytes() == lp1.tobytes()
    assert na + nb == n1
    eng.close()
