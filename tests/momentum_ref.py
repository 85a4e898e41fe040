"""tests/momentum_ref.py -- TEST INFRASTRUCTURE ONLY.
numpy restatement of the momentum-distribution reduction (coulombgas_amd/csrc/cg_momentum.hpp) and of the displaced ratios of a
plane-wave determinant (theta = 0: the identity flow), shared by tests/test_momentum_host.py and tests/test_gpu_momentum.py.

  n_k^(b) = (1/S) sum_{m < S n} e^{-2 pi i k.s_{b,m}} r_b(m),  m = j n + i; a term whose ratio is not finite adds nothing and is counted.
  packed: [0, 2 nK) sum_b n_k^(b) as (re, im); [2 nK, 3 nK) sum_b (Re n_k^(b))^2; [3 nK] dropped; [3 nK + 1] B."""
import numpy as np


def per_walker(ratios, shifts, K):
    """n_k^(b) (B, nK) complex and the dropped terms per walker (B,).  ratios (B, S, n) complex, shifts (B, S, n, dim), K (nK, dim)"""
    ratios = np.asarray(ratios)
    B, S, n = ratios.shape
    K = np.asarray(K, dtype=np.float64)
    r = ratios.reshape(B, S * n)
    s = np.asarray(shifts, dtype=np.float64).reshape(B, S * n, -1)
    bad = ~(np.isfinite(r.real) & np.isfinite(r.imag))
    with np.errstate(invalid="ignore"):
        ph = np.exp(-2j * np.pi * np.einsum("bmd,kd->bmk", s, K))
        term = np.where(bad[:, :, None], 0.0, ph * np.where(bad, 0.0, r)[:, :, None])
    return term.sum(1) / S, bad.sum(1)


def momentum_ref(ratios, shifts, K):
    """the packed vector of cg_momentum_sums"""
    nk, dropped = per_walker(ratios, shifts, K)
    nK = nk.shape[1]
    out = np.zeros(3 * nK + 2)
    out[0:2 * nK:2] = nk.real.sum(0)
    out[1:2 * nK:2] = nk.imag.sum(0)
    out[2 * nK:3 * nK] = (nk.real ** 2).sum(0)
    out[3 * nK] = dropped.sum()
    out[3 * nK + 1] = nk.shape[0]
    return out


def slater(x, kocc, L):
    """A[b, i, j] = exp(2 pi i k_{b,j}.x_{b,i} / L): the plane-wave Slater matrix (src/slater.py:14 without the constant L^{-n d / 2})"""
    return np.exp(2j * np.pi / L * np.einsum("bid,bjd->bij", x, kocc))


def planewave_ratios(x, kocc, L, shifts):
    """Psi(x with row i moved by s L) / Psi(x) for Psi = det A: moving row i multiplies A[i, j] by e^{2 pi i k_j.s}, so the ratio is
    sum_j e^{2 pi i k_j.s} A[i, j] (A^-1)[j, i].  x (B, n, dim), kocc (B, n, dim) in units of 2 pi / L, shifts (B, S, n, dim) -> (B, S, n)"""
    A = slater(np.asarray(x, dtype=np.float64), kocc, L)
    Ainv = np.linalg.inv(A)
    w = A * np.swapaxes(Ainv, 1, 2)                                              # w[b, i, j] = A[i, j] Ainv[j, i]
    ph = np.exp(2j * np.pi * np.einsum("bsid,bjd->bsij", np.asarray(shifts, dtype=np.float64), kocc))
    return np.einsum("bsij,bij->bsi", ph, w)


def occupation(K, kocc, tol=1e-9):
    """occ[b, k] = 1 if K[k] is one of walker b's occupied orbitals"""
    d = np.abs(np.asarray(K)[None, :, None, :] - np.asarray(kocc)[:, None, :, :]).max(-1)
    return (d < tol).any(-1).astype(np.float64)


def regular_grid(G, dim):
    """the G^dim displacements (a_1, ..., a_dim) / G"""
    ax = np.arange(G) / G
    return np.stack(np.meshgrid(*([ax] * dim), indexing="ij"), -1).reshape(-1, dim)


def grid_size(K, kocc):
    """smallest G that exceeds every |component difference| between a requested k and an occupied orbital (the differences are integers
    when k and the orbitals carry the same twist): on the regular G^dim grid the estimator is then exact for the identity flow"""
    return int(np.rint(np.abs(np.asarray(K)[None, :, None, :] - np.asarray(kocc)[:, None, :, :]).max())) + 1


def metropolis_planewave(rng, x, kocc, L, steps, stddev):
    """all-particle Metropolis moves on |det A|^2 (src/MCMC.py:22-39 in numpy), every walker its own chain"""
    x = np.array(x, dtype=np.float64)
    lp = 2.0 * np.linalg.slogdet(slater(x, kocc, L))[1]
    acc = 0
    for _ in range(steps):
        xp = x + stddev * rng.standard_normal(x.shape)
        lpp = 2.0 * np.linalg.slogdet(slater(xp, kocc, L))[1]
        ok = rng.uniform(size=x.shape[0]) < np.exp(np.minimum(lpp - lp, 0.0))
        x[ok], lp[ok] = xp[ok], lpp[ok]
        acc += ok.sum()
    return x, acc / (steps * x.shape[0])
