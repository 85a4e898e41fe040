"""tests/structure_ref.py -- TEST INFRASTRUCTURE ONLY.
numpy restatement of the structure observables (coulombgas_amd/csrc/cg_structure.hpp), shared by tests/test_structure_host.py and
tests/test_gpu_structure.py: rho_k = sum_i exp(2 pi i k.x_i / L); every pair i < j: r~ = (x_i - x_j)/L - rint(.), d = |r~|,
t = d * (nbins / rmax), bin (int)t if t < nbins else the overflow bin nbins."""
import numpy as np

# the three shapes the issue fixes, (n, dim, B, L), and their seed
SHAPES = ((13, 2, 256, 6.39), (57, 2, 64, 13.38), (14, 3, 64, 3.9))
SEED = 20261017


def seeded_walkers(n, dim, B, L, seed=SEED):
    return np.random.default_rng(seed).uniform(-0.5 * L, 1.5 * L, (B, n, dim))


def kgrid(dim):
    """kpoints(dim, Gmax) with k = 0 prepended; Gmax 15 in 2-D, 7 in 3-D"""
    from coulombgas_amd.potential import kpoints
    return np.concatenate([np.zeros((1, dim), dtype=np.int64), kpoints(dim, 15 if dim == 2 else 7).astype(np.int64)])


def pair_t(x, L, nbins, rmax):
    """t (B, n(n-1)/2) of every pair"""
    x = np.asarray(x, dtype=np.float64)
    i, j = np.triu_indices(x.shape[1], 1)
    with np.errstate(invalid="ignore"):
        r = (x[:, i] - x[:, j]) / L
        r = r - np.rint(r)
        return np.sqrt((r * r).sum(-1)) * (nbins / rmax)


def edge_gap(t):
    """smallest distance of a finite t to an integer (a bin edge)"""
    t = t[np.isfinite(t)]
    return float(np.abs(t - np.round(t)).min()) if t.size else np.inf


def structure_ref(x, L, K, nbins, rmax, chunk=64):
    """the packed vector of cg_structure_sums: [nK |rho|^2] [2 nK (re, im)] [nbins + 1 counts] [B]"""
    x = np.asarray(x, dtype=np.float64)
    K = np.asarray(K, dtype=np.int64)
    B, n, dim = x.shape
    nK = K.shape[0]
    out = np.zeros(3 * nK + nbins + 2)
    u = x / L
    with np.errstate(invalid="ignore"):
        u = u - np.floor(u)                                   # integer k: the phase only sees x modulo L
        for b0 in range(0, B, chunk):
            ph = 2.0 * np.pi * np.einsum("bnd,kd->bkn", u[b0:b0 + chunk], K.astype(np.float64))
            rho = (np.cos(ph) + 1j * np.sin(ph)).sum(-1)      # (chunk, nK)
            out[:nK] += (rho.real ** 2 + rho.imag ** 2).sum(0)
            out[nK:3 * nK:2] += rho.real.sum(0)
            out[nK + 1:3 * nK:2] += rho.imag.sum(0)
        t = pair_t(x, L, nbins, rmax)
        bins = np.where(t < nbins, t, nbins).astype(np.int64)
    out[3 * nK:3 * nK + nbins + 1] = np.bincount(bins.ravel(), minlength=nbins + 1)
    out[-1] = B
    return out
