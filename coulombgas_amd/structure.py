"""Structure observables of the sampled gas: the static structure factor S(k) = <|rho_k|^2> / n and the pair correlation
function g(r), accumulated on the device over sampling calls and ranks (cg_structure_sums; csrc/cg_structure.hpp).

The reference reports the energy and entropy moments only (src/VMC.py:44-53); these two have no counterpart there.  The
walkers never visit the host: each batch adds one packed vector of sums -- |rho_k|^2, rho_k, pair counts per radial bin,
number of walkers -- to an accumulator in HBM, and `result()` brings back that one vector (3 nK + nbins + 2 doubles)."""
import itertools
import math
import numpy as np
from .comm import get_comm

_IDS = itertools.count(1)


class StructureObservable:
    """see make_structure_observable"""

    def __init__(self, n, dim, L, K, nbins=128, rmax=0.5, comm=None, engine=None):
        self.n, self.dim, self.L = int(n), int(dim), float(L)
        self.K = np.ascontiguousarray(K, dtype=np.int64).reshape(-1, self.dim)
        self.nbins, self.rmax = int(nbins), float(rmax)
        if self.K.shape[0] < 1 or self.nbins < 1 or not (0.0 < self.rmax <= 0.5):
            raise ValueError("make_structure_observable: need at least one k vector, nbins >= 1 and 0 < rmax <= 0.5 (units of L)")
        self.comm, self.engine = comm, engine
        self.size = 3 * self.K.shape[0] + self.nbins + 2
        self._tag = "structure_acc_%d" % next(_IDS)
        self._acc, self._empty = None, True

    def _engine_of(self, x):
        if self.engine is None:
            if hasattr(x, "eng"):
                self.engine = x.eng
            else:
                from .flow import get_engine
                self.engine = get_engine(self.n, self.dim, 2, 16, 16, self.L)
        elif hasattr(x, "eng") and x.eng is not self.engine:
            raise ValueError("structure observable: the walkers live on another engine than the accumulator")
        return self.engine

    def accumulate(self, x):
        """adds one batch x (B, n, dim), a numpy array or a DeviceArray (then nothing crosses to the host)"""
        eng = self._engine_of(x)
        if tuple(np.shape(x)[-2:]) != (self.n, self.dim):
            raise ValueError("x must have trailing shape (%d,%d), got %s" % (self.n, self.dim, np.shape(x)))
        eng.set_structure(self.K, self.nbins, self.rmax)
        x_d = x if hasattr(x, "ptr") else eng.asdevice(np.asarray(x, dtype=np.float64).reshape(-1, self.n, self.dim), "structure_x")
        if self._acc is None:
            self._acc = eng.scratch(self._tag, (self.size,))
        out = eng.structure_sums_d(x_d)
        eng.axpby_d(1.0, out, 0.0 if self._empty else 1.0, self._acc, count=self.size)      # the first batch overwrites: no memset
        self._empty = False
        return self

    def reset(self):
        self._empty = True
        return self

    def sums(self):
        """the accumulated packed vector, summed over the ranks (one all-reduce, one download); the accumulator is left as it is"""
        if self._empty:
            raise RuntimeError("structure observable: nothing accumulated")
        eng, cm = self.engine, self.comm or get_comm()
        tmp = eng.scratch("structure_result", (self.size,))
        eng.axpby_d(1.0, self._acc, 0.0, tmp, count=self.size)
        cm.psum_d(tmp, count=self.size)
        return np.asarray(eng.to_host(tmp), dtype=np.float64)

    def result(self):
        """dict: k (nK, dim) = 2 pi K / L; S = sum |rho_k|^2 / (n count); rho = sum rho_k / count (complex); S_connected = S - |rho|^2 / n;
        r (bin centres, units of L's length); g = hist L^dim / (count n(n-1)/2 V_b) with V_b the volume of shell b of width rmax L / nbins
        (annulus in 2-D, spherical shell in 3-D), -> 1 for uncorrelated uniform particles; hist, overflow, count."""
        h = self.sums()
        n, dim, L, nK, nb = self.n, self.dim, self.L, self.K.shape[0], self.nbins
        count = float(h[-1])
        S = h[:nK] / (n * count)
        rho = (h[nK:3 * nK:2] + 1j * h[nK + 1:3 * nK:2]) / count
        hist, overflow = h[3 * nK:3 * nK + nb].copy(), float(h[3 * nK + nb])
        edges = self.rmax * L * np.arange(nb + 1) / nb
        shell = math.pi * np.diff(edges ** 2) if dim == 2 else 4.0 * math.pi / 3.0 * np.diff(edges ** 3)
        pairs = count * n * (n - 1) / 2.0
        g = hist * L ** dim / (pairs * shell) if pairs > 0 else np.zeros(nb)
        return {"k": 2.0 * math.pi * self.K / L, "S": S, "rho": rho, "S_connected": S - np.abs(rho) ** 2 / n,
                "r": 0.5 * (edges[1:] + edges[:-1]), "g": g, "hist": hist, "overflow": overflow, "count": count}


def make_structure_observable(n, dim, L, K, nbins=128, rmax=0.5, comm=None, engine=None):
    """Accumulator of S(k) and g(r) for n particles in a box L^dim.  K: (nK, dim) integer vectors (k = 2 pi K / L; K = 0 allowed),
    e.g. kpoints(dim, Gmax); nbins radial bins on [0, rmax L), rmax <= 0.5 so that every shell lies inside the nearest-image cell.
    engine: the Engine whose GPU holds the accumulator (default: the engine of the first DeviceArray accumulated, else the process's
    engine for (n, dim, L)); comm: the communicator `result()` sums over (default: get_comm()).
    Returns an object with accumulate(x), reset(), result()."""
    return StructureObservable(n, dim, L, K, nbins, rmax, comm, engine)
