"""Momentum distribution n(k) of the sampled gas from displaced wave-function ratios, accumulated on the device over sampling
calls and ranks (cg_momentum_sums; csrc/cg_momentum.hpp, k_displaced_ratios in csrc/cg_k_sampler.inc).

The reference reports the energy and entropy moments only (src/VMC.py:44-53); n(k) has no counterpart there.  It is the Fourier
transform of the one-body density matrix: for walkers (state_idx_b, x_b) ~ p(K) |Psi_K(x)|^2, k in units of 2 pi / L and
displacements s in units of L,

    n_k^(b) = (1/S) sum_{j < S} sum_{i < n} e^{-2 pi i k.s_{b,j,i}} Psi_K(x_b with row i moved by s_{b,j,i} L) / Psi_K(x_b),
    n_k     = mean over b of n_k^(b),

with S uniform displacements per particle drawn in the kernel (Philox).  Every displacement costs a full log Psi evaluation (the
backflow moves every quasi-particle), so a batch costs S n sampler steps per walker; neither the displaced configurations nor the
ratios leave HBM: each batch adds one packed vector of 3 nK + 2 sums to an accumulator there, and `result()` brings back that vector."""
import itertools
import math
import numpy as np
from .comm import get_comm

_IDS = itertools.count(1)


class MomentumObservable:
    """see make_momentum_observable"""

    def __init__(self, n, dim, L, K, shifts_per_particle=1, seed=0, comm=None, engine=None):
        self.n, self.dim, self.L = int(n), int(dim), float(L)
        self.K = np.ascontiguousarray(K, dtype=np.float64).reshape(-1, self.dim)
        self.S, self.seed = int(shifts_per_particle), int(seed) & (2 ** 64 - 1)
        if self.K.shape[0] < 1 or self.S < 1 or not np.isfinite(self.K).all():
            raise ValueError("make_momentum_observable: need at least one finite k vector and shifts_per_particle >= 1")
        self.comm, self.engine = comm, engine
        self.size = 3 * self.K.shape[0] + 2
        self._tag = "momentum_acc_%d" % next(_IDS)
        self._acc, self._empty = None, True
        self.offset = 0           # walkers seen so far: the Philox stream of the next batch starts behind them

    def _engine_of(self, x):
        if self.engine is None:
            if hasattr(x, "eng"):
                self.engine = x.eng
            else:
                raise ValueError("momentum observable: host walkers need engine= (the Engine whose flow parameters and orbital table define Psi)")
        elif hasattr(x, "eng") and x.eng is not self.engine:
            raise ValueError("momentum observable: the walkers live on another engine than the accumulator")
        return self.engine

    def accumulate(self, x, state_idx):
        """adds one batch: x (B, n, dim) and state_idx (B, n), numpy arrays or DeviceArrays (then nothing crosses to the host).  Psi is
        evaluated with the flow parameters currently bound to the engine.  Each call draws fresh displacements: the Philox walker
        offset advances by B (ranks are kept apart by rank * 2^40)."""
        eng = self._engine_of(x)
        if tuple(np.shape(x)[-2:]) != (self.n, self.dim):
            raise ValueError("x must have trailing shape (%d,%d), got %s" % (self.n, self.dim, np.shape(x)))
        x_d = x if hasattr(x, "ptr") else eng.asdevice(np.asarray(x, dtype=np.float64).reshape(-1, self.n, self.dim), "momentum_x")
        B = int(x_d.shape[0])
        if int(np.prod(np.shape(state_idx))) != B * self.n:
            raise ValueError("state_idx must have shape (%d,%d), got %s" % (B, self.n, np.shape(state_idx)))
        s_d = state_idx if hasattr(state_idx, "ptr") else eng.asdevice(np.asarray(state_idx).reshape(B, self.n), "momentum_sidx", np.int32)
        eng.set_momentum(self.K)
        if self._acc is None:
            self._acc = eng.scratch(self._tag, (self.size,))
        cm = self.comm or get_comm()
        out = eng.momentum_sums_d(x_d, s_d, self.S, seed=self.seed, walker_offset=(int(getattr(cm, "rank", 0)) << 40) + self.offset)
        eng.axpby_d(1.0, out, 0.0 if self._empty else 1.0, self._acc, count=self.size)      # the first batch overwrites: no memset
        self._empty = False
        self.offset += B
        return self

    def reset(self):
        """forgets the accumulated sums (the Philox offset keeps advancing: a later batch never reuses displacements)"""
        self._empty = True
        return self

    def sums(self):
        """the accumulated packed vector, summed over the ranks (one all-reduce, one download); the accumulator is left as it is"""
        if self._empty:
            raise RuntimeError("momentum observable: nothing accumulated")
        eng, cm = self.engine, self.comm or get_comm()
        tmp = eng.scratch("momentum_result", (self.size,))
        eng.axpby_d(1.0, self._acc, 0.0, tmp, count=self.size)
        cm.psum_d(tmp, count=self.size)
        return np.asarray(eng.to_host(tmp), dtype=np.float64)

    def result(self):
        """dict: k (nK, dim) = 2 pi K / L; n_k = Re sum_b n_k^(b) / count; n_k_imag the imaginary part (zero within noise);
        stderr = sqrt((sum_b (Re n_k^(b))^2 / count - n_k^2) / (count - 1)), the standard error of n_k over the walkers; dropped: terms
        left out because their ratio was not finite; count: walkers summed."""
        h = self.sums()
        nK = self.K.shape[0]
        count = float(h[-1])
        nk = h[0:2 * nK:2] / count
        var = np.maximum(h[2 * nK:3 * nK] / count - nk * nk, 0.0)
        return {"k": 2.0 * math.pi * self.K / self.L, "n_k": nk, "n_k_imag": h[1:2 * nK:2] / count,
                "stderr": np.sqrt(var / (count - 1.0)) if count > 1 else np.full(nK, np.inf), "dropped": float(h[3 * nK]), "count": count}


def make_momentum_observable(n, dim, L, K, shifts_per_particle=1, seed=0, comm=None, engine=None):
    """Accumulator of the momentum distribution n(k) for n particles in a box L^dim.  K: (nK, dim) real vectors in units of 2 pi / L,
    e.g. the (twisted) orbital table itself: k and the orbitals then carry the same twist and n_k is the occupation of orbital k
    (1 or 0 per walker for the identity flow).  shifts_per_particle: S uniform displacements per particle and walker, S n log Psi
    evaluations per walker; seed: of the in-kernel Philox stream.  engine: the Engine that holds Psi (flow.engine(n, dim, sp_indices);
    default: the engine of the first DeviceArray accumulated); comm: the communicator `result()` sums over (default: get_comm()).
    Returns an object with accumulate(x, state_idx), reset(), result()."""
    return MomentumObservable(n, dim, L, K, shifts_per_particle, seed, comm, engine)
