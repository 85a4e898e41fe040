"""Momentum distribution without a GPU: (i) the reduction of csrc/cg_momentum.hpp compiled for the host (tests/host_emul/
cg_momentum_emul.cpp, the 1-thread CgBlk shim) against the numpy restatement (tests/momentum_ref.py), (ii) the host logic of
coulombgas_amd.momentum against a stand-in engine, (iii) the known answers of the estimator for the identity flow, computed from
plane-wave determinants in numpy: exact occupations on the regular shift grid, and the statistical bound of the GPU test."""
import ctypes as C
import inspect
import math
import os
import subprocess

import numpy as np
import pytest

from tests import momentum_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- (i) device arithmetic on the host shim -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    src = os.path.join(ROOT, "tests", "host_emul", "cg_momentum_emul.cpp")
    out = str(tmp_path_factory.mktemp("momentum_emul") / "libcg_momentum_emul.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", out, src])
    lib = C.CDLL(out)
    lib.emu_momentum_sums.restype = C.c_int
    lib.emu_momentum_sums.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    return lib


def _emul_sums(lib, ratios, shifts, K):
    B, S, n = ratios.shape
    dim = K.shape[1]
    r2 = np.ascontiguousarray(np.stack([ratios.real, ratios.imag], -1), dtype=np.float64)
    sh = np.ascontiguousarray(shifts, dtype=np.float64)
    K = np.ascontiguousarray(K, dtype=np.float64)
    out = np.full(3 * K.shape[0] + 2, np.nan)
    assert lib.emu_momentum_sums(n, dim, K.ctypes.data, K.shape[0], r2.ctypes.data, sh.ctypes.data, B, S, out.ctypes.data) == 0
    return out


def _synthetic(rng, B, S, n, dim, bad=()):
    """ratios of magnitude ~1 (what |Psi'/Psi| is on average under |Psi|^2), uniform shifts; `bad`: (walker, term, value) entries"""
    ratios = rng.standard_normal((B, S, n)) + 1j * rng.standard_normal((B, S, n))
    shifts = rng.uniform(size=(B, S, n, dim))
    for b, m, v in bad:
        ratios.reshape(B, -1)[b, m] = v
    return ratios, shifts


@pytest.mark.parametrize("n,dim,B,S", [(5, 2, 5, 3), (13, 2, 1024, 2), (7, 3, 1500, 1)])
def test_device_arithmetic_on_the_host(emul, n, dim, B, S):
    """the sums to 1e-12 n B (a walker's n_k is a sum of S n terms of magnitude ~1 divided by S: ~n); dropped and count exactly; rows:
    B = 5 (one walker per row), 1024 (the row count itself), 1500 (476 rows hold two walkers)"""
    rng = np.random.default_rng(B)
    K = rng.integers(-4, 5, (37, dim)) + 0.25
    bad = [(0, 1, np.nan), (B - 1, S * n - 1, complex(np.inf, 0.0)), (B // 2, 0, complex(1.0, -np.inf)), (B // 2, 2, complex(np.nan, np.nan))]
    ratios, shifts = _synthetic(rng, B, S, n, dim, bad)
    ref, got = MR.momentum_ref(ratios, shifts, K), _emul_sums(emul, ratios, shifts, K)
    nK = K.shape[0]
    err = np.abs(got[:3 * nK] - ref[:3 * nK]).max()
    print("n=%d dim=%d B=%d S=%d: max |sums - numpy| = %.3e (bound %.3e)" % (n, dim, B, S, err, 1e-12 * n * B))
    assert err <= 1e-12 * n * B
    assert got[3 * nK] == ref[3 * nK] == 4 and got[3 * nK + 1] == B
    assert np.isfinite(got).all()
    # the row rule itself: rows of min(B, 1024) walkers r, r + R, ... summed in ascending order, then 16 row groups, ascending
    nk, _ = MR.per_walker(ratios, shifts, K)
    R = min(B, 1024)
    rows = np.zeros((R, nK))
    for b in range(B):                       # ascending b visits every row's walkers in ascending order
        rows[b % R] += nk[b].real
    groups = np.zeros((16, nK))
    for r in range(R):
        groups[r % 16] += rows[r]
    total = groups[0].copy()
    for g in range(1, 16):
        total += groups[g]
    # numpy's per-walker values differ from the shim's in the last bits (another sincos), so this is a tolerance, 100 times tighter than
    # the bound above; bit equality of the rule is what the GPU test checks between launches
    assert np.abs(got[0:2 * nK:2] - total).max() <= 1e-14 * n * B


def test_empty_batch_and_all_dropped_on_the_host(emul):
    K = np.array([[0.25, 0.25], [1.25, -0.75]])
    ratios, shifts = _synthetic(np.random.default_rng(1), 3, 2, 5, 2)
    assert np.array_equal(_emul_sums(emul, ratios[:0], shifts[:0], K), np.zeros(8))
    ratios[1] = np.nan
    got = _emul_sums(emul, ratios, shifts, K)
    assert got[6] == 10 and got[7] == 3 and np.isfinite(got).all()
    assert np.array_equal(got, _emul_sums(emul, ratios, shifts, K))
    keep = MR.momentum_ref(ratios[[0, 2]], shifts[[0, 2]], K)
    assert np.abs(got[:6] - keep[:6]).max() <= 1e-12 * 5 * 3


# ---- (ii) host logic against a stand-in engine ------------------------------------------------------------------------------------
class _Arr:
    def __init__(self, a, eng=None):
        self.a, self.ptr, self.shape = np.array(a), id(self), np.shape(a)
        if eng is not None:
            self.eng = eng


class _StandInEngine:
    """fills the packed vector from the numpy restatement with plane-wave ratios (theta = 0) and shifts drawn from (seed, offset)"""
    def __init__(self, L, table):
        self.L, self.table, self.pool, self.calls, self.offsets = L, table, {}, [], []

    def set_momentum(self, K):
        self.K = np.array(K)

    def asdevice(self, a, tag, dtype=np.float64):
        self.calls.append("upload")
        return _Arr(np.asarray(a, dtype=dtype))

    def scratch(self, tag, shape):
        if tag not in self.pool or self.pool[tag].a.shape != tuple(shape):
            self.pool[tag] = _Arr(np.full(shape, np.nan))           # uninitialised memory: whoever reads it before writing is caught
        return self.pool[tag]

    def draw(self, B, S, n, dim, seed, offset):
        return np.stack([np.random.default_rng([seed, offset + b]).uniform(size=(S, n, dim)) for b in range(B)])

    def momentum_sums_d(self, x_d, s_d, S, seed=0, walker_offset=0):
        B, n, dim = x_d.a.shape
        self.offsets.append(walker_offset)
        shifts = self.draw(B, S, n, dim, seed, walker_offset)
        ratios = MR.planewave_ratios(x_d.a, self.table[s_d.a], self.L, shifts)
        out = self.scratch("momentum", (3 * self.K.shape[0] + 2,))
        out.a[:] = MR.momentum_ref(ratios, shifts, self.K)
        return out

    def axpby_d(self, a, x, b, y, count=None):
        y.a[:count] = a * x.a[:count] + (b * y.a[:count] if b != 0.0 else 0.0)
        return y

    def to_host(self, a):
        self.calls.append("download")
        return a.a.copy()


def _gas(rng, B, n=5):
    import coulombgas_amd as cg
    from tests.common import box_length, state_indices
    L = box_length(n, 2)
    table = cg.sp_orbitals(2, 25)[0].astype(np.float64)
    sidx = state_indices(rng, B, n, table.shape[0])           # the last n rows with up to 3 single excitations
    return L, table, sidx, rng.uniform(0.0, L, (B, n, 2))


def test_observable_host_logic():
    import coulombgas_amd as cg
    from coulombgas_amd.comm import NullComm
    rng = np.random.default_rng(5)
    n, B, S = 5, 24, 3
    L, table, sidx, x = _gas(rng, B, n)
    K = table[-20:]
    eng = _StandInEngine(L, table)
    obs = cg.make_momentum_observable(n, 2, L, K, shifts_per_particle=S, seed=9, comm=NullComm(), engine=eng)
    with pytest.raises(RuntimeError):
        obs.result()
    r = obs.accumulate(x, sidx).result()
    shifts = eng.draw(B, S, n, 2, 9, 0)
    nk, _ = MR.per_walker(MR.planewave_ratios(x, table[sidx], L, shifts), shifts, K)
    assert r["count"] == B and r["dropped"] == 0 and r["k"].shape == (20, 2) and np.allclose(r["k"], 2 * math.pi * K / L, rtol=1e-15)
    assert np.allclose(r["n_k"], nk.real.mean(0), rtol=0, atol=1e-13) and np.allclose(r["n_k_imag"], nk.imag.mean(0), rtol=0, atol=1e-13)
    # the standard error over walkers, from the second moment
    want = np.sqrt(np.maximum((nk.real ** 2).mean(0) - nk.real.mean(0) ** 2, 0.0) / (B - 1))
    assert np.allclose(r["stderr"], want, rtol=1e-10, atol=1e-14)
    assert np.allclose(r["stderr"], nk.real.std(0, ddof=0) / math.sqrt(B - 1), rtol=1e-8, atol=1e-14)
    # every call advances the Philox offset by its batch: no batch reuses shifts; four batches = one sum
    h = B // 4
    four = cg.make_momentum_observable(n, 2, L, K, shifts_per_particle=S, seed=9, comm=NullComm(), engine=eng)
    eng.offsets.clear()
    for q in range(4):
        four.accumulate(x[q * h:(q + 1) * h], sidx[q * h:(q + 1) * h])
    assert eng.offsets == [0, h, 2 * h, 3 * h] and four.offset == B
    r4 = four.result()
    assert r4["count"] == B and np.allclose(r4["n_k"], r["n_k"], rtol=0, atol=1e-13) and np.allclose(r4["stderr"], r["stderr"], rtol=1e-9, atol=1e-14)
    assert np.array_equal(four.result()["n_k"], r4["n_k"])          # result() twice: the accumulator is not consumed
    assert np.array_equal(obs.result()["n_k"], r["n_k"])            # ... and the two objects do not share one
    four.reset()
    with pytest.raises(RuntimeError):
        four.result()
    r5 = four.accumulate(x[:h], sidx[:h]).result()
    assert r5["count"] == h and eng.offsets[-1] == B                # reset() does not rewind the stream
    # a DeviceArray-like batch is taken as it is (no upload); one of another engine is refused
    eng.calls.clear()
    four.accumulate(_Arr(x[:h], eng), _Arr(sidx[:h], eng))
    assert "upload" not in eng.calls
    with pytest.raises(ValueError):
        four.accumulate(_Arr(x[:h], _StandInEngine(L, table)), sidx[:h])
    with pytest.raises(ValueError):
        four.accumulate(np.zeros((4, n + 1, 2)), sidx[:4])
    with pytest.raises(ValueError):
        four.accumulate(x[:4], sidx[:3])


def test_argument_checks_and_train_signature():
    import coulombgas_amd as cg
    K = np.array([[0.25, 0.25]])
    with pytest.raises(ValueError):
        cg.make_momentum_observable(13, 2, 6.39, K, shifts_per_particle=0)
    with pytest.raises(ValueError):
        cg.make_momentum_observable(13, 2, 6.39, np.array([[np.nan, 0.0]]))
    with pytest.raises(ValueError):
        cg.make_momentum_observable(13, 2, 6.39, np.zeros((0, 2)))
    with pytest.raises(ValueError):                                  # host walkers and no engine: nothing defines Psi
        cg.make_momentum_observable(13, 2, 6.39, K).accumulate(np.zeros((2, 13, 2)), np.zeros((2, 13), dtype=np.int32))
    p = inspect.signature(cg.train).parameters
    assert p["momentum"].default is None and p["structure"].default is None
    # train(momentum=None): the epoch loop reaches the accumulator only behind `if momentum is not None`
    src = inspect.getsource(cg.train)
    assert src.count("momentum.") == 1 and "if momentum is not None:" in src


# ---- (iii) known answers of the estimator, identity flow, numpy ratios ----------------------------------------------------------------
def test_regular_grid_gives_the_occupations_exactly():
    """theta = 0 (identity flow): on the regular G^2 grid, G above every |component difference| between a requested k and an occupied
    orbital, the shift sum is a discrete orthogonality relation and n_k^(b) is the occupation of k in walker b; sum_i r(i, s) =
    sum_j e^{2 pi i k_j.s} for every s"""
    from tests.common import orbitals
    rng = np.random.default_rng(2)
    n, B = 5, 6
    L, _, _, x = _gas(rng, B, n)
    table = orbitals(2, 25)                                          # the twisted table: k and the orbitals carry the same twist
    from tests.common import state_indices
    sidx = state_indices(rng, B, n, table.shape[0])
    kocc = table[sidx]
    G = MR.grid_size(table, kocc)
    grid = MR.regular_grid(G, 2)
    shifts = np.broadcast_to(grid[None, :, None, :], (B, G * G, n, 2))
    ratios = MR.planewave_ratios(x, kocc, L, shifts)
    nk, dropped = MR.per_walker(ratios, shifts, table)
    occ = MR.occupation(table, kocc)
    err = np.abs(nk - occ).max()
    print("G = %d: max |n_k^(b) - occupation| = %.2e" % (G, err))
    assert err <= 1e-10 and dropped.sum() == 0 and occ.sum(1).tolist() == [n] * B
    assert np.abs(nk.sum(1) - n).max() <= 1e-10
    rows = np.exp(2j * np.pi * np.einsum("sd,bjd->bsj", grid, kocc)).sum(-1)
    assert np.abs(ratios.sum(-1) - rows).max() <= 1e-10


def test_statistical_bound_holds_for_the_reference():
    """What the GPU statistics test asserts, with numpy in the place of both kernels: theta = 0, n = 13, the closed shell plus excited
    states, walkers from a short numpy Metropolis run on |det|^2 (every walker its own chain: independent), S = 2 uniform shifts per
    particle from a fixed seed.  For every one of the 81 table vectors n_k lies within 5 of its own standard errors (over walkers) of
    the occupation marginal of the batch.  (For the identity flow the estimator is unbiased for ANY x: the shift average of
    e^{-2 pi i k.s} r(i, s) is A[i, k] Ainv[k, i], which sums to the occupation over i; the Metropolis run only gives it the finite
    variance it has under |Psi|^2.)"""
    import coulombgas_amd as cg
    from tests.common import box_length
    rng = np.random.default_rng(20261017)
    n, B, S = 13, 2048, 2
    L = box_length(n, 2)
    table = cg.sp_orbitals(2, 25)[0].astype(np.float64)
    assert table.shape == (81, 2)
    sidx = np.tile(np.arange(n), (B, 1))
    for b in range(B // 2, B):                                       # half the batch: one or two single excitations out of the closed shell
        for _ in range(1 + b % 2):
            free = [i for i in range(40) if i not in sidx[b]]
            sidx[b, rng.integers(0, n)] = free[rng.integers(0, len(free))]
    kocc = table[sidx]
    x, rate = MR.metropolis_planewave(rng, rng.uniform(0.0, L, (B, n, 2)), kocc, L, 150, 0.3)
    shifts = rng.uniform(size=(B, S, n, 2))
    nk, dropped = MR.per_walker(MR.planewave_ratios(x, kocc, L, shifts), shifts, table)
    mean, want = nk.real.mean(0), MR.occupation(table, kocc).mean(0)
    stderr = np.sqrt(np.maximum((nk.real ** 2).mean(0) - mean ** 2, 0.0) / (B - 1))
    z = np.abs(mean - want) / stderr
    zi = np.abs(nk.imag.mean(0)) / (nk.imag.std(0) / math.sqrt(B - 1))
    print("accept rate %.3f; max |n_k - occupation| / stderr = %.2f at k = %s (n_k %.4f, occupation %.4f, stderr %.4f); imaginary part: %.2f"
          % (rate, z.max(), table[z.argmax()], mean[z.argmax()], want[z.argmax()], stderr[z.argmax()], zi.max()))
    assert dropped.sum() == 0 and 0.1 < rate < 0.6
    assert z.max() < 5.0
    assert zi.max() < 5.0
