"""Structure observables without a GPU: (i) the host logic and normalisation of coulombgas_amd.structure against a stand-in engine that
fills the packed vector from the numpy restatement (tests/structure_ref.py), (ii) the device arithmetic of csrc/cg_structure.hpp
compiled for the host (tests/host_emul/cg_structure_emul.cpp, the 1-thread CgBlk shim) against the same restatement."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from tests.structure_ref import SHAPES, seeded_walkers, kgrid, pair_t, edge_gap, structure_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Arr:
    """what a DeviceArray is to coulombgas_amd.structure: something with .ptr that the engine's calls take"""
    def __init__(self, a):
        self.a, self.ptr, self.shape = np.array(a, dtype=np.float64), id(self), np.shape(a)


class _StandInEngine:
    def __init__(self, L):
        self.L, self.pool, self.calls = L, {}, []

    def set_structure(self, K, nbins, rmax):
        self.cfg = (np.array(K), int(nbins), float(rmax))

    def asdevice(self, a, tag, dtype=np.float64):
        self.calls.append("upload")
        return _Arr(a)

    def scratch(self, tag, shape):
        if tag not in self.pool or self.pool[tag].a.shape != tuple(shape):
            self.pool[tag] = _Arr(np.full(shape, np.nan))           # uninitialised memory: whoever reads it before writing is caught
        return self.pool[tag]

    def structure_sums_d(self, x_d):
        out = self.scratch("structure", (3 * self.cfg[0].shape[0] + self.cfg[1] + 2,))
        out.a[:] = structure_ref(x_d.a, self.L, *self.cfg)
        return out

    def axpby_d(self, a, x, b, y, count=None):
        y.a[:count] = a * x.a[:count] + (b * y.a[:count] if b != 0.0 else 0.0)
        return y

    def to_host(self, a):
        self.calls.append("download")
        return a.a.copy()


@pytest.mark.parametrize("n,dim,B,L", SHAPES)
def test_normalisation_and_host_logic(n, dim, B, L):
    import coulombgas_amd as cg
    from coulombgas_amd.comm import NullComm
    nbins, rmax = 128, 0.5
    K = kgrid(dim)
    x = seeded_walkers(n, dim, B, L)
    eng = _StandInEngine(L)
    obs = cg.make_structure_observable(n, dim, L, K, nbins=nbins, rmax=rmax, comm=NullComm(), engine=eng)
    with pytest.raises(RuntimeError):
        obs.result()
    r = obs.accumulate(x).result()
    raw = structure_ref(x, L, K, nbins, rmax)
    pairs = B * n * (n - 1) // 2
    assert r["count"] == B and r["hist"].sum() + r["overflow"] == pairs and r["overflow"] > 0
    assert r["k"].shape == (K.shape[0], dim) and np.allclose(r["k"], 2 * math.pi * K / L, rtol=1e-15)
    # S(k = 0) = n, rho_0 = n; S is the packed sum over n count; the connected part removes |<rho>|^2 / n
    assert abs(r["S"][0] - n) < 1e-12 * n and abs(r["rho"][0] - n) < 1e-12 * n and abs(r["S_connected"][0]) < 1e-10 * n
    assert np.allclose(r["S"], raw[:K.shape[0]] / (n * B), rtol=1e-14)
    assert np.allclose(r["S_connected"], r["S"] - np.abs(r["rho"]) ** 2 / n, rtol=1e-14, atol=1e-14)
    # g integrates back to the pair count: sum_b g_b V_b (count n(n-1)/2) / L^dim = the pairs inside rmax
    edges = rmax * L * np.arange(nbins + 1) / nbins
    shell = math.pi * np.diff(edges ** 2) if dim == 2 else 4 * math.pi / 3 * np.diff(edges ** 3)
    assert np.allclose(r["r"], 0.5 * (edges[1:] + edges[:-1]), rtol=1e-15)
    back = (r["g"] * shell).sum() * pairs / L ** dim
    assert abs(back - (pairs - r["overflow"])) < 1e-10 * pairs
    # uncorrelated uniform particles: g -> 1 (the outer half of the bins holds thousands of pairs each)
    w = r["hist"][nbins // 2:]
    assert abs((r["g"][nbins // 2:] * w).sum() / w.sum() - 1.0) < 0.05
    # two accumulate calls = one call on the concatenated batch; the accumulator survives result(); reset() starts over
    h = B // 2
    two = cg.make_structure_observable(n, dim, L, K, nbins=nbins, rmax=rmax, comm=NullComm(), engine=eng)
    r2 = two.accumulate(x[:h]).accumulate(x[h:]).result()
    assert np.array_equal(r2["hist"], r["hist"]) and r2["overflow"] == r["overflow"] and r2["count"] == B
    assert np.allclose(r2["S"], r["S"], rtol=1e-13) and np.allclose(r2["rho"], r["rho"], rtol=0, atol=1e-13 * n)
    assert np.array_equal(two.result()["hist"], r["hist"])          # result() twice: the accumulator is not consumed
    assert np.array_equal(obs.result()["hist"], r["hist"])          # ... and the two objects do not share one
    two.reset()
    with pytest.raises(RuntimeError):
        two.result()
    r3 = two.accumulate(x[:h]).result()
    assert r3["count"] == h and np.array_equal(r3["hist"], structure_ref(x[:h], L, K, nbins, rmax)[3 * K.shape[0]:-2])


def test_argument_checks_and_train_signature():
    import inspect
    import coulombgas_amd as cg
    with pytest.raises(ValueError):
        cg.make_structure_observable(13, 2, 6.39, kgrid(2), rmax=0.6)
    with pytest.raises(ValueError):
        cg.make_structure_observable(13, 2, 6.39, kgrid(2), nbins=0)
    obs = cg.make_structure_observable(13, 2, 6.39, kgrid(2), engine=_StandInEngine(6.39))
    with pytest.raises(ValueError):
        obs.accumulate(np.zeros((4, 12, 2)))
    assert inspect.signature(cg.train).parameters["structure"].default is None
    from coulombgas_amd.comm import NullComm
    a = object()
    assert NullComm().psum_d(a) is a


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    src = os.path.join(ROOT, "tests", "host_emul", "cg_structure_emul.cpp")
    out = str(tmp_path_factory.mktemp("structure_emul") / "libcg_structure_emul.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", out, src])
    lib = C.CDLL(out)
    lib.emu_structure_sums.restype = C.c_int
    lib.emu_structure_sums.argtypes = [C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_int, C.c_void_p]
    return lib


def _emul_sums(lib, x, L, K, nbins, rmax):
    B, n, dim = x.shape
    K32 = np.ascontiguousarray(K, dtype=np.int32)
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.full(3 * K32.shape[0] + nbins + 2, np.nan)
    assert lib.emu_structure_sums(n, dim, L, K32.ctypes.data, K32.shape[0], nbins, rmax, x.ctypes.data, B, out.ctypes.data) == 0
    return out


@pytest.mark.parametrize("n,dim,B,L", SHAPES)
def test_device_arithmetic_on_the_host(emul, n, dim, B, L):
    """|rho|^2 and rho sums to 1e-12 of n^2 B; every histogram bin and the overflow EXACTLY, no pair excluded -- legitimate because no
    pair of these seeded inputs has t within 1e-9 of a bin edge (asserted; the gap is ~1.5e-5, nine orders above fp64 rounding of d)"""
    nbins, rmax = 128, 0.5
    K = kgrid(dim)
    nK = K.shape[0]
    x = seeded_walkers(n, dim, B, L)
    t = pair_t(x, L, nbins, rmax)
    gap = edge_gap(t)
    print("n=%d dim=%d B=%d: smallest gap to a bin edge %.3e, overflow share %.3f, nearest pair t/nbins*rmax = %.3e"
          % (n, dim, B, gap, float((t >= nbins).mean()), float(t.min()) * rmax / nbins))
    assert gap >= 1e-9
    ref = structure_ref(x, L, K, nbins, rmax)
    got = _emul_sums(emul, x, L, K, nbins, rmax)
    err = np.abs(got[:3 * nK] - ref[:3 * nK]).max() / (n * n * B)
    print("max |rho sums - numpy| / (n^2 B) = %.3e" % err)
    assert err <= 1e-12
    assert np.array_equal(got[3 * nK:], ref[3 * nK:])
    assert got[3 * nK:-1].sum() == B * n * (n - 1) // 2 and got[-1] == B
    # the row rule: B walkers in min(B, 1024) rows; an empty batch gives zeros; a NaN walker keeps the pair count
    assert np.array_equal(_emul_sums(emul, x[:0], L, K, nbins, rmax), np.zeros(3 * nK + nbins + 2))
    xn = x[:8].copy(); xn[3, 1, 0] = np.nan
    gn = _emul_sums(emul, xn, L, K, nbins, rmax)
    assert gn[3 * nK:-1].sum() == 8 * n * (n - 1) // 2 and gn[-1] == 8 and np.isnan(gn[1:3 * nK]).any()
    assert np.array_equal(gn[3 * nK:], structure_ref(xn, L, K, nbins, rmax)[3 * nK:])


def test_rows_beyond_the_row_count_on_the_host(emul):
    """B > 1024: rows hold several walkers each (the grid-stride path of the kernel); histogram exact, sums to 1e-12"""
    n, dim, L, nbins, rmax = 5, 2, 3.0, 32, 0.5
    K = kgrid(dim)[:40]
    x = seeded_walkers(n, dim, 2500, L, seed=7)
    assert edge_gap(pair_t(x, L, nbins, rmax)) >= 1e-9
    ref, got = structure_ref(x, L, K, nbins, rmax), _emul_sums(emul, x, L, K, nbins, rmax)
    assert np.array_equal(got[120:], ref[120:])
    assert np.abs(got[:120] - ref[:120]).max() <= 1e-12 * n * n * 2500
