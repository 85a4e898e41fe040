"""tests/probes_emul.py -- TEST INFRASTRUCTURE ONLY.
tests/host_emul/cg_probes_emul.cpp (the probe loop of cg_grad_laplacian_probes compiled for the host) bound with ctypes, and an
EmulEngine that adds Engine.grad_laplacian_probes / grad_laplacian_probes_d on top of it.  The product never imports it."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.emul_engine import EmulEngine, _p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = {}


def lib(outdir):
    """builds the shim into outdir (once per directory) and returns the loaded library"""
    out = os.path.join(str(outdir), "libcg_probes_emul.so")
    if out not in _LIB:
        src = os.path.join(ROOT, "tests", "host_emul", "cg_probes_emul.cpp")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", out, src])
        L = C.CDLL(out)
        L.emu_grad_laplacian_probes.restype = C.c_int
        L.emu_grad_laplacian_probes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_long]
        L.emu_probe_combine.restype = None
        L.emu_probe_combine.argtypes = [C.c_int, C.c_void_p, C.c_double, C.c_void_p]
        _LIB[out] = L
    return _LIB[out]


class ProbesEmulEngine(EmulEngine):
    shim = None         # the loaded cg_probes_emul library (set by the test module's fixture)

    def grad_laplacian_probes(self, x, sidx, mode, v, weight=None):
        xb, lead = self._xb(x)
        B = xb.shape[0]
        s = np.ascontiguousarray(sidx, dtype=np.int32).reshape(B, self.n)
        v = np.ascontiguousarray(v, dtype=np.float64)
        K = v.shape[0]
        if v.shape != (K,) + tuple(np.shape(x)):
            raise ValueError("v must have shape (K,) + x.shape")
        g = np.empty((B, self.n, self.dim, 2)); l = np.empty((B, 2))
        rc = self.shim.emu_grad_laplacian_probes(self.n, self.dim, self.hs, self.ht, self.L, _p(self.theta), _p(self.sp), self.sp.shape[0], _p(s), _p(xb),
                                                 B, int(mode), K, _p(v), 1.0 / K if weight is None else float(weight), _p(g), _p(l), self.lds_budget)
        assert rc == 0
        return (g[..., 0] + 1j * g[..., 1]).reshape(lead + (self.n, self.dim)), (l[:, 0] + 1j * l[:, 1]).reshape(lead)

    def grad_laplacian_probes_d(self, x, s, mode, v, weight=None, with_scores=False):
        if with_scores:
            self.scores_compute_d(x, s)
        return self.grad_laplacian_probes(x, s, mode, v, weight)


def install(monkeypatch, shim):
    """Route coulombgas_amd's engine factory to the host emulation with the probes entry (CPU tests only)."""
    import coulombgas_amd.flow as fl
    cache = {}
    ProbesEmulEngine.shim = shim

    def get_engine(n, dim, depth, spsize, tpsize, L, sp_indices=None, device=None):
        key = (n, dim, depth, spsize, tpsize, float(L), None if sp_indices is None else np.asarray(sp_indices, dtype=np.float64).tobytes())
        if key not in cache:
            cache[key] = ProbesEmulEngine(n, dim, depth, spsize, tpsize, L, sp_indices)
        return cache[key]
    monkeypatch.setattr(fl, "get_engine", get_engine)
