"""cg_grad_laplacian_probes without a GPU: the probe loop of csrc/cg_lap.hpp on the host shim (tests/host_emul/cg_probes_emul.cpp:
n = 5 with every array in the "LDS" block, n = 17 with the block-wise layout), the combination rule both device headers share, and the
host-side logic of the Python layer (argument validation, key shapes, the factory's code paths).  The planned kernel's own loop
(cg_big.hpp: DPP / MFMA passes) runs on the GPU only: tests/test_gpu_probes.py."""
import inspect

import numpy as np
import pytest

from tests.common import orbitals, box_length, flow_theta, state_indices, walkers
from tests import probes_emul

B = 3
KS = (1, 2, 5)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return probes_emul.lib(tmp_path_factory.mktemp("probes_emul"))


class Case:
    def __init__(self, shim, n, mode):
        dim = 2
        self.n, self.dim, self.mode = n, dim, mode
        self.L = box_length(n, dim)
        self.sp = orbitals(dim)
        rng = np.random.default_rng(77 * n + mode)
        self.theta = flow_theta(rng, 2, 16, 16, dim, 0.05, 0.02)
        self.x = walkers(rng, B, n, dim, self.L)
        self.s = state_indices(rng, B, n, self.sp.shape[0])
        self.v = rng.standard_normal((max(KS),) + self.x.shape)
        probes_emul.ProbesEmulEngine.shim = shim
        self.eng = probes_emul.ProbesEmulEngine(n, dim, 2, 16, 16, self.L, self.sp)
        self.eng.set_params(self.theta)
        self.single = [self.eng.grad_laplacian(self.x, self.s, mode, self.v[k]) for k in range(max(KS))]


_CASES = {}


@pytest.fixture
def case(shim):
    def get(n, mode):
        if (n, mode) not in _CASES:
            _CASES[(n, mode)] = Case(shim, n, mode)
        return _CASES[(n, mode)]
    return get


CASES = [(5, 1), (5, 2), (17, 1), (17, 2)]


def lap_close(a, b):
    return float(np.abs(a - b).max()), 1e-9 * max(1.0, float(np.abs(b).max()))


@pytest.mark.parametrize("n,mode", CASES)
def test_one_probe_is_the_single_probe_code_bit_for_bit(case, n, mode):
    c = case(n, mode)
    g, l = c.eng.grad_laplacian_probes(c.x, c.s, mode, c.v[:1], weight=1.0)
    assert np.array_equal(g, c.single[0][0]) and np.array_equal(l, c.single[0][1])
    for K in (2, 5):
        assert np.array_equal(c.eng.grad_laplacian_probes(c.x, c.s, mode, c.v[:K])[0], c.single[0][0])


@pytest.mark.parametrize("n,mode", CASES)
def test_mean_of_oracle_evaluations(case, n, mode):
    import torch
    from oracle import cg_ref as R
    c = case(n, mode)
    rflow = R.FermiNet(2, 16, 16, c.L)
    rparams = R.flow_unravel(R.T(c.theta), 2, 16, 16, c.dim)
    kw = dict(hutchinson=True)
    if mode == 2:
        kw["logphi"], kw["logjacdet"] = R.make_logphi_logjacdet(rflow, c.sp, c.L)
    _, rfn = R.make_logpsi_grad_laplacian(R.make_logpsi(rflow, c.sp, c.L), **kw)
    Km = max(KS)                                   # one batched evaluation: the walkers repeated once per probe
    sb = torch.as_tensor(np.tile(c.s, (Km, 1)).astype(np.int64))
    go, lo = rfn(R.T(np.tile(c.x, (Km, 1, 1))), rparams, sb, R.T(c.v.reshape((Km * B,) + c.x.shape[1:])))
    go, lo = go.numpy().reshape((Km,) + c.x.shape), lo.numpy().reshape(Km, B)
    gr = go[0]
    for K in KS:
        g, l = c.eng.grad_laplacian_probes(c.x, c.s, mode, c.v[:K])
        lr = np.mean(lo[:K], axis=0)
        assert np.abs(g - gr).max() < 1e-10 * max(1.0, np.abs(gr).max()), K
        assert np.abs(l - lr).max() < 1e-9 * max(1.0, np.abs(lr).max()), K
        ref = np.mean([c.single[k][1] for k in range(K)], axis=0)
        err, bound = lap_close(l, ref)
        assert err < bound, (K, err, bound)


@pytest.mark.parametrize("n,mode", CASES)
def test_probes_do_not_leak_between_passes(case, n, mode):
    c = case(n, mode)
    _, l01 = c.eng.grad_laplacian_probes(c.x, c.s, mode, c.v[:2])
    _, l10 = c.eng.grad_laplacian_probes(c.x, c.s, mode, c.v[[1, 0]])
    err, bound = lap_close(l10, l01)
    assert err < bound, (err, bound)
    _, l00 = c.eng.grad_laplacian_probes(c.x, c.s, mode, c.v[[0, 0]], weight=0.5)
    err, bound = lap_close(l00, c.single[0][1])
    assert err < bound, (err, bound)


@pytest.mark.parametrize("n", [5, 17])
def test_basis_probes_give_the_exact_laplacian(case, n):
    c = case(n, 2)
    N = n * c.dim
    x1, s1 = c.x[:1], c.s[:1]
    ge, le = c.eng.grad_laplacian(x1, s1, 0)
    g, l = c.eng.grad_laplacian_probes(x1, s1, 2, np.eye(N).reshape(N, 1, n, c.dim), weight=1.0)
    err, bound = lap_close(l, le)
    assert err < bound, (err, bound)
    assert np.abs(g - ge).max() < 1e-10 * max(1.0, np.abs(ge).max())


def test_combination_rule(shim):
    """cg_probe_add / cg_probe_fold (csrc/cg_lap.hpp), shared by the loops of CgLap and CgBig: ascending sum that starts from probe 0's
    values, one multiplication by the weight, then the addition to the probe-free partials"""
    rng = np.random.default_rng(3)
    for K in (1, 2, 5):
        r = rng.standard_normal((K, 4)); tot = rng.standard_normal(4); w = 1.0 / K
        out = tot.copy()
        shim.emu_probe_combine(K, r.ctypes.data, w, out.ctypes.data)
        acc = r[0].copy()
        for k in range(1, K):
            acc = acc + r[k]
        assert np.array_equal(out, tot + w * acc)
    r = rng.standard_normal((1, 4)); tot = rng.standard_normal(4); out = tot.copy()
    shim.emu_probe_combine(1, r.ctypes.data, 1.0, out.ctypes.data)
    assert np.array_equal(out, tot + r[0])                  # one probe, weight 1: the single-probe statement `tot += r`


def test_shim_refuses_what_the_entry_point_refuses(case, shim):
    c = case(5, 2)
    g = np.empty((B, 5, 2, 2)); l = np.empty((B, 2))
    args = lambda mode, K, v: (5, 2, 16, 16, c.L, c.theta.ctypes.data, c.sp.ctypes.data, c.sp.shape[0], c.s.ctypes.data, c.x.ctypes.data, B, mode, K,
                               v, 0.5, g.ctypes.data, l.ctypes.data, 10080)
    assert shim.emu_grad_laplacian_probes(*args(0, 2, c.v.ctypes.data)) == -1
    assert shim.emu_grad_laplacian_probes(*args(2, 0, c.v.ctypes.data)) == -1
    assert shim.emu_grad_laplacian_probes(*args(2, 2, None)) == -1


# ---- the Python layer on the emulated engine --------------------------------------------------------------------------------------
def _factory(c, **kw):
    import coulombgas_amd as cg
    flow = cg.FermiNet(2, 16, 16, c.L)
    logpsi = cg.make_logpsi(flow, c.sp, c.L)
    logphi, logjacdet = cg.make_logphi_logjacdet(flow, c.sp, c.L)
    return cg.make_logpsi_grad_laplacian(logpsi, hutchinson=True, logphi=logphi, logjacdet=logjacdet, **kw)[1]


def test_factory_paths_and_key_shapes(case, shim, monkeypatch):
    probes_emul.install(monkeypatch, shim)
    c = case(5, 2)
    fn3, fn1, fn0 = _factory(c, probes=3), _factory(c, probes=1), _factory(c)
    assert fn3.probes == 3 and fn0.probes == 1 and fn3.mode == 2
    g, l = fn3(c.x, c.theta, c.s, c.v[:3])                                  # explicit probes
    gr, lr = c.eng.grad_laplacian_probes(c.x, c.s, 2, c.v[:3])
    assert np.array_equal(g, gr) and np.array_equal(l, lr)
    ga, la = fn1(c.x, c.theta, c.s, c.v[0]); gb, lb = fn0(c.x, c.theta, c.s, c.v[0])
    assert np.array_equal(la, lb) and np.array_equal(la, c.single[0][1]) and np.array_equal(ga, gb)
    _, ls = fn3(c.x, c.theta, c.s, 11)                                      # a seed: one standard_normal((K,) + x.shape)
    vs = np.random.default_rng(11).standard_normal((3,) + c.x.shape)
    assert np.array_equal(ls, c.eng.grad_laplacian_probes(c.x, c.s, 2, vs)[1])
    for bad in (c.v[0], c.v[:2], c.v[:3, :2]):                              # x.shape, another K, another batch
        with pytest.raises(ValueError):
            fn3(c.x, c.theta, c.s, bad)


def test_factory_and_driver_arguments():
    import coulombgas_amd as cg
    from coulombgas_amd.driver import train
    flow = cg.FermiNet(2, 16, 16, 4.0)
    logpsi = cg.make_logpsi(flow, orbitals(2), 4.0)
    with pytest.raises(ValueError):
        cg.make_logpsi_grad_laplacian(logpsi, probes=2)                     # the exact mode takes no probe
    with pytest.raises(ValueError):
        cg.make_logpsi_grad_laplacian(logpsi, hutchinson=True, probes=0)
    assert cg.make_logpsi_grad_laplacian(logpsi, hutchinson=True)[1].probes == 1
    assert inspect.signature(cg.make_logpsi_grad_laplacian).parameters["probes"].default == 1
    assert inspect.signature(train).parameters["hutchinson_probes"].default == 1


def test_engine_wrapper_checks_the_probe_shape_before_any_call():
    from coulombgas_amd.engine import Engine
    e = Engine.__new__(Engine)                      # no context: the shape check comes before the library is touched
    e.n, e.dim, e._ctx, e.sp_indices = 5, 2, None, orbitals(2).astype(np.float64)
    x = np.zeros((B, 5, 2)); s = np.tile(np.arange(5, dtype=np.int32), (B, 1))
    for bad in (np.zeros((B, 5, 2)), np.zeros((2, B + 1, 5, 2)), np.zeros((2, B, 5, 3))):
        with pytest.raises(ValueError):
            e.grad_laplacian_probes(x, s, 2, bad)
    assert e._probe_weight(4, None) == 0.25 and e._probe_weight(4, 1.0) == 1.0
