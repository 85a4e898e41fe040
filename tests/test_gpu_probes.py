"""cg_grad_laplacian_probes on the GPU: K Hutchinson probes per walker behind one set-up (csrc/cg_lap.hpp, cg_big.hpp: the probe
loop around the jet pass; cg_k_derivs_a.hip: the entry point and the route of the configurations without such a kernel).

Shapes: the smallest at which each code path can still go wrong --
  n5     (2, 16, 16) n = 5    k_grad_lap2_probes, one wave of work
  n13    (2, 16, 16) n = 13   everything in LDS, incl. T^a / K^ab in the persistent block in mode 1
  n7d3   (3, 4, 4)   n = 7    the second translation unit
  n17    (2, 16, 16) n = 17   smallest size of the planned kernel (k_gradlap_big_probes)
  n32    (2, 16, 16) n = 32   planned kernel, last size with two rows per wave in the pair pass of the jet
  n33    (2, 16, 16) n = 33   planned kernel, first size with one row per wave
  n5d3   depth 3     n = 5    no probe-loop kernel: nprobe + 1 launches of the single-probe kernel, combined on the device
  c8n13  (2, 8, 8)   n = 13   k_grad_lap2_probes of the other configurations of the second translation unit: one per hidden width and
  c32n5  (2, 32, 32) n = 5      dimension (tests/config_shapes.py: the path map of these configurations)
  c16n8  (3, 16, 16) n = 8
  c8n7d3 (3, 8, 8)   n = 7
  c8n17  (2, 8, 8)   n = 17   such a configuration beyond the all-LDS kernel: single-probe launches of k_grad_lap2<AL = false>, combined
B = 3 walkers, K in {1, 2, 5}.  The single-probe results, and the oracle's, are computed once per (shape, mode) and shared."""
import numpy as np
import pytest

from tests.common import GOLDEN, orbitals, box_length, flow_theta, state_indices, walkers

pytestmark = pytest.mark.gpu

SHAPES = {"n5": (5, 2, 2, 16, 16), "n13": (13, 2, 2, 16, 16), "n7d3": (7, 3, 2, 4, 4), "n17": (17, 2, 2, 16, 16),
          "n32": (32, 2, 2, 16, 16), "n33": (33, 2, 2, 16, 16), "n5d3": (5, 2, 3, 16, 16),
          "c8n13": (13, 2, 2, 8, 8), "c32n5": (5, 2, 2, 32, 32), "c16n8": (8, 3, 2, 16, 16), "c8n7d3": (7, 3, 2, 8, 8), "c8n17": (17, 2, 2, 8, 8)}
NATIVE = [("n5", 2), ("n13", 1), ("n13", 2), ("n7d3", 2), ("n17", 2), ("n32", 1), ("n32", 2), ("n33", 2),
          ("c8n13", 1), ("c8n13", 2), ("c32n5", 2), ("c16n8", 1), ("c16n8", 2), ("c8n7d3", 2)]
EVERY = NATIVE + [("n5d3", 2), ("c8n17", 1), ("c8n17", 2)]
KS = (1, 2, 5)
B = 3


def lap_close(a, b):
    """the project's Laplacian tolerance: 1e-9 max(1, |lap|); returns (error, bound)"""
    return float(np.abs(a - b).max()), 1e-9 * max(1.0, float(np.abs(b).max()))


class Case:
    def __init__(self, name, mode):
        from coulombgas_amd.engine import Engine
        n, dim, depth, hs, ht = SHAPES[name]
        self.cfg, self.mode = SHAPES[name], mode
        self.L = box_length(n, dim)
        self.sp = orbitals(dim)
        rng = np.random.default_rng(1000 * n + 10 * dim + depth)
        self.theta = flow_theta(rng, depth, hs, ht, dim, 0.05, 0.02)
        self.x = walkers(rng, B, n, dim, self.L)
        self.s = state_indices(rng, B, n, self.sp.shape[0])
        self.v = rng.standard_normal((max(KS),) + self.x.shape)
        self.eng = Engine(n, dim, depth, hs, ht, self.L, self.sp)
        self.eng.set_params(self.theta)
        self.single = [self.eng.grad_laplacian(self.x, self.s, mode, self.v[k]) for k in range(max(KS))]
        self._probes, self._oracle = {}, None

    def probes(self, K):
        if K not in self._probes:
            self._probes[K] = self.eng.grad_laplacian_probes(self.x, self.s, self.mode, self.v[:K])
        return self._probes[K]

    def oracle(self):
        if self._oracle is None:
            import torch
            from oracle import cg_ref as R
            n, dim, depth, hs, ht = self.cfg
            rflow = R.FermiNet(depth, hs, ht, self.L)
            rparams = R.flow_unravel(R.T(self.theta), depth, hs, ht, dim)
            r_logpsi = R.make_logpsi(rflow, self.sp, self.L)
            kw = dict(hutchinson=True)
            if self.mode == 2:
                kw["logphi"], kw["logjacdet"] = R.make_logphi_logjacdet(rflow, self.sp, self.L)
            _, rfn = R.make_logpsi_grad_laplacian(r_logpsi, **kw)
            K = max(KS)                            # one batched evaluation: the walkers repeated once per probe
            sb = torch.as_tensor(np.tile(self.s, (K, 1)).astype(np.int64))
            g, l = rfn(R.T(np.tile(self.x, (K, 1, 1))), rparams, sb, R.T(self.v.reshape((K * B,) + self.x.shape[1:])))
            g, l = g.numpy().reshape((K,) + self.x.shape), l.numpy().reshape(K, B)
            self._oracle = [(g[k], l[k]) for k in range(K)]
        return self._oracle


_CASES = {}


@pytest.fixture(scope="module")
def case():
    def get(name, mode):
        if (name, mode) not in _CASES:
            _CASES[(name, mode)] = Case(name, mode)
        return _CASES[(name, mode)]
    yield get
    for c in _CASES.values():
        c.eng.close()
    _CASES.clear()


@pytest.mark.parametrize("name,mode", NATIVE)
def test_one_probe_is_the_single_probe_call_bit_for_bit(case, name, mode):
    c = case(name, mode)
    g, l = c.eng.grad_laplacian_probes(c.x, c.s, mode, c.v[:1], weight=1.0)
    g1, l1 = c.single[0]
    assert np.array_equal(g, g1) and np.array_equal(l, l1)


@pytest.mark.parametrize("name,mode", NATIVE)
def test_gradient_ignores_the_probes(case, name, mode):
    c = case(name, mode)
    for K in (2, 5):
        assert np.array_equal(c.probes(K)[0], c.single[0][0]), K


@pytest.mark.parametrize("name,mode", EVERY)
def test_mean_of_single_calls(case, name, mode):
    """lap with weight 1 / K against the mean of the K single-call Laplacians: summation order only (measured maxima: DESIGN section 4)"""
    c = case(name, mode)
    worst = 0.0
    for K in KS:
        g, l = c.probes(K)
        ref = np.mean([c.single[k][1] for k in range(K)], axis=0)
        err, bound = lap_close(l, ref)
        worst = max(worst, err / max(1.0, float(np.abs(ref).max())))
        print("probes vs mean of single calls: %s mode %d K %d  max |dlap| %.3e (bound %.3e)" % (name, mode, K, err, bound))
        assert err < bound, (K, err, bound)
        assert np.abs(g - c.single[0][0]).max() < 1e-10 * max(1.0, np.abs(c.single[0][0]).max())
    print("probes vs mean of single calls: %s mode %d  worst relative %.3e" % (name, mode, worst))


@pytest.mark.parametrize("name,mode", EVERY)
def test_mean_of_oracle_evaluations(case, name, mode):
    """the same against oracle/cg_ref.py evaluated once per probe: the bounds of tests/test_gpu_parity.py for modes 1 and 2"""
    c = case(name, mode)
    ora = c.oracle()
    for K in KS:
        g, l = c.probes(K)
        gr = ora[0][0]
        lr = np.mean([ora[k][1] for k in range(K)], axis=0)
        assert np.abs(g - gr).max() < 1e-10 * max(1.0, np.abs(gr).max()), K
        assert np.abs(l - lr).max() < 1e-9 * max(1.0, np.abs(lr).max()), K


@pytest.mark.parametrize("name,mode", EVERY)
def test_probes_do_not_leak_between_passes(case, name, mode):
    """(v0, v1) against (v1, v0), and (v0, v0) with weight 1/2 against the single call on v0: a jet array laid over something the
    next pass reads would show here"""
    c = case(name, mode)
    _, l01 = c.probes(2)
    _, l10 = c.eng.grad_laplacian_probes(c.x, c.s, mode, c.v[[1, 0]])
    err, bound = lap_close(l10, l01)
    assert err < bound, (err, bound)
    _, l00 = c.eng.grad_laplacian_probes(c.x, c.s, mode, c.v[[0, 0]], weight=0.5)
    err, bound = lap_close(l00, c.single[0][1])
    assert err < bound, (err, bound)


def _basis_probes_case(eng, x1, s1, n, dim):
    N = n * dim
    ge, le = eng.grad_laplacian(x1, s1, 0)
    v = np.eye(N).reshape(N, 1, n, dim)
    g, l = eng.grad_laplacian_probes(x1, s1, 2, v, weight=1.0)
    err, bound = lap_close(l, le)
    print("basis probes vs exact mode: n %d  |dlap| %.3e (bound %.3e)" % (n, err, bound))
    assert err < bound, (err, bound)
    assert np.abs(g - ge).max() < 1e-10 * max(1.0, np.abs(ge).max())


@pytest.mark.parametrize("name", ["n17", "n33"])
def test_basis_probes_give_the_exact_laplacian(case, name):
    c = case(name, 2)
    n, dim = c.cfg[:2]
    _basis_probes_case(c.eng, c.x[:1], c.s[:1], n, dim)


def test_basis_probes_give_the_exact_laplacian_on_a_golden_walker():
    from coulombgas_amd.engine import Engine
    g = np.load(GOLDEN + "/golden_n29_d2_rs1.npz")
    n, dim, L = int(g["n"]), int(g["dim"]), float(g["L"])
    eng = Engine(n, dim, 2, 16, 16, L, g["sp_indices"])
    eng.set_params(g["theta"])
    _basis_probes_case(eng, g["x"][1:2], g["state_idx"][1:2], n, dim)
    eng.close()


def test_second_launch_chunk(monkeypatch):
    """n = 17, B = 300, K = 2 with the planned kernel held to ONE workgroup per CU and one round per launch (256 walkers a launch on the
    256 CUs of an MI355X; CG_BIG_ROUNDS alone leaves two workgroups per CU at this size, 512 a launch): rows 256 ... 299 go through a
    second launch that reuses the workspace slots of the first"""
    from coulombgas_amd.engine import Engine
    monkeypatch.setenv("CG_BIG_ROUNDS", "1")
    monkeypatch.setenv("CG_BIG_PER_CU", "1")
    n, dim, Bb, K = 17, 2, 300, 2
    L = box_length(n, dim)
    sp = orbitals(dim)
    rng = np.random.default_rng(17300)
    eng = Engine(n, dim, 2, 16, 16, L, sp)
    eng.set_params(flow_theta(rng, 2, 16, 16, dim, 0.05, 0.02))
    x = walkers(rng, Bb, n, dim, L); s = state_indices(rng, Bb, n, sp.shape[0]); v = rng.standard_normal((K,) + x.shape)
    g, l = eng.grad_laplacian_probes(x, s, 2, v)
    g2, l2 = eng.grad_laplacian_probes(x, s, 2, v)
    assert np.array_equal(g, g2) and np.array_equal(l, l2)
    gt, lt = eng.grad_laplacian_probes(x[256:], s[256:], 2, v[:, 256:])
    assert np.array_equal(g[256:], gt) and np.array_equal(l[256:], lt)
    eng.close()


def test_argument_errors(case):
    from coulombgas_amd._lib import CoulombGasError, CG_ERR_ARG
    c = case("n5", 2)
    before = c.eng.grad_laplacian(c.x, c.s, 2, c.v[0])
    for kw in (dict(mode=0, v=c.v[:2]), dict(mode=2, v=c.v[:0]), dict(mode=2, v=None)):
        with pytest.raises(CoulombGasError) as ei:
            c.eng.grad_laplacian_probes(c.x, c.s, **kw)
        assert ei.value.code == CG_ERR_ARG, kw
    with pytest.raises(ValueError):
        c.eng.grad_laplacian_probes(c.x, c.s, 2, c.v[0])                # a single probe without the leading axis
    after = c.eng.grad_laplacian(c.x, c.s, 2, c.v[0])
    assert np.array_equal(before[1], after[1])


@pytest.mark.parametrize("name", ["n13", "n17"])
def test_python_layer(case, name):
    import coulombgas_amd as cg
    from coulombgas_amd.engine import DeviceArray
    c = case(name, 2)
    n, dim, depth, hs, ht = c.cfg
    flow = cg.FermiNet(depth, hs, ht, c.L)
    logpsi = cg.make_logpsi(flow, c.sp, c.L)
    logphi, logjacdet = cg.make_logphi_logjacdet(flow, c.sp, c.L)
    _, fn3 = cg.make_logpsi_grad_laplacian(logpsi, hutchinson=True, logphi=logphi, logjacdet=logjacdet, probes=3)
    _, fn1 = cg.make_logpsi_grad_laplacian(logpsi, hutchinson=True, logphi=logphi, logjacdet=logjacdet, probes=1)
    _, fn0 = cg.make_logpsi_grad_laplacian(logpsi, hutchinson=True, logphi=logphi, logjacdet=logjacdet)
    assert fn3.probes == 3 and fn1.mode == fn3.mode == 2
    eng = flow.engine(n, dim, c.sp)
    eng.set_params(c.theta)
    g_ref, l_ref = eng.grad_laplacian_probes(c.x, c.s, 2, c.v[:3])
    # explicit probes, numpy in / numpy out
    g, l = fn3(c.x, c.theta, c.s, c.v[:3])
    assert np.array_equal(g, g_ref) and np.array_equal(l, l_ref)
    # probes = 1 is today's closure
    ga, la = fn1(c.x, c.theta, c.s, c.v[0]); gb, lb = fn0(c.x, c.theta, c.s, c.v[0])
    assert np.array_equal(ga, gb) and np.array_equal(la, lb)
    # device arrays; with_scores leaves the scores of scores_compute_d resident, under the key an optimisation step looks them up by
    x_d = DeviceArray.from_numpy(eng, c.x); s_d = DeviceArray.from_numpy(eng, c.s, np.int32)
    mean = eng.scratch("probe_test_mean", (2 * eng.P,))
    gd, ld = fn3(x_d, c.theta, s_d, c.v[:3], with_scores=True)
    gd, ld = np.asarray(gd), np.asarray(ld)
    assert np.array_equal(gd.reshape(g_ref.shape), g_ref) and np.array_equal(ld.reshape(l_ref.shape), l_ref)
    assert eng._score_key_d == (x_d.token, x_d.version, s_d.token, s_d.version, eng._theta_version)
    eng.scores_mean_d(mean)
    got = np.asarray(mean).copy()
    x_d.upload(c.x)                                                      # a new version of the walkers: the scores are computed again
    eng.scores_compute_d(x_d, s_d)
    eng.scores_mean_d(mean)
    assert np.array_equal(np.asarray(mean), got) and np.abs(got).max() > 0
    # a seed: one cg_randn draw of K B n dim values, the same at every call
    _, l1 = fn3(x_d, c.theta, s_d, 20261017); l1 = np.asarray(l1).copy()
    _, l2 = fn3(x_d, c.theta, s_d, 20261017); l2 = np.asarray(l2).copy()
    assert np.array_equal(l1, l2) and not np.array_equal(l1, ld)
    vd = np.asarray(eng.scratch("probes", (3,) + c.x.shape))
    _, l3 = eng.grad_laplacian_probes(c.x, c.s, 2, vd)
    assert np.array_equal(l1.reshape(l3.shape), l3)
