"""GPU parity tests of the flow configurations of the second translation unit (csrc/cg_dispatch.hpp: CG_FAST_CONFIGS_B) on every
kernel path they take.  The shapes and the path each stands for come from tests/config_shapes.py, which tests/test_path_coverage.py
keeps complete on the CPU; the inputs come from the package's generators with the seed 1000 n + 10 dim + spsize.

Sampler family (every "S" shape, weight scales 0.3 -- a flow near the identity -- and 1.5 -- row exchanges in every LU): log phi,
1/2 log|det J|, the flow and its Jacobian against oracle/cg_oracle.c, a 4-step chain with supplied draws against cgo_mcmc, one Philox
chain against the separate log Psi kernel.  Derivative family: modes 1 and 2 against oracle/cg_ref.py, mode 0 against it (n <= 7) or
against tests/golden/golden_configs_exact.npz and against the sum of the basis probes of mode 2, scores / theta-VJP / Fisher matrix
against the oracle, and the second launch chunk of the workspace kernels.

Tolerances are those of tests/test_gpu_parity.py: test_large_n_against_c_oracle (1e-10, 1e-10, 1e-11) at the weight scale 0.3,
test_large_n_with_row_exchanges_against_c_oracle (1e-9) at 1.5, test_flow_and_jacobian (1e-12, here times max(1, |J|) as well: an entry
of J is a sum of ~ n spsize products, rounding error ~ 1e-14 |J|), test_grad_laplacian_all_modes, test_param_vjp_and_scores,
test_quantum_fisher_and_sr_update.  Every figure is printed before it is asserted (pytest -s)."""
import ctypes as C

import numpy as np
import pytest

from tests import config_shapes as cs
from tests.common import GOLDEN

pytestmark = pytest.mark.gpu

B_SAMPLER = 3


def _id(shape, extra=""):
    d, hs, ht, n = shape
    return "d%ds%dt%d-n%d-%s" % (d, hs, ht, n, extra)


def _sampler_id(shape):
    thr, lu, flags = cs.SHAPES[shape]["S"].split(":")
    return _id(shape, "T%s-%s-%s" % (thr, lu.replace("<", "").replace(">", "").replace(",", "x"), flags))


def _engine(shape, s):
    from coulombgas_amd.engine import Engine
    dim, hs, ht, n = shape
    eng = Engine(n, dim, 2, hs, ht, s["L"], s["sp"])
    eng.set_params(s["theta"])
    info = eng.launch_info()
    p = cs.paths(*shape)
    assert info["threads"] == p["threads"] and info["fast"] == p["fast"] == 1, (info, p)
    return eng


_ORACLE = None


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


# ---------------------------------------------------------------------------------------------------------------------------------
# sampler family
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ws", [0.3, 1.5], ids=["ws03", "ws15"])
@pytest.mark.parametrize("shape", cs.shapes_of("S"), ids=_sampler_id)
def test_sampler_against_c_oracle(shape, ws):
    dim, hs, ht, n = shape
    N, B = n * dim, B_SAMPLER
    s = cs.inputs(shape, B, ws)
    L, sp, theta, x, sidx, rng = s["L"], s["sp"], s["theta"], s["x"], s["sidx"], s["rng"]
    lib = _c_oracle()
    eng = _engine(shape, s)
    print("%s ws %.1f: %s" % (shape, ws, cs.SHAPES[shape]["S"]))
    tol = 1e-10 if ws < 1.0 else 1e-9
    # log phi, 1/2 log|det J|
    out = np.zeros((B, 3))
    lib.cgo_logpsi(n, dim, 2, hs, ht, C.c_double(L), _p(theta), _p(sp), sp.shape[0], _p(sidx), _p(x), B, _p(out))
    lphi, hld = eng.logphi_logjacdet(x, sidx)
    _check("Re log phi", np.abs(lphi[:, 0] - out[:, 0]).max(), tol * np.abs(out[:, 0]).max())
    _check("Im log phi (mod 2 pi)", np.abs(np.angle(np.exp(1j * (lphi[:, 1] - out[:, 1])))).max(), tol)
    if ws < 1.0:
        _check("1/2 log|det J|", np.abs(hld - out[:, 2]).max(), 1e-11)
    else:
        _check("1/2 log|det J|", np.abs(hld - out[:, 2]).max(), 1e-9 * max(1.0, np.abs(out[:, 2]).max()))
    # flow and Jacobian
    zr = np.zeros((B, n, dim)); Jr = np.zeros((B, N, N))
    lib.cgo_flow(n, dim, 2, hs, ht, C.c_double(L), _p(theta), _p(x), B, _p(zr), _p(Jr))
    z = eng.flow_forward(x)
    J = np.asarray(eng.flow_jacobian(x)).reshape(B, N, N)
    _check("flow", np.abs(z - zr).max(), 1e-12 * max(1.0, np.abs(zr).max()))
    _check("Jacobian", np.abs(J - Jr).max(), 1e-12 * max(1.0, np.abs(Jr).max()))
    if ws > 1.0 and n > 1:
        d = np.abs(np.diagonal(J, axis1=1, axis2=2)); off = np.abs(J).sum(-1) - d
        assert (off > d).any()                              # the case does exercise pivoting: J is not diagonally dominant
    # 4 steps with supplied draws
    steps, std = 4, 0.1
    noise = rng.standard_normal((steps, B, n, dim)); unif = rng.uniform(size=(steps, B))
    xg, lpg, nacc = eng.mcmc(x, sidx, steps, std, noise=noise, unif=unif)
    xc = x.copy(); lpc = np.zeros(B)
    rate = lib.cgo_mcmc(n, dim, 2, hs, ht, C.c_double(L), _p(theta), _p(sp), sp.shape[0], _p(sidx), _p(xc), B, steps, C.c_double(std),
                        _p(noise), _p(unif), _p(lpc))
    print("  accepted %d of %d (oracle rate %.4f)" % (nacc, steps * B, rate))
    assert nacc / (steps * B) == pytest.approx(rate, abs=1e-15)
    if n == 1:
        assert nacc == steps * B                            # |Psi|^2 of one particle is constant: every step is accepted
    _check("chain positions", np.abs(xg - xc).max(), 1e-12)
    _check("chain log p against the oracle", np.abs(lpg - lpc).max(), 1e-9 * max(1.0, np.abs(lpc).max()))
    _check("chain log p against the log Psi kernel", np.abs(lpg - eng.logp(xg, sidx)).max(), tol * max(1.0, np.abs(lpg).max()))
    # Philox chain: final log p == log p of the final positions
    xf, lpf, _ = eng.mcmc(x, sidx, 10, std, seed=42)
    assert np.isfinite(xf).all()
    _check("Philox chain bookkeeping", np.abs(lpf - eng.logp(xf, sidx)).max(), tol * max(1.0, np.abs(lpf).max()))
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# derivative family
# ---------------------------------------------------------------------------------------------------------------------------------
def _oracle_fns(shape, s):
    from oracle import cg_ref as R
    dim, hs, ht, n = shape
    rflow = R.FermiNet(2, hs, ht, s["L"])
    rparams = R.flow_unravel(R.T(s["theta"]), 2, hs, ht, dim)
    r_logpsi = R.make_logpsi(rflow, s["sp"], s["L"])
    return R, rflow, rparams, r_logpsi


HUTCH = [(sh, m) for sh in sorted(cs.SHAPES) for m in (1, 2) if "L%d" % m in cs.SHAPES[sh]]


@pytest.mark.parametrize("shape,mode", HUTCH, ids=lambda v: _id(v, "lap") if isinstance(v, tuple) else "mode%d" % v)
def test_hutchinson_modes_against_the_oracle(shape, mode):
    """modes 1 and 2 with an explicit probe array; the two modes share their gradient"""
    import torch
    dim, hs, ht, n = shape
    B = 1 if n >= 30 else 2
    s = cs.inputs(shape, B, cs.DERIV_WS)
    x, sidx = s["x"], s["sidx"]
    v = s["rng"].standard_normal(x.shape)
    eng = _engine(shape, s)
    print("%s mode %d: %s" % (shape, mode, cs.SHAPES[shape]["L%d" % mode]))
    R, rflow, rparams, r_logpsi = _oracle_fns(shape, s)
    kw = dict(hutchinson=True)
    if mode == 2:
        kw["logphi"], kw["logjacdet"] = R.make_logphi_logjacdet(rflow, s["sp"], s["L"])
    _, rfn = R.make_logpsi_grad_laplacian(r_logpsi, **kw)
    gr, lr = rfn(R.T(x), rparams, torch.as_tensor(sidx.astype(np.int64)), R.T(v))
    gr, lr = gr.numpy(), lr.numpy()
    g, l = eng.grad_laplacian(x, sidx, mode, v)
    assert g.shape == x.shape and l.shape == (B,)
    _check("gradient", np.abs(g - gr).max(), 1e-10 * max(1.0, np.abs(gr).max()))
    _check("Laplacian", np.abs(l - lr).max(), 1e-9 * max(1.0, np.abs(lr).max()))
    g_other, _ = eng.grad_laplacian(x, sidx, 3 - mode, v)
    _check("gradient of the other mode", np.abs(g_other - g).max(), 1e-10 * max(1.0, np.abs(g).max()))
    eng.close()


_EXACT = None


def _exact_golden(shape):
    global _EXACT
    if _EXACT is None:
        _EXACT = np.load(GOLDEN + "/" + cs.EXACT_GOLDEN)
    k = cs.key_of(shape)
    return {f: _EXACT[k + "/" + f] for f in ("theta", "x", "sidx", "grad", "lap")}


@pytest.mark.parametrize("shape", cs.shapes_of("L0"), ids=lambda sh: _id(sh, "exact"))
def test_exact_mode(shape):
    """mode 0 against the oracle (n <= 7: at test time; above: its stored result, one walker), and against the sum over the n d
    basis probes of mode 2 (one batch of n d + 1 copies of the walker: the basis vectors and the zero probe)"""
    import torch
    dim, hs, ht, n = shape
    N = n * dim
    s = cs.inputs(shape, 1, cs.DERIV_WS)
    if n <= cs.EXACT_LIVE_MAX_N:
        R, rflow, rparams, r_logpsi = _oracle_fns(shape, s)
        _, rfn = R.make_logpsi_grad_laplacian(r_logpsi)
        gr, lr = rfn(R.T(s["x"]), rparams, torch.as_tensor(s["sidx"].astype(np.int64)))
        gr, lr = gr.numpy(), lr.numpy()
    else:
        g = _exact_golden(shape)
        assert np.array_equal(g["theta"], s["theta"])       # the generators still produce the stored flow
        s["x"], s["sidx"], gr, lr = g["x"], g["sidx"], g["grad"], g["lap"]
    eng = _engine(shape, s)
    print("%s mode 0: %s" % (shape, cs.SHAPES[shape]["L0"]))
    ge, le = eng.grad_laplacian(s["x"], s["sidx"], 0)
    _check("gradient", np.abs(ge - gr).max(), 1e-10 * max(1.0, np.abs(gr).max()))
    _check("Laplacian", np.abs(le - lr).max(), 1e-9 * max(1.0, np.abs(lr).max()))
    # mode 2 returns (probe-free part) + (probe terms of v): the zero probe (row N) gives the former, which the N basis calls each carry
    xs = np.repeat(s["x"], N + 1, axis=0); ss = np.repeat(s["sidx"], N + 1, axis=0)
    gh, lh = eng.grad_laplacian(xs, ss, 2, np.concatenate([np.eye(N), np.zeros((1, N))]).reshape(N + 1, n, dim))
    _check("sum of the basis probes", abs(lh[:N].sum() - (N - 1) * lh[N] - le[0]), 1e-9 * max(1.0, abs(le[0])))
    _check("gradient of the probe calls", np.abs(gh - ge).max(), 1e-10 * max(1.0, np.abs(ge).max()))
    eng.close()


@pytest.mark.parametrize("shape", cs.shapes_of("Q"), ids=lambda sh: _id(sh, "scores"))
def test_scores_param_vjp_and_fisher(shape):
    import torch
    from coulombgas_amd.flow import ravel_order
    dim, hs, ht, n = shape
    B = 3
    s = cs.inputs(shape, B, cs.DERIV_WS)
    x, sidx, theta = s["x"], s["sidx"], s["theta"]
    w_re, w_im = s["rng"].standard_normal(B), s["rng"].standard_normal(B)
    eng = _engine(shape, s)
    print("%s scores: %s" % (shape, cs.SHAPES[shape]["Q"]))
    R, rflow, rparams, r_logpsi = _oracle_fns(shape, s)
    sb = torch.as_tensor(sidx.astype(np.int64))
    lpt = lambda xb, th, sbb: r_logpsi(xb, R.flow_unravel(th, 2, hs, ht, dim), sbb)
    qr = R.make_quantum_score(lpt)(R.T(x), R.T(theta), sb).numpy()
    qs = eng.quantum_score(x, sidx)
    assert qs.shape == (B, sum(int(np.prod(shp)) for _, _, shp in ravel_order(2, hs, ht, dim)))
    _check("per-sample scores", np.abs(qs - qr).max(), 1e-10 * max(1.0, np.abs(qr).max()))

    def S(th):
        out = torch.stack([lpt(R.T(x[b]), th, sb[b]) for b in range(B)])
        return (R.T(w_re) * out[:, 0] + R.T(w_im) * out[:, 1]).sum()
    gr = torch.func.grad(S)(R.T(theta)).numpy()
    g = eng.param_vjp(x, sidx, w_re, w_im, use_scores=False)
    _check("theta-VJP", np.abs(g - gr).max(), 1e-10 * max(1.0, np.abs(gr).max()))
    g2 = eng.param_vjp(x, sidx, w_re, w_im)
    _check("theta-VJP from resident scores", np.abs(g2 - g).max(), 1e-11 * max(1.0, np.abs(g).max()))
    F, sm = eng.quantum_fisher(x, sidx)
    Fr = (qr.conj().T @ qr).real / B
    _check("Fisher matrix", np.abs(F - Fr).max(), 1e-10 * np.abs(Fr).max())
    _check("mean score", np.abs(sm - qr.mean(axis=0)).max(), 1e-10 * np.abs(qr).max())
    assert np.abs(F - F.T).max() == 0.0
    eng.close()


@pytest.mark.parametrize("shape", [(2, 8, 8, 24), (3, 16, 16, 23)], ids=lambda sh: _id(sh, "chunks"))
def test_second_launch_chunk(shape, monkeypatch):
    """k_grad_lap2<AL = false> and k_param_vjp at 512 threads held to ONE workgroup per CU and a launch (CG_LAP_PER_CU, CG_VJP_PER_CU = 1),
    a batch of cu_count + 3: the last three walkers go through a second launch that reuses the workspace slots of the first.  Their rows
    equal the same walkers evaluated alone, bit for bit."""
    monkeypatch.setenv("CG_LAP_PER_CU", "1")
    monkeypatch.setenv("CG_VJP_PER_CU", "1")
    fams = cs.paths(*shape)
    assert fams["L2"].startswith("ws") and fams["Q"].startswith("vjp512")      # the chunked kernels
    dim, hs, ht, n = shape
    s0 = cs.inputs(shape, 1, cs.DERIV_WS)
    eng = _engine(shape, s0)
    cu = eng.launch_info()["cu_count"]
    B = cu + 3
    s = cs.inputs(shape, B, cs.DERIV_WS)
    x, sidx = s["x"], s["sidx"]
    v = s["rng"].standard_normal(x.shape)
    g, l = eng.grad_laplacian(x, sidx, 2, v)
    gt, lt = eng.grad_laplacian(x[cu:], sidx[cu:], 2, v[cu:])
    assert np.isfinite(g).all() and np.isfinite(l).all()
    assert np.array_equal(g[cu:], gt) and np.array_equal(l[cu:], lt)
    g1, l1 = eng.grad_laplacian(x[:2], sidx[:2], 2, v[:2])
    assert np.array_equal(g[:2], g1) and np.array_equal(l[:2], l1)
    sc = eng.quantum_score(x, sidx)
    st = eng.quantum_score(x[cu:], sidx[cu:])
    assert np.isfinite(sc).all() and np.array_equal(sc[cu:], st)
    assert np.array_equal(sc[:2], eng.quantum_score(x[:2], sidx[:2]))
    eng.close()
