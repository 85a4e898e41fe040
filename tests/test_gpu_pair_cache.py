"""GPU tests of the n = 13 sampler's pair cache (k_mcmc<2,16,16,64,13>: the pair-primal pass keeps sigmoid(u_ij[h]) in registers and the
Jacobian pair loop takes it from there instead of recomputing u and its exponential).  The separate log Psi kernel (k_logpsi) does not
use the cache, so a Metropolis chain driven from Python through it with the same draws is an independent statement of the same chain."""
import numpy as np
import pytest
import torch

from tests.common import orbitals, box_length, flow_theta, state_indices, walkers

pytestmark = pytest.mark.gpu


def _inputs(n, B, seed, w_std=0.3, b_std=0.2):
    import coulombgas_amd as cg
    L = box_length(n, 2)
    rng = np.random.default_rng(seed)
    sp = orbitals(2)
    theta = flow_theta(rng, 2, 16, 16, 2, w_std, b_std)
    x = walkers(rng, B, n, 2, L)
    sidx = state_indices(rng, B, n, sp.shape[0])
    return dict(n=n, L=L, sp=sp, theta=theta, x=x, sidx=sidx, rng=rng, flow=cg.FermiNet(2, 16, 16, L))


def _python_chain(eng, x, sidx, noise, unif, std):
    """src/MCMC.py:22-39 with every log-probability from the separate log Psi kernel; the accept rule of the fused kernel."""
    x = x.copy()
    logp = eng.logp(x, sidx)
    nacc = 0
    for s in range(noise.shape[0]):
        xp = x + std * noise[s]
        lp = eng.logp(xp, sidx)
        d = lp - logp
        with np.errstate(over="ignore", invalid="ignore"):
            acc = (d >= 0.0) | ((d > -745.0) & (unif[s] < np.exp(np.minimum(d, 0.0))))
        x[acc] = xp[acc]
        logp = np.where(acc, lp, logp)
        nacc += int(acc.sum())
    return x, logp, nacc


@pytest.mark.parametrize("n", [13, 12, 16])
def test_fused_chain_equals_chain_through_the_logpsi_kernel(n):
    """n = 13: the specialised kernel with the pair cache; n = 12, 16: the size-generic single-wave kernel (unchanged path).
    Same accept decisions, same walkers, log-probabilities to the 1e-10 of the bookkeeping check in test_mcmc_philox_statistics."""
    s = _inputs(n, 96, seed=21)
    eng = s["flow"].engine(n, 2, s["sp"])
    eng.set_params(s["theta"])
    assert eng.launch_info()["threads"] == 64
    steps, std = 24, 0.1
    noise = s["rng"].standard_normal((steps,) + s["x"].shape)
    unif = s["rng"].uniform(size=(steps, s["x"].shape[0]))
    xf, lpf, nacc = eng.mcmc(s["x"], s["sidx"], steps, std, noise=noise, unif=unif)
    xr, lpr, nacc_r = _python_chain(eng, s["x"], s["sidx"], noise, unif, std)
    print("n=%d: accepts %d / %d (python chain %d), max |dx| %.3e, max |dlogp| %.3e"
          % (n, nacc, steps * 96, nacc_r, np.abs(xf - xr).max(), np.abs(lpf - lpr).max()))
    assert 0 < nacc < steps * 96
    assert nacc == nacc_r
    assert np.abs(xf - xr).max() < 1e-12
    assert np.abs(lpf - lpr).max() < 1e-10
    assert np.abs(lpf - eng.logp(xf, s["sidx"])).max() < 1e-10


def test_saturated_two_particle_units_against_oracle():
    """Two-particle pre-activations beyond |u| = 40 in both signs (e^-|u| ~ 1e-18 .. 1e-27: 1 + e rounds to 1, sigmoid -> 1 or e):
    the log-probability the n = 13 chain ends on against the oracle at the 1e-11 of test_logpsi."""
    from oracle import cg_ref as R
    n, B = 13, 8
    s = _inputs(n, B, seed=22)
    theta = s["theta"].copy()
    P, HT = 5, 16
    tb = theta[-(P + 1) * HT:-P * HT]                       # tp0.b, then tp0.w (P x HT) close the parameter vector
    tb[:] = np.where(np.arange(HT) % 2 == 0, 50.0, -50.0)
    tb[6:8] = 0.0                                           # two units stay in the ordinary range
    tw = theta[-P * HT:].reshape(P, HT)
    L = s["L"]
    r = s["x"][0][:, None, :] - s["x"][0][None, :, :]
    feat = np.concatenate([np.cos(2 * np.pi * r / L), np.sin(2 * np.pi * r / L),
                           np.sqrt((np.sin(np.pi * r / L) ** 2).sum(-1, keepdims=True))], axis=-1)
    u = feat @ tw + tb
    assert u.max() > 40.0 and u.min() < -40.0
    eng = s["flow"].engine(n, 2, s["sp"])
    eng.set_params(theta)
    steps, std = 6, 0.1
    noise = s["rng"].standard_normal((steps,) + s["x"].shape)
    unif = s["rng"].uniform(size=(steps, B))
    xf, lpf, nacc = eng.mcmc(s["x"], s["sidx"], steps, std, noise=noise, unif=unif)
    rflow = R.FermiNet(2, 16, 16, L)
    rparams = R.flow_unravel(R.T(theta), 2, 16, 16, 2)
    r_logpsi = R.make_logpsi(rflow, s["sp"], L)
    for b in range(B):
        ref = r_logpsi(R.T(xf[b]), rparams, torch.as_tensor(s["sidx"][b].astype(np.int64))).numpy()
        print("walker %d: logp %.15e, oracle %.15e, diff %.3e" % (b, lpf[b], 2 * ref[0], lpf[b] - 2 * ref[0]))
        assert abs(lpf[b] - 2 * ref[0]) < 2e-11 * max(1.0, abs(ref[0]))
    assert np.isfinite(lpf).all()
