"""Momentum distribution on hardware (run with -m gpu): cg_displaced_ratios against the oracle, the known answers of the identity flow,
cg_momentum_sums against the numpy restatement (tests/momentum_ref.py), the reduction-order rule, non-finite walkers, the statistics of
the in-kernel shifts, the observable object and the limits."""
import numpy as np
import pytest

from tests import momentum_ref as MR
from tests.common import orbitals, box_length, flow_theta, state_indices, walkers

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _model(n, dim, hs, ht, B, seed=0, w_std=0.3, b_std=0.2, zero=False):
    import coulombgas_amd as cg
    L = box_length(n, dim)
    rng = np.random.default_rng(seed)
    sp = orbitals(dim)
    theta = flow_theta(rng, 2, hs, ht, dim, w_std, b_std)
    if zero:
        theta = np.zeros_like(theta)
    x = walkers(rng, B, n, dim, L)
    sidx = state_indices(rng, B, n, sp.shape[0])
    flow = cg.FermiNet(2, hs, ht, L)
    eng = flow.engine(n, dim, sp)
    eng.set_params(theta)
    return dict(n=n, dim=dim, hs=hs, ht=ht, L=L, sp=sp, theta=theta, x=x, sidx=sidx, flow=flow, eng=eng, rng=rng)


def _device(eng, x, sidx, shifts=None):
    from coulombgas_amd.engine import DeviceArray
    return (DeviceArray.from_numpy(eng, x), DeviceArray.from_numpy(eng, sidx, np.int32),
            None if shifts is None else DeviceArray.from_numpy(eng, shifts))


# ---- 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dim,hs,ht", [(5, 2, 16, 16), (13, 2, 16, 16), (7, 3, 4, 4), (29, 2, 16, 16),
                                         # k_displaced_ratios of the other configurations of the second translation unit, on the LU
                                         # paths of tests/config_shapes.py: fused and two-phase wave-level, sequential in one wave
                                         # and in four, the first-generation concurrent pair
                                         (13, 2, 8, 8), (5, 2, 32, 32), (8, 3, 16, 16), (11, 3, 8, 8), (27, 2, 4, 4), (23, 3, 16, 16)])
def test_ratios_against_the_oracle(n, dim, hs, ht):
    """|r / r_ref - 1| <= 2e-11 max(1, |Re log Psi|) with r_ref from the oracle's log Psi at the displaced and the base configuration
    (twice the bound test_gpu_parity.test_logpsi applies to one evaluation); both pointer modes give identical bits"""
    import torch
    from oracle import cg_ref as R
    B, S = 3, 2
    s = _model(n, dim, hs, ht, B)
    eng, L, x, sidx = s["eng"], s["L"], s["x"], s["sidx"]
    shifts = s["rng"].uniform(-1.0, 2.0, (B, S, n, dim))            # beyond one box length as well
    got, used = eng.displaced_ratios(x, sidx, S, shifts=shifts)
    assert got.shape == (B, S, n) and _same_bits(used, shifts)
    x_d, s_d, h_d = _device(eng, x, sidx, shifts)
    r_d, so_d = eng.displaced_ratios_d(x_d, s_d, S, shifts_d=h_d)
    assert _same_bits(np.asarray(r_d), got) and _same_bits(np.asarray(so_d), shifts)
    # the oracle, vmapped over the 1 + S n configurations of each walker
    rparams = R.flow_unravel(R.T(s["theta"]), 2, hs, ht, dim)
    logpsi = torch.func.vmap(R.make_logpsi(R.FermiNet(2, hs, ht, L), s["sp"], L), (0, None, None))
    worst = 0.0
    for b in range(B):
        conf = np.repeat(x[b][None], 1 + S * n, 0)
        for j in range(S):
            for i in range(n):
                conf[1 + j * n + i, i] += shifts[b, j, i] * L
        lp = logpsi(R.T(conf), rparams, torch.as_tensor(sidx[b].astype(np.int64))).numpy()
        ref = np.exp((lp[1:, 0] - lp[0, 0]) + 1j * (lp[1:, 1] - lp[0, 1])).reshape(S, n)
        scale = np.maximum(1.0, np.maximum(np.abs(lp[1:, 0]), abs(lp[0, 0]))).reshape(S, n)
        err = np.abs(got[b] / ref - 1.0) / scale
        worst = max(worst, float(err.max()))
    print("n=%d dim=%d (%d,%d): max |r / r_ref - 1| / max(1, |Re log Psi|) = %.3e" % (n, dim, hs, ht, worst))
    assert worst <= 2e-11


# ---- 2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 13])
def test_known_answer_identity_flow_regular_grid(n):
    """theta = 0 is the identity flow.  K = the whole (twisted) orbital table, shifts = the regular G^2 grid with G above every
    |component difference| between a table vector and an occupied orbital, the same for every particle and walker: the per-walker
    n_k^(b) is the occupation of k in walker b (1e-10), sum_k n_k^(b) = n, and sum_i r(i, s) = sum_j e^{2 pi i k_j.s}.
    Measured on an MI355X: see the printed maxima (recorded in DESIGN.md)."""
    dim, B = 2, 16
    s = _model(n, dim, 16, 16, B, seed=n, zero=True)
    eng, sp, x, sidx = s["eng"], s["sp"], s["x"], s["sidx"]
    kocc = sp[sidx]
    G = MR.grid_size(sp, kocc)
    grid = MR.regular_grid(G, dim)
    S = G * G
    shifts = np.ascontiguousarray(np.broadcast_to(grid[None, :, None, :], (B, S, n, dim)))
    ratios, _ = eng.displaced_ratios(x, sidx, S, shifts=shifts)
    occ = MR.occupation(sp, kocc)
    assert (occ.sum(1) == n).all() and (sidx != np.arange(sp.shape[0] - n, sp.shape[0])).any()        # excited states among them
    nk, dropped = MR.per_walker(ratios, shifts, sp)
    e_ratio = np.abs(nk - occ).max()
    rows = np.exp(2j * np.pi * np.einsum("sd,bjd->bsj", grid, kocc)).sum(-1)
    e_rows = np.abs(ratios.sum(-1) - rows).max()
    # ... and through the reduction kernel, one walker per call
    eng.set_momentum(sp)
    nK = sp.shape[0]
    e_call = 0.0
    for b in range(0, B, 5):
        out = eng.momentum_sums(x[b:b + 1], sidx[b:b + 1], S, shifts=shifts[b:b + 1])
        assert out[3 * nK] == 0 and out[3 * nK + 1] == 1
        e_call = max(e_call, np.abs(out[0:2 * nK:2] - occ[b]).max(), np.abs(out[1:2 * nK:2]).max(), np.abs(out[2 * nK:3 * nK] - occ[b]).max())
        assert abs(out[0:2 * nK:2].sum() - n) <= 1e-10 * n
    print("n=%d G=%d: max |n_k^(b) - occupation| = %.2e from the ratios, %.2e through cg_momentum_sums; max |sum_i r - sum_j e^{iks}| = %.2e"
          % (n, G, e_ratio, e_call, e_rows))
    assert dropped.sum() == 0
    assert e_ratio <= 1e-10 and e_call <= 1e-10 and e_rows <= 1e-10
    assert np.abs(nk.sum(1) - n).max() <= 1e-10 * n


# ---- 3 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,B", [(13, 1500), (29, 64)])
def test_sums_against_numpy(n, B):
    """cg_momentum_sums = the numpy restatement applied to the ratios and shifts of cg_displaced_ratios (same seed and offset), within
    1e-12 n B; dropped and count exactly.  B = 1500 crosses the 1024-row rule."""
    dim, S = 2, 2
    s = _model(n, dim, 16, 16, B, seed=3, w_std=0.05, b_std=0.02)
    eng, sp, x, sidx = s["eng"], s["sp"], s["x"], s["sidx"]
    K = sp[-40:]
    nK = K.shape[0]
    eng.set_momentum(K)
    assert eng.momentum_size() == 3 * nK + 2
    ratios, shifts = eng.displaced_ratios(x, sidx, S, seed=77, walker_offset=5)
    ref = MR.momentum_ref(ratios, shifts, K)
    host = eng.momentum_sums(x, sidx, S, seed=77, walker_offset=5)
    err = np.abs(host[:3 * nK] - ref[:3 * nK]).max()
    print("n=%d B=%d: max |sums - numpy| = %.3e (bound %.3e); largest |ratio| %.3e" % (n, B, err, 1e-12 * n * B, np.abs(ratios).max()))
    assert err <= 1e-12 * n * B
    assert host[3 * nK] == ref[3 * nK] == 0 and host[3 * nK + 1] == B
    x_d, s_d, _ = _device(eng, x, sidx)
    assert _same_bits(np.asarray(eng.momentum_sums_d(x_d, s_d, S, seed=77, walker_offset=5)), host)
    # supplied shifts go the same way
    sup = eng.momentum_sums(x, sidx, S, shifts=shifts)
    assert _same_bits(sup, host)
    assert np.array_equal(eng.momentum_sums(x[:0], sidx[:0], S), np.zeros(3 * nK + 2))


# ---- 4 -------------------------------------------------------------------------------------------------------------------------
def test_reproducibility_and_philox_shifts(monkeypatch):
    n, dim, B, S = 13, 2, 1500, 2
    s = _model(n, dim, 16, 16, B, seed=4, w_std=0.05, b_std=0.02)
    eng, sp, x, sidx = s["eng"], s["sp"], s["x"], s["sidx"]
    eng.set_momentum(sp[-30:])
    a = eng.momentum_sums(x, sidx, S, seed=1)
    assert _same_bits(a, eng.momentum_sums(x, sidx, S, seed=1))
    for grid in (1000, 37):
        monkeypatch.setenv("CG_MOMENTUM_GRID", str(grid))
        assert _same_bits(a, eng.momentum_sums(x, sidx, S, seed=1)), grid
    monkeypatch.delenv("CG_MOMENTUM_GRID")
    # Philox mode: the drawn shifts, fed back as supplied ones, reproduce the ratios bit for bit
    r1, sh1 = eng.displaced_ratios(x[:64], sidx[:64], S, seed=1, walker_offset=10)
    r2, sh2 = eng.displaced_ratios(x[:64], sidx[:64], S, shifts=sh1)
    assert _same_bits(r1, r2) and _same_bits(sh1, sh2)
    assert sh1.min() >= 0.0 and sh1.max() < 1.0
    assert abs(sh1.mean() - 0.5) < 5.0 / np.sqrt(12.0 * sh1.size)
    # walker b at offset o draws what walker b + 1 draws at offset o - 1; another offset or seed gives other shifts
    _, sh3 = eng.displaced_ratios(x[:64], sidx[:64], S, seed=1, walker_offset=11)
    assert _same_bits(sh3[:-1], sh1[1:]) and not np.array_equal(sh3, sh1)
    _, sh4 = eng.displaced_ratios(x[:64], sidx[:64], S, seed=2, walker_offset=10)
    assert not np.array_equal(sh4, sh1) and len(np.unique(sh1)) == sh1.size


# ---- 5 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [13, 29])
def test_a_nan_walker_and_coincident_electrons(n):
    """one walker with a NaN coordinate, one with two electrons at the same place: the call returns, the NaN walker's M terms are counted in
    `dropped`, the other walkers' ratios are bitwise those of the clean batch"""
    dim, B, S = 2, 8, 2
    s = _model(n, dim, 16, 16, B, seed=6, w_std=0.05, b_std=0.02)
    eng, sp, x, sidx = s["eng"], s["sp"], s["x"], s["sidx"]
    shifts = s["rng"].uniform(size=(B, S, n, dim))
    clean, _ = eng.displaced_ratios(x, sidx, S, shifts=shifts)
    assert np.isfinite(clean.view(np.float64)).all()
    xb = x.copy()
    xb[2, 3, 1] = np.nan
    xb[5, 4] = xb[5, 1]
    got, _ = eng.displaced_ratios(xb, sidx, S, shifts=shifts)              # CG_OK: anything else raises
    others = [b for b in range(B) if b not in (2, 5)]
    assert _same_bits(got[others], clean[others])
    assert not np.isfinite(got[2].view(np.float64)).any()
    eng.set_momentum(sp[-20:])
    out = eng.momentum_sums(xb, sidx, S, shifts=shifts)
    bad5 = int((~(np.isfinite(got[5].real) & np.isfinite(got[5].imag))).sum())
    print("n=%d: coincident pair: %d of %d terms not finite" % (n, bad5, S * n))
    assert out[-1] == B and out[-2] == S * n + bad5
    ref = MR.momentum_ref(got, shifts, sp[-20:])
    assert out[-2] == ref[-2] and np.isfinite(out).all()
    # the finite terms still sum as in numpy (linear entries; 1e-12 n B per unit of the largest finite |ratio|)
    fin = np.abs(got[np.isfinite(got.real) & np.isfinite(got.imag)]).max()
    assert np.abs(out[:40] - ref[:40]).max() <= 1e-12 * n * B * max(1.0, fin)


# ---- 6 -------------------------------------------------------------------------------------------------------------------------
def test_statistics_in_philox_mode():
    """theta = 0, n = 13, B = 4096, S = 2 in-kernel shifts per particle, walkers from cg.mcmc as in test_ideal_fermi_gas_structure_factor
    (closed shell, untwisted table, 20 calls of 50 steps at width 0.3): every n_k of the 81 table vectors lies within 5 of the
    observable's own standard errors of the occupation marginal of the batch (1 on the closed shell, 0 elsewhere).  The bound is the one
    tests/test_momentum_host.py verifies for numpy ratios."""
    import coulombgas_amd as cg
    from coulombgas_amd.engine import DeviceArray
    n, dim, B, steps, stddev = 13, 2, 4096, 50, 0.3
    L = box_length(n, dim)
    idx, _ = cg.sp_orbitals(dim, 25)
    sp = idx.astype(np.float64)
    flow = cg.FermiNet(2, 16, 16, L)
    eng = flow.engine(n, dim, sp)
    theta = np.zeros(eng.P)
    sidx = np.tile(np.arange(n, dtype=np.int32), (B, 1))
    logp = cg.make_logp(cg.make_logpsi(flow, sp, L))
    x = DeviceArray.from_numpy(eng, np.random.default_rng(1).uniform(0.0, L, (B, n, dim)))
    rates = []
    for call in range(20):
        _, rate = cg.mcmc(logp.bind(theta, sidx), x, 1000 + call, steps, stddev, wrap_L=L)
        rates.append(rate)
    obs = cg.make_momentum_observable(n, dim, L, sp, shifts_per_particle=2, seed=12345, engine=eng)
    r = obs.accumulate(x, sidx).result()
    occ = MR.occupation(sp, sp[sidx[:1]])[0]
    z = np.abs(r["n_k"] - occ) / r["stderr"]
    print("accept rate %.3f; max |n_k - occupation| / stderr = %.2f at k = %s (n_k %.4f, stderr %.4f); sum_k n_k = %.4f; dropped %d; "
          "largest |Im n_k| %.2e" % (np.mean(rates), z.max(), sp[z.argmax()], r["n_k"][z.argmax()], r["stderr"][z.argmax()], r["n_k"].sum(),
                                     r["dropped"], np.abs(r["n_k_imag"]).max()))
    assert r["count"] == B and r["dropped"] == 0 and occ.sum() == n
    assert z.max() <= 5.0


# ---- 7 -------------------------------------------------------------------------------------------------------------------------
def test_observable_object_on_device_and_host_arrays():
    """device and host batches into one accumulator = one numpy sum over the four batches' own ratios; psum_d on a world of one"""
    import coulombgas_amd as cg
    from coulombgas_amd.comm import RcclComm
    n, dim, B, S = 13, 2, 64, 2
    s = _model(n, dim, 16, 16, 4 * B, seed=8, w_std=0.05, b_std=0.02)
    eng, sp, x, sidx, L = s["eng"], s["sp"], s["x"], s["sidx"], s["L"]
    K = sp[-25:]
    nK = K.shape[0]
    comm = RcclComm(eng, 0, 1)
    obs = cg.make_momentum_observable(n, dim, L, K, shifts_per_particle=S, seed=31, comm=comm, engine=eng)
    total = np.zeros(3 * nK + 2)
    for q in range(4):
        xq, sq = x[q * B:(q + 1) * B], sidx[q * B:(q + 1) * B]
        ratios, shifts = eng.displaced_ratios(xq, sq, S, seed=31, walker_offset=q * B)
        total += MR.momentum_ref(ratios, shifts, K)
        if q % 2:
            x_d, s_d, _ = _device(eng, xq, sq)
            obs.accumulate(x_d, s_d)
        else:
            obs.accumulate(xq, sq)
    h = obs.sums()
    assert h[-1] == 4 * B and h[-2] == total[-2] and np.abs(h[:3 * nK] - total[:3 * nK]).max() <= 1e-12 * n * 4 * B
    r = obs.result()
    assert r["count"] == 4 * B and np.abs(r["n_k"] - total[0:2 * nK:2] / (4 * B)).max() <= 1e-12 * n
    var = total[2 * nK:3 * nK] / (4 * B) - (total[0:2 * nK:2] / (4 * B)) ** 2
    assert np.allclose(r["stderr"], np.sqrt(var / (4 * B - 1)), rtol=1e-9)
    # one batch, device against host arrays: the same bits
    one_h = cg.make_momentum_observable(n, dim, L, K, shifts_per_particle=S, seed=31, engine=eng).accumulate(x[:B], sidx[:B]).sums()
    x_d, s_d, _ = _device(eng, x[:B], sidx[:B])
    one_d = cg.make_momentum_observable(n, dim, L, K, shifts_per_particle=S, seed=31, engine=eng).accumulate(x_d, s_d).sums()
    assert _same_bits(one_h, one_d)
    comm.close()


def test_training_accumulates_without_changing_the_run():
    """train(momentum=obs): the data.txt rows and parameters of the run are those of the run without it, bit for bit; the accumulator
    holds epochs x acc_steps batches"""
    import coulombgas_amd as cg
    n, dim = 13, 2
    L = box_length(n, dim)
    sp = orbitals(dim)
    out = {}
    for name in ("plain", "momentum"):
        flow = cg.FermiNet(2, 16, 16, L)
        obs = cg.make_momentum_observable(n, dim, L, sp[-30:], seed=5) if name == "momentum" else None
        samp = cg.GroundStateSampler(n, sp.shape[0])
        p0 = flow.init(3, np.zeros((n, dim)))
        pv, pf, rows = cg.train(flow, p0, sp, n, dim, L, rs=10.0, beta=1 / (4 * 0.15), batch=256, epochs=2, sampler=samp,
                                log_prob=samp.log_prob, sr=(1e-3, 1e-3), mc_therm=2, mc_steps=10, acc_steps=2, seed=11, momentum=obs)
        out[name] = (rows, flow.ravel(pf, dim))
    assert out["plain"][0] == out["momentum"][0] and np.array_equal(out["plain"][1], out["momentum"][1])
    r = obs.result()
    assert r["count"] == 2 * 2 * 256 and obs.offset == r["count"] and np.isfinite(r["n_k"]).all()
    # ground-state sampler, nearly the identity flow: the 13 occupied orbitals (the last rows of the table) stand out
    print("train: n_k of the occupied rows %.3f .. %.3f, of the others %.3f .. %.3f" % (r["n_k"][-13:].min(), r["n_k"][-13:].max(),
                                                                                       r["n_k"][:-13].min(), r["n_k"][:-13].max()))


# ---- 8 -------------------------------------------------------------------------------------------------------------------------
def test_limits():
    import coulombgas_amd as cg
    from coulombgas_amd._lib import CoulombGasError
    n, dim = 5, 2
    L = box_length(n, dim)
    sp = orbitals(dim)
    rng = np.random.default_rng(0)
    x, sidx = walkers(rng, 2, n, dim, L), state_indices(rng, 2, n, sp.shape[0])

    def code(fn):
        with pytest.raises(CoulombGasError) as ei:
            fn()
        return ei.value.code, str(ei.value)

    eng = cg.Engine(n, dim, 2, 16, 16, L, sp)
    assert code(lambda: eng.displaced_ratios(x, sidx, 1))[0] == -4           # no flow parameters
    assert code(lambda: eng.momentum_size())[0] == -4
    eng.set_params(np.zeros(eng.P))
    assert code(lambda: eng.momentum_sums(x, sidx, 1))[0] == -4              # no cg_set_momentum
    assert code(lambda: eng.displaced_ratios(x, sidx, 0))[0] == -1
    assert code(lambda: eng.set_momentum(np.array([[np.inf, 0.0]])))[0] == -1
    assert code(lambda: eng.set_momentum(np.zeros((0, 2))))[0] == -1
    from coulombgas_amd._lib import lib
    assert lib().cg_displaced_ratios(eng._ctx, None, None, 2, 1, None, 0, 0, None, None) == -1
    assert lib().cg_set_momentum(eng._ctx, None, 3) == -1
    eng.set_momentum(sp[:4])
    assert eng.momentum_size() == 14
    assert code(lambda: eng.momentum_sums(x, sidx, 0))[0] == -1
    assert lib().cg_momentum_sums(eng._ctx, None, None, 2, 1, None, 0, 0, None) == -1
    assert eng.momentum_sums(x, sidx, 1)[-1] == 2
    eng.close()
    deep = cg.Engine(n, dim, 3, 16, 16, L, sp)
    deep.set_params(np.zeros(deep.P))
    c, msg = code(lambda: deep.displaced_ratios(x, sidx, 1))
    assert c == -3 and "depth" in msg
    deep.set_momentum(sp[:4])
    assert code(lambda: deep.momentum_sums(x, sidx, 1))[0] == -3
    deep.close()
