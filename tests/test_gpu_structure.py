"""Structure observables on hardware (run with -m gpu): cg_structure_sums against the numpy restatement (tests/structure_ref.py) in both
pointer modes, conservation, the reduction-order rule of csrc/cg_structure.hpp, accumulation on the device, a NaN walker, and the
exactly known S(k) of the ideal Fermi gas."""
import numpy as np
import pytest

from tests.common import box_length
from tests.structure_ref import SHAPES, seeded_walkers, kgrid, pair_t, edge_gap, structure_ref

pytestmark = pytest.mark.gpu

NBINS, RMAX = 128, 0.5
PARITY = SHAPES + ((29, 2, 2048, box_length(29, 2)),)


def _engine(n, dim, L, K=None, nbins=NBINS, rmax=RMAX):
    import coulombgas_amd as cg
    eng = cg.Engine(n, dim, 2, 16, 16, L)
    if K is not None:
        eng.set_structure(K, nbins, rmax)
    return eng


def _check(got, ref, n, B, nK, tol=1e-12):
    err = np.abs(got[:3 * nK] - ref[:3 * nK]).max() / (n * n * B)
    print("max |rho sums - numpy| / (n^2 B) = %.3e" % err)
    assert err <= tol
    assert np.array_equal(got[3 * nK:], ref[3 * nK:])


@pytest.mark.parametrize("n,dim,B,L", PARITY)
def test_parity_with_numpy_in_both_pointer_modes_and_conservation(n, dim, B, L):
    """|rho|^2 and rho sums to 1e-12 of n^2 B, every histogram bin and the overflow exactly (no pair of the seeded inputs has t within
    1e-9 of a bin edge: asserted, no pair excluded)"""
    from coulombgas_amd.engine import DeviceArray
    K = kgrid(dim)
    nK = K.shape[0]
    x = seeded_walkers(n, dim, B, L)
    gap = edge_gap(pair_t(x, L, NBINS, RMAX))
    print("n=%d dim=%d B=%d nK=%d: smallest gap to a bin edge %.3e" % (n, dim, B, nK, gap))
    assert gap >= 1e-9
    ref = structure_ref(x, L, K, NBINS, RMAX)
    eng = _engine(n, dim, L, K)
    assert eng.structure_size() == 3 * nK + NBINS + 2
    host = eng.structure_sums(x)
    _check(host, ref, n, B, nK)
    dev = np.asarray(eng.structure_sums_d(DeviceArray.from_numpy(eng, x)))
    _check(dev, ref, n, B, nK)
    assert np.array_equal(host, dev)
    # conservation: every pair is in exactly one counter, the count is B, |rho_0|^2 = n^2
    assert host[3 * nK:-1].sum() == B * n * (n - 1) // 2 and host[-1] == B
    assert abs(host[0] - B * n * n) <= 1e-12 * B * n * n
    assert np.array_equal(eng.structure_sums(x[:0]), np.zeros(3 * nK + NBINS + 2))
    eng.close()


def test_reduction_order(monkeypatch):
    """two calls agree bit for bit; so do launches with other numbers of workgroups; a batch split over two calls reproduces the
    histogram exactly and the rho sums to reassociation error (1e-13 relative)"""
    n, dim, B = 29, 2, 2048
    L = box_length(n, dim)
    K = kgrid(dim)
    nK = K.shape[0]
    x = seeded_walkers(n, dim, B, L)
    eng = _engine(n, dim, L, K)
    a = eng.structure_sums(x)
    assert np.array_equal(a, eng.structure_sums(x))
    for grid in (1000, 37):
        monkeypatch.setenv("CG_STRUCT_GRID", str(grid))
        assert np.array_equal(a, eng.structure_sums(x)), grid
    monkeypatch.delenv("CG_STRUCT_GRID")
    s = eng.structure_sums(x[:1024]) + eng.structure_sums(x[1024:])
    assert np.array_equal(s[3 * nK:], a[3 * nK:])
    err = np.abs(s[:3 * nK] - a[:3 * nK]).max() / (n * n * B)
    print("split-and-add: max |difference| / (n^2 B) = %.3e" % err)
    assert err <= 1e-13
    eng.close()


def test_accumulation_on_the_device_and_psum():
    from coulombgas_amd.comm import RcclComm
    from coulombgas_amd.engine import DeviceArray
    n, dim, B, L = SHAPES[0]
    K = kgrid(dim)
    nK = K.shape[0]
    eng = _engine(n, dim, L, K)
    size = eng.structure_size()
    acc = DeviceArray.from_numpy(eng, np.zeros(size))
    total = np.zeros(size)
    for i in range(4):
        x = seeded_walkers(n, dim, B, L, seed=100 + i)
        total += eng.structure_sums(x)
        assert eng.structure_sums_d(DeviceArray.from_numpy(eng, x), acc) is acc
    got = np.asarray(acc)
    assert np.array_equal(got[3 * nK:], total[3 * nK:]) and got[-1] == 4 * B
    assert np.abs(got[:3 * nK] - total[:3 * nK]).max() <= 1e-13 * n * n * 4 * B
    comm = RcclComm(eng, 0, 1)
    v0 = acc.version
    assert comm.psum_d(acc) is acc and acc.version == v0 + 1 and np.array_equal(np.asarray(acc), got)
    comm.psum_d(acc, count=NBINS + 2, index=3 * nK)
    assert np.array_equal(np.asarray(acc), got)
    with pytest.raises(IndexError):
        comm.psum_d(acc, count=size + 1)
    comm.close(); eng.close()


def test_observable_object_on_device_and_host_arrays():
    """make_structure_observable end to end: DeviceArray and numpy batches into one accumulator, normalised as documented"""
    import coulombgas_amd as cg
    from coulombgas_amd.engine import DeviceArray
    n, dim, B, L = SHAPES[2]
    K = kgrid(dim)
    nK = K.shape[0]
    eng = _engine(n, dim, L)
    x = seeded_walkers(n, dim, B, L)
    obs = cg.make_structure_observable(n, dim, L, K, nbins=NBINS, rmax=RMAX, engine=eng)
    obs.accumulate(DeviceArray.from_numpy(eng, x[:40])).accumulate(x[40:])
    r = obs.result()
    ref = structure_ref(x, L, K, NBINS, RMAX)
    assert r["count"] == B and np.array_equal(r["hist"], ref[3 * nK:3 * nK + NBINS]) and r["overflow"] == ref[3 * nK + NBINS]
    assert np.abs(r["S"] - ref[:nK] / (n * B)).max() <= 1e-12 * n
    assert np.abs(r["rho"] - (ref[nK:3 * nK:2] + 1j * ref[nK + 1:3 * nK:2]) / B).max() <= 1e-12 * n
    edges = RMAX * L * np.arange(NBINS + 1) / NBINS
    shell = 4 * np.pi / 3 * np.diff(edges ** 3)
    assert np.allclose(r["g"], r["hist"] * L ** 3 / (B * n * (n - 1) / 2 * shell), rtol=1e-14)
    assert np.array_equal(obs.result()["hist"], r["hist"])
    eng.close()


def test_a_nan_walker_is_counted_and_contained():
    n, dim, B, L = SHAPES[0]
    K = kgrid(dim)
    nK = K.shape[0]
    x = seeded_walkers(n, dim, B, L)
    x[77, 5, 1] = np.nan
    eng = _engine(n, dim, L, K)
    out = eng.structure_sums(x)                      # CG_OK: anything else raises
    assert out[3 * nK:-1].sum() == B * n * (n - 1) // 2 and out[-1] == B
    assert np.array_equal(out[3 * nK:], structure_ref(x, L, K, NBINS, RMAX)[3 * nK:])
    ky = K[:, 1] != 0                                # the NaN coordinate enters every k with a y component (k_y = 0 reads table entry 0)
    assert np.isnan(out[:nK][ky]).all() and np.isnan(out[nK:3 * nK:2][ky]).all() and np.isnan(out[nK + 1:3 * nK:2][ky]).all()
    eng.close()


def test_limits():
    from coulombgas_amd._lib import CoulombGasError
    eng = _engine(57, 2, 13.38)
    with pytest.raises(CoulombGasError) as ei:
        eng.structure_sums(np.zeros((1, 57, 2)))
    assert ei.value.code == -4
    with pytest.raises(CoulombGasError) as ei:
        eng.set_structure(np.array([[100, 0]]), 256, 0.5)        # 57 * 2 * 101 * 16 bytes of tables
    assert ei.value.code == -3 and "LDS" in str(ei.value)
    with pytest.raises(CoulombGasError) as ei:
        eng.set_structure(kgrid(2), 128, 0.6)
    assert ei.value.code == -1
    eng.set_structure(kgrid(2), 256, 0.5)                        # kpoints(2, 15) at n = 57 with 256 bins fits
    assert eng.structure_size() == 3 * kgrid(2).shape[0] + 258      # kpoints keeps 0 < |k|^2 <= 15^2: 708 vectors, + k = 0
    eng.close()
    eng = _engine(14, 3, 3.9, kgrid(3), nbins=256)               # kpoints(3, 7) at n = 14
    assert eng.structure_sums(seeded_walkers(14, 3, 8, 3.9))[-1] == 8
    eng.close()


def test_training_accumulates_without_changing_the_run():
    """train(structure=obs): the rows and parameters of the run are those of the run without it, bit for bit; the accumulator holds
    epochs x acc_steps batches"""
    import coulombgas_amd as cg
    from tests.common import orbitals
    n, dim = 13, 2
    L = box_length(n, dim)
    sp = orbitals(dim)
    out = {}
    for name in ("plain", "structure"):
        flow = cg.FermiNet(2, 16, 16, L)
        obs = cg.make_structure_observable(n, dim, L, kgrid(dim), nbins=64) if name == "structure" else None
        samp = cg.GroundStateSampler(n, sp.shape[0])
        p0 = flow.init(3, np.zeros((n, dim)))
        pv, pf, rows = cg.train(flow, p0, sp, n, dim, L, rs=10.0, beta=1 / (4 * 0.15), batch=256, epochs=2, sampler=samp,
                                log_prob=samp.log_prob, sr=(1e-3, 1e-3), mc_therm=2, mc_steps=10, acc_steps=2, seed=11, structure=obs)
        out[name] = (rows, flow.ravel(pf, dim))
    assert out["plain"][0] == out["structure"][0] and np.array_equal(out["plain"][1], out["structure"][1])
    r = obs.result()
    assert r["count"] == 2 * 2 * 256 and r["hist"].sum() + r["overflow"] == r["count"] * n * (n - 1) // 2
    assert abs(r["S"][0] - n) < 1e-12 * n and np.isfinite(r["g"]).all()


def test_ideal_fermi_gas_structure_factor():
    """Known answer: ideal spin-polarised Fermi gas, n = 13, dim = 2, identity flow (theta = 0), closed-shell ground state, no twist.
    For integer k != 0, S(k) = 1 - (1/n) #{p in Omega : p + k in Omega}, Omega the occupied orbital vectors (only the exchange term
    survives).  In-kernel RNG, fixed seeds, B = 4096, 20 equilibration calls of 50 steps, then 16 measured batches one 50-step call
    apart; for all k with |k|^2 <= 16: max_k |mean - exact| / stderr <= 5 with stderr = scatter of the 16 batch means / 4, and the
    real and imaginary parts of <rho_k> within 5 standard errors of 0 (translation invariance).
    Largest z observed on an MI355X: 2.62 for S(k) (at k = (-3, 1); max |S - exact| = 7.0e-3), 2.55 / 2.51 for Re / Im <rho_k>; accept rate
    0.246 at the proposal width 0.3.  The equilibration was not changed from the 20 calls above."""
    import coulombgas_amd as cg
    from coulombgas_amd.engine import DeviceArray
    n, dim, B, steps, stddev = 13, 2, 4096, 50, 0.3
    L = box_length(n, dim)
    idx, _ = cg.sp_orbitals(dim, 25)
    sp = idx.astype(np.float64)
    occ = {tuple(int(v) for v in p) for p in idx[:n]}
    assert sorted((np.array(sorted(occ)) ** 2).sum(-1))[-1] == 4 and len(occ) == 13          # shells |p|^2 = 0, 1, 2, 4: closed
    K = np.array([(a, b) for a in range(-4, 5) for b in range(-4, 5) if 0 < a * a + b * b <= 16], dtype=np.int64)
    exact = np.array([1.0 - sum((p[0] + k[0], p[1] + k[1]) in occ for p in occ) / n for k in K])
    nK = K.shape[0]
    flow = cg.FermiNet(2, 16, 16, L)
    eng = flow.engine(n, dim, sp)
    eng.set_structure(K, NBINS, RMAX)
    theta = np.zeros(eng.P)
    sidx = np.tile(np.arange(n, dtype=np.int32), (B, 1))
    logp = cg.make_logp(cg.make_logpsi(flow, sp, L))
    x = DeviceArray.from_numpy(eng, np.random.default_rng(1).uniform(0.0, L, (B, n, dim)))
    call, rates = 0, []
    def advance():
        nonlocal call
        call += 1
        _, rate = cg.mcmc(logp.bind(theta, sidx), x, 1000 + call, steps, stddev, wrap_L=L)
        rates.append(rate)
    for _ in range(20):
        advance()
    S, re, im = [], [], []
    for _ in range(16):
        advance()
        o = np.asarray(eng.structure_sums_d(x))
        assert o[-1] == B
        S.append(o[:nK] / (n * B)); re.append(o[nK:3 * nK:2] / B); im.append(o[nK + 1:3 * nK:2] / B)
    S, re, im = np.array(S), np.array(re), np.array(im)
    se = lambda a: a.std(axis=0, ddof=1) / 4.0
    z = np.abs(S.mean(0) - exact) / se(S)
    zr, zi = np.abs(re.mean(0)) / se(re), np.abs(im.mean(0)) / se(im)
    print("ideal gas S(k): accept rate %.3f, max z = %.2f (k = %s), max |S - exact| = %.2e, max z of Re/Im <rho_k> = %.2f / %.2f"
          % (np.mean(rates), z.max(), K[z.argmax()], np.abs(S.mean(0) - exact).max(), zr.max(), zi.max()))
    assert z.max() <= 5.0
    assert zr.max() <= 5.0 and zi.max() <= 5.0
