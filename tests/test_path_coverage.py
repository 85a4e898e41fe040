"""CPU guard of the GPU tests of the second translation unit's flow configurations (tests/test_gpu_configs.py): every kernel path a
configuration of CG_FAST_CONFIGS_B takes at any particle number of the fast path has a shape in tests/config_shapes.py, and every
shape there still takes the path it was chosen for.  The paths come from tests/host_emul/cg_pathmap.cpp, i.e. from the layout
functions of the library itself: a change of a threshold or of a layout that moves a shape to another kernel, or opens a path no
shape reaches, fails here instead of leaving a GPU test that covers nothing."""
import pytest

from tests import config_shapes as cs

CONFIGS_B = [(3, 16, 16), (2, 4, 4), (3, 4, 4), (2, 8, 8), (3, 8, 8), (2, 32, 32)]


def test_the_configurations_are_those_of_the_header():
    assert sorted(cs.unit_b_configs()) == sorted(CONFIGS_B)


def test_known_paths_of_the_shipped_configuration():
    """the path map itself against facts the GPU suite pins for (2, 16, 16): workgroup sizes (test_mcmc_at_sizes_without_a_specialised_
    kernel), the fast path ends before n = 72 (test_beyond_the_lds_limit_...), the fused single-wave LU pair at n = 13, the concurrent
    pair from 256 threads, the exact and the split mode and the scores in LDS at the benchmark size"""
    for n, t in ((13, 64), (17, 128), (23, 256), (24, 256), (41, 512), (45, 512), (57, 512)):
        assert cs.paths(2, 16, 16, n)["threads"] == t
    assert cs.paths(2, 16, 16, 57)["fast"] == 1 and cs.paths(2, 16, 16, 72)["fast"] == 0
    assert cs.paths(2, 16, 16, 13)["S"] == "64:wave-both<26,13>:w1d0j0u0"
    assert cs.paths(2, 16, 16, 29)["S"] == "256:dual2:w0d1j0u0" and cs.paths(2, 16, 16, 57)["S"] == "512:dual2:w0d1j0u0"
    assert [cs.paths(2, 16, 16, 13)[f] for f in ("L0", "L2", "Q")] == ["lds", "lds", "k_scores"]
    assert cs.paths(3, 16, 16, 7)["Q"].startswith("vjp256") and cs.paths(3, 16, 16, 8)["Q"] == "k_scores"


@pytest.mark.parametrize("cfg", CONFIGS_B)
def test_every_path_has_a_shape(cfg):
    last = cs.last_fast_n(*cfg)
    assert last >= 38 and not cs.paths(*cfg, last + 1)["fast"]
    have = {f: {} for f in cs.FAMILIES}
    for shape, fams in cs.SHAPES.items():
        if shape[:3] == cfg:
            for f, sig in fams.items():
                have[f].setdefault(sig, shape[3])
    uncovered = []
    for n in range(1, last + 1):
        p = cs.paths(*cfg, n)
        for f in cs.FAMILIES:
            if p[f] not in have[f]:
                uncovered.append((n, f, p[f]))
    print("%s: n = 1 ... %d, %d signatures, %d uncovered" % (cfg, last, sum(len(v) for v in have.values()), len(uncovered)))
    assert not uncovered, uncovered
    assert any(shape[:3] == cfg and shape[3] == last and "S" in fams for shape, fams in cs.SHAPES.items()), "the last n of the fast path"


def test_every_shape_takes_the_path_it_stands_for():
    assert cs.SHAPES
    for shape, fams in cs.SHAPES.items():
        assert shape[:3] in CONFIGS_B and fams and set(fams) <= set(cs.FAMILIES), shape
        p = cs.paths(*shape)
        assert p["fast"] == 1, shape
        for f, sig in fams.items():
            assert p[f] == sig, (shape, f, sig, p[f])
