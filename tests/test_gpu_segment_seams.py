"""epi_cx_segment_dev at the seams of its two scans (the forward scan of max-plus matrices and the backward scan of psi maps
share the same thread and workgroup ranges, so every size below crosses both).  With B = epi_segment_block_sites() and t =
epi_segment_thread_sites(): one chain of t - 1, t, t + 1, B - 1, B, B + 1, 2 B + 1 and 3 B + 2 sites (a carry that crosses a
whole workgroup with no head in it); a chain head at site B - 1, B, B + 1 and at 2 B; more than B chains of one site each (the
carry workgroup's own scan); two classes meeting on a seam.  Models with exact ties (dyadic) and random ones, K = 2, 3, 4,
pure decodes and refits.  Everything is compared exactly with the restatement (tests/segment_np.py)."""
import numpy as np
import pytest

import segment_np as G
import smooth_np as S
from test_gpu_segment import check_segment, ea, one_series  # noqa: F401  (ea: the module fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def geometry(ea):  # noqa: F811
    lib = ea._lib.load()
    return lib.epi_segment_block_sites(), lib.epi_segment_thread_sites()


def blocky(rng, n, depth, run=37):
    """counts of n sites whose level alternates every `run` sites, so that states change inside every thread range"""
    level = np.where((np.arange(n) // run) % 2 == 0, 0.15, 0.85)
    cov = rng.integers(0, depth + 1, n)
    meth = rng.binomial(cov, level)
    return meth, cov - meth


def models(rng, K):
    return [(G.random_model(rng, K, dyadic=True), 2), (G.random_model(rng, K, dyadic=False), 6)]


@pytest.mark.parametrize("K", [2, 3, 4])
def test_one_chain_across_the_seams(ea, geometry, K):  # noqa: F811
    B, t = geometry
    rng = np.random.default_rng(50 + K)
    for n in (t - 1, t, t + 1, B - 1, B, B + 1, 2 * B + 1, 3 * B + 2):
        for model, depth in models(rng, K):
            meth, unmeth = blocky(rng, n, depth)
            got = check_segment(ea, one_series(meth, unmeth), model, (K, n, depth), max_gap=10, max_iter=1)
            assert got.nchain == 1
    # a chain longer than a workgroup's range whose middle workgroup sees no state change at all
    n = 3 * B + 2
    meth = np.where(np.arange(n) < B // 2, 9, 0)
    got = check_segment(ea, one_series(meth, 9 - meth), G.start_model((0.1, 0.5, 0.9, 0.3)[:K], 0.9), max_gap=10, max_iter=3)
    assert got.nchain == 1 and got.nsegment == 2


@pytest.mark.parametrize("K", [2, 3, 4])
def test_chain_heads_at_the_seams(ea, geometry, K):  # noqa: F811
    B, t = geometry
    rng = np.random.default_rng(60 + K)
    n = 2 * B + t + 3
    for heads in ([B - 1], [B], [B + 1], [2 * B], [B - 1, B, B + 1, 2 * B], [t - 1, t, t + 1, B - t, 2 * B - 1, 2 * B + 1]):
        gaps = np.ones(n, np.int64)
        gaps[heads] = 100                                              # above max_gap: site `h` starts a chain
        pos = np.cumsum(gaps)
        for model, depth in models(rng, K):
            meth, unmeth = blocky(rng, n, depth)
            got = check_segment(ea, one_series(meth, unmeth, pos), model, (K, heads, depth), max_gap=50, max_iter=1 if depth == 2 else 3)
            assert got.nchain == len(heads) + 1


def test_more_chains_than_a_workgroup_has_sites(ea, geometry):  # noqa: F811
    B, t = geometry
    rng = np.random.default_rng(70)
    n = B + 3
    meth, unmeth = blocky(rng, n, 3, run=1)
    tab = one_series(meth, unmeth, np.arange(n) * 5 + 1)
    for K in (2, 3, 4):
        for model, _ in models(rng, K):
            got = check_segment(ea, tab, model, K, max_gap=4, max_iter=2)   # every gap is above max_gap
            assert got.nchain == n and got.nsegment == n


@pytest.mark.parametrize("K", [2, 4])
def test_two_classes_meet_on_a_seam(ea, geometry, K):  # noqa: F811
    B, t = geometry
    rng = np.random.default_rng(80 + K)
    for first in (B - 1, B, B + 1, t, 2 * B):                              # sites of the first class in series order
        second = B + t + 1
        m1, u1 = blocky(rng, first, 3)
        m2, u2 = blocky(rng, second, 3)
        # the '+' CG series sorts before the '-' CHH one whatever the positions: interleave them in the table
        tab = S.series_table([(1, 1, S.CG, np.arange(first) * 2 + 10, m1, u1), (1, 2, S.CHH, np.arange(second) * 2 + 11, m2, u2)])
        for model, depth in models(rng, K):
            got = check_segment(ea, tab, model, (K, first), max_gap=10, max_iter=1 if depth == 2 else 4)
            assert got.nchain == 2


def test_refit_counts_beyond_one_round(ea):  # noqa: F811
    """the counts kernel runs at most 512 workgroups of 256 threads, each over a strided share of the sites: a table that takes
    a second round, refitted once (K = 2 keeps the restatement's loops to under two seconds)"""
    rng = np.random.default_rng(90)
    n = 512 * 256 + 300
    meth, unmeth = blocky(rng, n, 6, run=5000)
    gaps = np.ones(n, np.int64)
    gaps[[1000, 512 * 256 - 1, 512 * 256]] = 100                     # chain heads in both rounds
    got = check_segment(ea, one_series(meth, unmeth, np.cumsum(gaps)), ([0.3, 0.6], [[0.9, 0.1], [0.1, 0.9]], [0.5, 0.5]), max_gap=50, max_iter=2)
    assert got.nchain == 4 and got.fit["iterations"] == 2 and got.fit["p"][0] < 0.2 and got.fit["p"][1] > 0.8
