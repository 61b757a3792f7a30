"""epi_cx_smooth_dev at its seams: series of T - 1, T, T + 1 and 2 T + 1 sites around the T = epi_smooth_tile_sites() sites a
workgroup of the fit kernel owns, a cluster cut and a class change exactly on a tile seam, a range of
epi_smooth_stage_sites() + 300 sites that no workgroup can stage (the global-memory path) beside ranges that are staged,
row counts around the 256-thread workgroups and the 4096-row tiles of the scan and the sort, and the window limit.  Against
the numpy restatement (tests/smooth_np.py): integer columns exactly, float columns bit for bit."""
import numpy as np
import pytest

import smooth_np as S
from test_gpu_smooth import MARK, _untouched, check_merge, check_smooth, ea, raw_smooth  # noqa: F401

pytestmark = pytest.mark.gpu


def _sizes(ea):
    lib = ea._lib.load()
    return lib.epi_smooth_tile_sites(), lib.epi_smooth_stage_sites()


def _series(rng, n, start=100, max_step=30):
    pos = start + np.cumsum(rng.integers(1, max_step + 1, n))
    cov = rng.poisson(5, n) * (rng.random(n) >= 0.2)
    meth = rng.binomial(cov, 0.4)
    return pos, meth, cov - meth


@pytest.mark.parametrize("which", ["T-1", "T", "T+1", "2T+1"])
def test_series_around_a_tile(ea, which):
    T, _ = _sizes(ea)
    n = {"T-1": T - 1, "T": T, "T+1": T + 1, "2T+1": 2 * T + 1}[which]
    rng = np.random.default_rng(n)
    t = S.series_table([(1, 1, S.CG, *_series(rng, n))])
    for kw in (dict(bandwidth=100, min_sites=9), dict(bandwidth=1, min_sites=1, degree=0), dict(bandwidth=10 ** 6, min_sites=70, degree=1)):
        got = check_smooth(ea, t, (which, kw), **kw)
    assert got.max_window == n and got.ncluster == 1                    # the last bandwidth spans the series


def test_cuts_on_a_tile_seam(ea):
    T, _ = _sizes(ea)
    rng = np.random.default_rng(4)
    a, b = _series(rng, T), _series(rng, T // 2 + 3, start=10 ** 6)
    # series order = table order here (one class): the second cluster starts at series index T, by the gap ...
    t = S.series_table([(1, 1, S.CG, *a), (1, 1, S.CG, *b)])
    assert check_smooth(ea, t, bandwidth=200, min_sites=20, max_gap=1000).ncluster == 2
    assert check_smooth(ea, t, bandwidth=200, min_sites=20, max_gap=10 ** 6).ncluster == 1
    # ... by the rname ...
    t = S.series_table([(1, 1, S.CG, *a), (2, 1, S.CG, *_series(rng, T + 5, start=50))])
    assert check_smooth(ea, t, bandwidth=200, min_sites=20).ncluster == 2
    # ... and by the class: '+' CHH sorts in front of '+' CG and '-' rows behind both, whatever the table order
    t = S.series_table([(1, 1, S.CHH, *a), (2, 1, S.CG, *_series(rng, T, start=90)), (1, 2, S.CHH, *_series(rng, T - 1, start=95)),
                        (2, 2, S.CHH, *_series(rng, 2, start=5))])
    got = check_smooth(ea, t, bandwidth=200, min_sites=20)
    assert got.ncluster == 4


def test_global_memory_path(ea):
    """stage + 300 sites at consecutive positions under a bandwidth that spans them all: every workgroup's range is the whole
    series and does not fit the staging buffer; the second series on the same table does fit and is staged."""
    T, stage = _sizes(ea)
    n = stage + 300
    rng = np.random.default_rng(6)
    cov = rng.poisson(4, n)
    meth = rng.binomial(cov, np.linspace(0.1, 0.9, n))
    small = _series(rng, T + 7, start=10)
    t = S.series_table([(1, 1, S.CG, 1000 + np.arange(n), meth, cov - meth), (2, 1, S.CG, *small)])
    got = check_smooth(ea, t, bandwidth=n + 10, min_sites=70)
    assert got.max_window == n and (got["nsites"][got["rname"] == 1] == n).all() and got.ncluster == 2
    # a range one site above and exactly at what is staged: T sites whose windows reach stage - T + 1 and stage - T sites further
    for extra in (1, 0):
        m = stage + extra
        cov = rng.poisson(4, m)
        meth = rng.binomial(cov, 0.5)
        t = S.series_table([(1, 2, S.CHG, 5 + np.arange(m), meth, cov - meth)])
        check_smooth(ea, t, extra, bandwidth=m - T + 1, min_sites=3, degree=1)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4095, 4096, 4097])
def test_row_counts_around_the_workgroup_scan_and_sort_tiles(ea, n):
    rng = np.random.default_rng(n)
    t = S.random_cx(rng, n + 40)
    t = {k: v[:n] for k, v in t.items()}
    assert t["pos"].size == n
    check_smooth(ea, t, n, bandwidth=30, min_sites=4, max_gap=500)
    check_merge(ea, t, n)


def test_window_limit(ea):
    from epialleler_amd import _lib
    n = S.MAX_WINDOW + 1
    ones = np.ones(n, np.int64)
    t = S.series_table([(1, 1, S.CG, 10 + np.arange(n), ones, ones)])
    rc, ncluster, max_window, cols, msg = raw_smooth(ea, t, bandwidth=n)
    assert rc == _lib.EPI_ERR_ARG and max_window == n and ncluster == 1 and b"65537 sites, at most 65536" in msg and _untouched(cols)
    # one site fewer is served: the largest window there is (checked at its ends and in the middle against the restatement's sum)
    t = {k: v[:n - 1] for k, v in t.items()}
    rc, ncluster, max_window, cols, msg = raw_smooth(ea, t, bandwidth=n, degree=0)
    assert rc == _lib.EPI_OK and (ncluster, max_window) == (1, n - 1) and (cols[6] == n - 1).all() and (cols[7] == n).all()
    assert (cols[8] == 0).all() and (cols[10] == 0.5).all()
    for i in (0, n // 2, n - 2):
        S0 = S.window_sums(t["pos"].astype(np.int64), t["meth"].astype(np.int64), (t["meth"] + t["unmeth"]).astype(np.int64), i, n)[0][0]
        assert cols[11][i] == S0, i
