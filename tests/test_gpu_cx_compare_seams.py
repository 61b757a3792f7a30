"""The Fisher kernel against exact arithmetic, regions whose pooled cells pass int32, and the join and region kernels of
csrc/cx_compare.hip at the sizes where their indexing changes: the 256-thread workgroup, the 4096-item block of util.hip's
scan, more than 256 such blocks (the scan of the block sums takes a second round), runs and flag walks that cross those
boundaries, and arguments at the ends of int32.  Helpers, comparison rules and RTOL are test_gpu_cx_compare.py's; the
restatements and tables are tests/cx_compare_np.py's.  Nothing in a reference reads a GPU result.

Fisher against exact arithmetic: the host epi_fisher_exact is within X.EXACT_RTOL = 8.02e-13 of the 60-digit value
(test_cx_compare_host.py::test_fisher_host_against_exact_arithmetic, measured 1.002e-13) and the device within RTOL of the
host, so the device bound is their sum, 9.15e-13."""
import functools

import numpy as np
import pytest

import cx_compare_np as X
import test_gpu_cx_compare as T

pytestmark = pytest.mark.gpu

EXACT_DEVICE_RTOL = X.EXACT_RTOL + T.RTOL
M31 = X.M31


@pytest.fixture(scope="module")
def ea():
    import epialleler_amd
    return epialleler_amd


# ---- Fisher against exact arithmetic ---------------------------------------------------------------------------------------

def test_fisher_kernel_against_exact_arithmetic(ea):
    """fisherExact on LARGE_TABLES, the three tables with cells near 2^31 and every 7th table with cells 0 .. 6 against
    cx_compare_np.exact_fisher; exactly 1.0 on degenerate margins, the four tables with exact p below 1e-280 left out."""
    t, _, _ = X.exact_values()
    got = ea.fisherExact(*t.T)
    rel, t = X.worst_exact_error(got, "device")
    assert rel.max() <= EXACT_DEVICE_RTOL, (rel.max(), t[int(rel.argmax())].tolist())


# ---- pooled cells beyond int32 ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(X.wide_tables()))
def test_regions_pool_cells_beyond_int32(ea, name):
    """Runs of 2 to 4 rows with meth_a / meth_b near 2^31 - 1: k_reg_emit sums in 64 bits and hands 64-bit cells to the
    Fisher arithmetic.  Integer columns, pooled betas and mean_delta_beta bit for bit; p against exact fractions within the
    device's bound against exact arithmetic; exactly 1.0 on the degenerate run, exactly 0.0 where p underflows."""
    table, args = X.wide_tables()[name]
    want = X.regions_np(table, *args)
    assert np.all(want["cells"].max(axis=1) >= 2 ** 31)
    got = T.gpu_regions(ea, table, *args)
    T.assert_regions_equal(got, want, EXACT_DEVICE_RTOL)
    assert got["p"][-2] == 1.0 and got["p"][-1] == 0.0 and np.all(got["p"][:-2] > 0)


# ---- regions at the seams --------------------------------------------------------------------------------------------------

SEAM_SIZES = (255, 256, 257, 4095, 4096, 4097, 8193, 70001)
REGION_ARGS = [(0.05, 0.1, 300, 1), (0.05, 0.1, 40, 3), (1.0, 0.0, 2 ** 31 - 1, 2), (0.02, 0.5, 100, 1)]    # test_regions_random's


@functools.lru_cache(maxsize=None)
def _random_table(n):
    return X.random_comparison(np.random.default_rng(n), n)


@pytest.mark.parametrize("args", REGION_ARGS)
@pytest.mark.parametrize("n", SEAM_SIZES)
def test_regions_random_at_the_seams(ea, n, args):
    table = _random_table(n)
    want = X.regions_np(table, *args)
    assert want["rname"].size > 10
    T.assert_regions_equal(T.gpu_regions(ea, table, *args), want)


def test_regions_one_run_of_70001_rows(ea):
    """One thread walks the whole table; mean_delta_beta is its sum in ascending row order, bit for bit."""
    table = X.stretches_comparison(np.random.default_rng(3), [(70001, -1)])
    want = X.regions_np(table, 0.05, 0.1, 50, 3)
    assert want["nsites"].tolist() == [70001] and want["direction"].tolist() == [-1]
    T.assert_regions_equal(T.gpu_regions(ea, table, 0.05, 0.1, 50, 3), want)


@pytest.mark.parametrize("min_sites", X.LONG_MIN_SITES)
def test_regions_flag_walk_crosses_workgroups_and_scan_blocks(ea, min_sites):
    """Stretches of 250 to 6000 rows around min_sites = 300 and 5000
    (test_cx_compare_host.py::test_long_stretches_have_what_the_gpu_test_needs: at least 3 reported, at least 3 too short)."""
    table = X.long_stretches_table()
    want = X.regions_np(table, 0.05, 0.1, 50, min_sites)
    assert want["rname"].size >= 3 and want["nsites"].min() >= min_sites
    T.assert_regions_equal(T.gpu_regions(ea, table, 0.05, 0.1, 50, min_sites), want)


@pytest.mark.parametrize("min_sites", [1001, M31])
def test_regions_min_sites_above_the_row_count(ea, min_sites):
    """No run can be long enough: the report is empty (the Python side leaves room for n // min_sites = 0 regions, so a
    flagged row would be an error).  A table that is one run ends the flag walk at its last row."""
    for table in (_random_table(1000), X.stretches_comparison(np.random.default_rng(4), [(1000, 1)])):
        assert table["pos"].size // min_sites == 0
        got = T.gpu_regions(ea, table, 1.0, 0.0, M31, min_sites)
        assert got.nrow == 0
        for k in X.DMR_INT + X.DMR_FLOAT:
            assert got[k].shape == (0,) and got[k].dtype == (np.int32 if k in X.DMR_INT else np.float64), k


def test_regions_more_reported_than_a_scan_block(ea):
    """20 000 rows whose direction alternates every row, min_sites = 1: 20 000 regions, offsets past 4096."""
    table = X.stretches_comparison(np.random.default_rng(6), [(1, 1), (1, -1)] * 10000)
    want = X.regions_np(table, 0.05, 0.1, 50, 1)
    assert want["rname"].size == 20000 and want["direction"].tolist() == [1, -1] * 10000
    T.assert_regions_equal(T.gpu_regions(ea, table, 0.05, 0.1, 50, 1), want)


@pytest.mark.parametrize("min_sites,rows", [(1, [255, 256, 4095, 4096, 4198]), (2, [256, 4096])])
def test_regions_runs_that_start_on_a_boundary(ea, min_sites, rows):
    """Runs placed by hand: one row at 255, three from 256, one row at 4095, two from 4096, and the table's last row."""
    table = X.stretches_comparison(np.random.default_rng(8), [(255, 0), (1, 1), (3, -1), (3836, 0), (1, 1), (2, -1), (100, 0), (1, 1)])
    assert table["pos"].size == 4199
    want = X.regions_np(table, 0.05, 0.1, 50, min_sites)
    assert want["start"].tolist() == table["pos"][rows].tolist()
    T.assert_regions_equal(T.gpu_regions(ea, table, 0.05, 0.1, 50, min_sites), want)


def test_regions_positions_and_gaps_at_the_ends_of_int32(ea):
    """pos 0 and 2^31 - 1 are 2^31 - 1 apart: one run under max_gap = 2^31 - 1, two under 2^31 - 2 (the difference is taken
    in 64 bits).  max_gap = 0 joins the two strands of one position and nothing else."""
    far = T._cmp_table([(1, 0, 0.3, 0.01), (1, M31, 0.3, 0.01), (2, M31, 0.3, 0.01), (3, 1, -0.3, 0.01), (3, M31, -0.3, 0.01)])
    for max_gap, nsites in ((M31, [2, 1, 2]), (M31 - 1, [1, 1, 1, 2]), (M31 - 2, [1, 1, 1, 1, 1])):
        want = X.regions_np(far, 0.05, 0.1, max_gap, 1)
        assert want["nsites"].tolist() == nsites
        T.assert_regions_equal(T.gpu_regions(ea, far, 0.05, 0.1, max_gap, 1), want)
    strands = T._cmp_table([(1, 10, 0.3, 0.01), (1, 10, 0.3, 0.01), (1, 11, 0.3, 0.01), (1, 11, 0.3, 0.01), (1, 12, 0.3, 0.01)])
    want = X.regions_np(strands, 0.05, 0.1, 0, 2)
    assert list(zip(want["start"].tolist(), want["end"].tolist(), want["nsites"].tolist())) == [(10, 10, 2), (11, 11, 2)]
    T.assert_regions_equal(T.gpu_regions(ea, strands, 0.05, 0.1, 0, 2), want)


# ---- the join at the seams -------------------------------------------------------------------------------------------------

def _draw(rng, n, npos, **kw):
    """random_cx; above 5000 rows its loop-free form (the same distribution, drawn at once)."""
    return (X.random_cx if n <= 5000 else X.random_cx_vec)(rng, n, npos, **kw)


@pytest.mark.parametrize("n_a,n_b,min_coverage", [(70001, 3, 1), (3, 70001, 1), (65537, 65536, 10), (4096, 4096, 25), (4097, 1, 1)])
def test_join_random_at_the_seams(ea, n_a, n_b, min_coverage):
    """One table far longer than the other (the search runs over 3 rows, or over 70 001), both past 65 536 rows, both
    exactly one scan block, one block and a row against a single row.  Five of six keys are taken, so most rows of the
    shorter table are common."""
    rng = np.random.default_rng(n_a + n_b)
    npos = (2 * max(n_a, n_b) + 9) // 10
    a, b = _draw(rng, n_a, npos), _draw(rng, n_b, npos)
    want = X.join_np(a, b, min_coverage)
    assert want["ncommon"] >= 1 and (min(n_a, n_b) < 4096 or 0.3 * min(n_a, n_b) < want["pos"].size < want["ncommon"])
    T.assert_join_equal(T.gpu_join(ea, a, b, min_coverage), want)


def test_join_b_entirely_below_or_above_a(ea):
    """Every search ends at b's first row, or past its last one; on another rname and on a's own."""
    rng = np.random.default_rng(9)
    a = X.random_cx(rng, 300, 200, nrname=1)
    a["rname"] += 1
    a["pos"] += 1000
    for rname, shift in ((1, 0), (2, 0), (2, 5000), (3, 0)):
        b = X.random_cx(rng, 257, 200, nrname=1)
        b["rname"][:] = rname
        b["pos"] += shift
        for x, y in ((a, b), (b, a)):
            want = X.join_np(x, y, 1)
            assert want["ncommon"] == 0 and want["pos"].size == 0
            T.assert_join_equal(T.gpu_join(ea, x, y, 1), want)


def test_join_keys_and_coverage_at_the_ends_of_int32(ea):
    """rname and pos of 2^31 - 1; coverage meth + unmeth = 2^32 - 2 against min_coverage = 2^31 - 1: reported (in 32 bits the
    sum would be -2), as is coverage of exactly 2^31 - 1, while 2^31 - 2 is not."""
    a = X.cx_table([(1, 1, 5, 6, 3, 4), (1, 1, M31, 6, M31, 0), (M31, 1, 1, 6, M31 - 1, 0), (M31, 1, M31 - 1, 6, 7, 2), (M31, 1, M31, 6, M31, M31),
                    (M31, 2, M31, 6, M31, M31)])
    b = X.cx_table([(1, 1, 5, 6, 1, 9), (1, 1, M31, 6, M31 - 1, 1), (M31, 1, 1, 6, M31, M31), (M31, 1, M31 - 2, 6, 7, 2), (M31, 1, M31, 6, M31, M31),
                    (M31, 2, M31, 5, M31, M31)])
    want = X.join_np(a, b, 1)
    assert want["ncommon"] == 4 and want["pos"].tolist() == [5, M31, 1, M31]
    T.assert_join_equal(T.gpu_join(ea, a, b, 1), want)
    want = X.join_np(a, b, M31)
    assert want["ncommon"] == 4 and list(zip(want["rname"].tolist(), want["pos"].tolist())) == [(1, M31), (M31, M31)]
    assert want["p"].tolist() == [1.0, 1.0]
    T.assert_join_equal(T.gpu_join(ea, a, b, M31), want)


def test_join_above_256_scan_blocks(ea):
    """256 x 4096 + 4097 rows on either side: 258 block sums, so k_scan_bsums goes round twice.  Against join_vec
    (test_cx_compare_host.py::test_vectorised_join_equals_the_loop); coverage at most 12, so few distinct tables."""
    n = 256 * 4096 + 4097
    rng = np.random.default_rng(7)
    a, b = X.random_cx_vec(rng, n, 300000, depth=7), X.random_cx_vec(rng, n, 300000, depth=7)
    want = X.join_vec(a, b, 4)
    assert 256 * 4096 < n and 300000 < want["pos"].size < want["ncommon"] < n
    T.assert_join_equal(T.gpu_join(ea, a, b, 4), want)
