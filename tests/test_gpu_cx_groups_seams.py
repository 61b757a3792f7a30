"""epi_cx_groups_dev at its seams: per-sample row counts around the 256-thread workgroup and the 4096-item tiles of the scan
and the sort, with overlapping and with disjoint position sets; about 20 000 rows a sample; 32 + 32 samples; the ends of
the 64-bit key; and the call between other reports.  Compared with tests/cx_groups_np.py as test_gpu_cx_groups.py does."""
import numpy as np
import pytest

import cx_compare_np as X
import cx_groups_np as G
from test_gpu_cx_groups import allocations, assert_groups_equal, dev_report, ea, gpu_groups  # noqa: F401

pytestmark = pytest.mark.gpu

TESTS = ("lrt", "lrt_mn", "welch", "fisher")


@pytest.mark.parametrize("disjoint", [False, True])
@pytest.mark.parametrize("nrows", [0, 1, 255, 256, 257, 4095, 4096, 4097])
def test_rows_around_the_tiles(ea, nrows, disjoint):
    """2 + 1 samples of nrows rows each, all from one position set or each from its own; the test and the minimum rotate."""
    rng = np.random.default_rng(1000 + nrows)
    a, b = G.random_groups(rng, 2, 1, nrows, max(nrows + nrows // 8, 1), depth=12, disjoint=disjoint)
    assert all(t["pos"].size == nrows for t in a + b)
    test = TESTS[nrows % 4]
    min_a = 1 + nrows % 2
    want = G.groups_np(a, b, 2, min_a, 1, test)
    got = gpu_groups(ea, a, b, 2, min_a, 1, test)
    assert_groups_equal(got, want, test, "%d rows%s" % (nrows, " disjoint" if disjoint else ""))
    if disjoint or nrows == 0:
        assert got.nrow == 0 and (got.nsites > 2 * nrows or nrows < 8)
    elif nrows > 1:
        assert got.nrow > nrows // 4


def test_twenty_thousand_rows_a_sample(ea):
    rng = np.random.default_rng(77)
    a, b = G.random_groups(rng, 2, 2, 20000, 24000, depth=25)
    before = allocations(ea)
    for test, mins in (("lrt", (2, 2)), ("welch", (2, 2))):
        want = G.groups_np(a, b, 4, *mins, test)
        assert want["pos"].size > 5000
        assert_groups_equal(gpu_groups(ea, a, b, 4, *mins, test), want, test, "20 000 rows")
    assert allocations(ea) == before


def test_thirty_two_samples_a_side(ea):
    """Runs of up to 64 entries: every sample has nearly every site."""
    rng = np.random.default_rng(64)
    a, b = G.random_groups(rng, 32, 32, 258, 260, depth=40)
    for test, mins in (("lrt_mn", (32, 32)), ("welch", (30, 31)), ("fisher", (1, 32)), ("lrt", (32, 1))):
        want = G.groups_np(a, b, 1, *mins, test)
        assert want["pos"].size > 20 and (want["nsamples_a"].max(), want["nsamples_b"].max()) == (32, 32)
        assert_groups_equal(gpu_groups(ea, a, b, 1, *mins, test), want, test, "32 + 32")


def test_key_ends(ea):
    """pos = 2^31 - 1 and 0, the largest accepted rname code and 0, both strands, every context code: the columns come
    back out of the key as they went in, in (rname, pos, strand, context) order."""
    top, m31 = G.MAX_RNAME, 2 ** 31 - 1
    rows = [(0, 1, 0, 0, 3, 1), (0, 2, 0, 7, 2, 2), (0, 1, m31, 1, 4, 0), (0, 2, m31, 6, 1, 5),
            (1, 1, 7, 2, 1, 1), (1, 2, 7, 2, 2, 1), (top, 1, 0, 3, 0, 4), (top, 1, m31, 4, 5, 5), (top, 2, m31, 5, 6, 1)]
    a = [X.cx_table(rows), X.cx_table(rows[1:])]
    shifted = [(r, s, p, c, m + 1, u + 2) for r, s, p, c, m, u in rows]
    b = [X.cx_table(shifted), X.cx_table([(r, s, p, (c + 1) % 8, m, u) for r, s, p, c, m, u in rows[::2]] + [])]
    for t in a + b:
        assert X.is_sorted(t)
    for test in TESTS:
        want = G.groups_np(a, b, 1, 1, 1, test)
        got = gpu_groups(ea, a, b, 1, 1, 1, test)
        assert_groups_equal(got, want, test, "key ends")
        assert got.nrow == len(rows) and got.nsites == len(rows) + len(rows[::2])
        assert got["rname"].tolist() == [r[0] for r in rows] and got["pos"].tolist() == [r[2] for r in rows]
        assert got["strand"].tolist() == [r[1] for r in rows] and got["context"].tolist() == [r[3] for r in rows]
    # one position and strand under two context codes: two sites, in context order
    two = gpu_groups(ea, [X.cx_table([(5, 2, 9, 6, 1, 1)]), X.cx_table([(5, 2, 9, 2, 2, 2)])], [X.cx_table([(5, 2, 9, 2, 3, 3)]), X.cx_table([(5, 2, 9, 6, 4, 4)])],
                     1, 1, 1, "fisher")
    assert two["context"].tolist() == [2, 6] and two["meth_a"].tolist() == [2, 1] and two["meth_b"].tolist() == [3, 4] and two.nsites == 2
