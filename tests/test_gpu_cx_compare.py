"""fisherExact, the cytosine report comparison and its regions against the host Fisher test and the plain restatement of
tests/cx_compare_np.py (include/epihip.h: epi_fisher_exact_dev, epi_cx_compare_dev, epi_cx_compare_regions_dev).  Nothing in
the restatement reads a GPU result.  Integer columns and row sets compare exactly; beta_a, beta_b, delta_beta (one IEEE
division or subtraction of integers each) and mean_delta_beta (a sequential sum in row order) bit for bit.

p compares with the host epi_fisher_exact: NaN where it has NaN, exactly 1.0 on degenerate margins, exactly equal where it
returns 0.0, within 1e-300 absolute in the denormal range, and elsewhere within RTOL relative.  Device and host run the
same operations in the same order (csrc/fisher_math.hpp); what differs is lgamma / log / exp, by ulps that the size
of the exponent scales.  RTOL is 8 times the largest relative difference measured over the tables of
test_fisher_kernel_against_the_host on an MI355X (profiles/cx_compare.txt): measured 1.405e-14, RTOL = 1.124e-13 (measured
again, and the same, after dbinom_raw's lf became log((n - x) / n)).  A
difference above 1e-9 would be a wrong port, not an imprecise one (the tie band is 1e-7 wide;
test_cx_compare_host.py::test_fisher_tables_stay_clear_of_the_tie_band shows no table of the list can change sides).
What the shared header itself gets wrong shows in neither side of this comparison: test_gpu_cx_compare_seams.py and
test_cx_compare_host.py hold both against exact arithmetic.

The last three tests run the calls in sequence on the `samples` fixture: they keep no state and leave no report changed."""
import ctypes as C

import numpy as np
import pytest

import cx_compare_np as X
import helpers as H

pytestmark = pytest.mark.gpu

MEASURED_REL = 1.405e-14
RTOL = 8 * MEASURED_REL
LEVELS = ("chrA", "chrB", "chrC")


@pytest.fixture(scope="module")
def ea():
    import epialleler_amd
    return epialleler_amd


def dev_report(ea, t, names, levels=LEVELS):
    import torch
    return ea.Report({k: torch.from_numpy(np.ascontiguousarray(t[k])).cuda() for k in names}, levels)


def gpu_join(ea, a, b, min_coverage=1):
    rep = ea.rcpp_cx_compare(dev_report(ea, a, X.CX), dev_report(ea, b, X.CX), min_coverage)
    assert list(rep) == list(X.CMP_INT + X.CMP_FLOAT) and rep.levels["rname"] == LEVELS
    return rep


def gpu_regions(ea, t, max_p, min_delta_beta, max_gap, min_sites):
    rep = ea.rcpp_cx_compare_regions(dev_report(ea, t, X.CMP_INT + X.CMP_FLOAT), max_p, min_delta_beta, max_gap, min_sites)
    assert list(rep) == list(X.DMR_INT + X.DMR_FLOAT)
    return rep


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def assert_join_equal(got, want):
    assert got.ncommon == want["ncommon"]
    for k in X.CMP_INT:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), k
    for k in ("beta_a", "beta_b", "delta_beta"):
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    X.compare_p(got["p"], want["p"], np.stack([want[k] for k in X.CMP_INT[4:]], 1), RTOL)


def assert_regions_equal(got, want, rtol=RTOL):
    for k in X.DMR_INT:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), k
    for k in ("beta_a", "beta_b", "delta_beta", "mean_delta_beta"):
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    X.compare_p(got["p"], want["p"], want["cells"], rtol)


# ---- the Fisher kernel ---------------------------------------------------------------------------------------------------

def test_fisher_kernel_against_the_host(ea):
    """All 2401 tables with cells 0 .. 6, tables through every branch of stirlerr and both of bd0, underflow to 0, cells of
    10^6 and of 2^31 - 1, negative cells.  Prints the largest relative difference: the figure RTOL comes from."""
    t, want = X.fisher_cases()
    got = ea.fisherExact(t[:, 0], t[:, 1], t[:, 2], t[:, 3])
    assert got.dtype == np.float64 and got.shape == want.shape
    X.compare_p(got, want, t, RTOL)
    assert np.all(got[~np.isnan(got)] <= 1.0) and np.all(got[~np.isnan(got)] >= 0.0)
    assert abs(got[np.flatnonzero((t == (3, 1, 1, 3)).all(axis=1))[0]] / X.KAT_P_3113 - 1) < 1e-12


def test_fisher_device_tensors_and_empty(ea):
    import torch
    t, want = X.fisher_cases()
    cells = [torch.from_numpy(np.ascontiguousarray(t[:, i])).cuda() for i in range(4)]
    got = ea.fisherExact(*cells, as_device=True)
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float64
    assert np.array_equal(bits(got.cpu().numpy()), bits(ea.fisherExact(*[t[:, i].astype(np.int64) for i in range(4)])))
    assert ea.fisherExact([], [], [], []).shape == (0,)
    with pytest.raises(ValueError):
        ea.fisherExact(cells[0].double(), *cells[1:])


# ---- the join ------------------------------------------------------------------------------------------------------------

def _row(r, s, p, ctx=6, m=5, u=5):
    return (r, s, p, ctx, m, u)


EMPTY = X.cx_table([])
BASE = X.cx_table([_row(1, 1, 10, m=3, u=1), _row(1, 2, 11), _row(1, 1, 20), _row(2, 1, 5, m=0, u=9), _row(2, 2, 6), _row(3, 2, 7, m=7, u=0)])
OTHER = X.cx_table([_row(1, 1, 10, m=1, u=3), _row(1, 1, 11), _row(1, 2, 20), _row(2, 1, 5, ctx=5), _row(2, 2, 6, m=2, u=0), _row(3, 1, 1),
                    _row(3, 2, 7, m=0, u=7)])
JOIN_CASES = {
    "a_empty": (EMPTY, BASE, 1), "b_empty": (BASE, EMPTY, 1), "both_empty": (EMPTY, EMPTY, 1),
    "nothing_common": (BASE, X.cx_table([_row(1, 1, 9), _row(1, 2, 10), _row(2, 1, 6), _row(4, 1, 1)]), 1),
    "a_is_b": (BASE, BASE, 1),
    # common rows first and last in both; a strand present in one table only (1:11, 1:20); a context mismatch (2:5);
    # three rnames
    "mixed": (BASE, OTHER, 1), "mixed_swapped": (OTHER, BASE, 1),
    "first_and_last_of_a_only": (BASE, X.cx_table([_row(0, 1, 1), _row(1, 1, 10), _row(3, 2, 7), _row(3, 2, 8)]), 1),
    "min_coverage_cuts": (BASE, OTHER, 3), "min_coverage_zero_is_one": (X.cx_table([_row(1, 1, 1, m=0, u=0), _row(1, 1, 2)]),
                                                                       X.cx_table([_row(1, 1, 1), _row(1, 1, 2)]), 0),
    "min_coverage_cuts_all": (BASE, OTHER, 100),
}


@pytest.mark.parametrize("name", sorted(JOIN_CASES))
def test_join_hand_made(ea, name):
    a, b, min_coverage = JOIN_CASES[name]
    want = X.join_np(a, b, min_coverage)
    assert_join_equal(gpu_join(ea, a, b, min_coverage), want)
    if name == "mixed":
        assert want["ncommon"] == 3 and want["pos"].tolist() == [10, 6, 7] and want["p"][0] == pytest.approx(X.KAT_P_3113, rel=1e-12)
    if name == "min_coverage_cuts":
        assert want["ncommon"] == 3 and want["pos"].tolist() == [10, 7]
    if name == "a_is_b":
        assert want["ncommon"] == 6 and np.all(want["p"] == 1.0)


@pytest.mark.parametrize("n_a,n_b,min_coverage", [(1003, 997, 1), (997, 1003, 25), (4099, 4500, 10)])
def test_join_random(ea, n_a, n_b, min_coverage):
    """Row counts that are no multiple of the workgroup; the last pair also crosses the scan's 4096-item blocks."""
    rng = np.random.default_rng(n_a)
    a, b = X.random_cx(rng, n_a, n_a // 2), X.random_cx(rng, n_b, n_a // 2)
    want = X.join_np(a, b, min_coverage)
    assert 50 < want["pos"].size < want["ncommon"] < min(n_a, n_b) or min_coverage == 1
    assert_join_equal(gpu_join(ea, a, b, min_coverage), want)


def raw_join(ea, a, b, min_coverage, cap):
    """epi_cx_compare_dev itself, into columns filled with a mark: (rc, ncommon, nrow, columns)."""
    import torch
    from epialleler_amd import _lib, api
    lib = _lib.load()
    da, db = [dev_report(ea, t, X.CX) for t in (a, b)]
    icols = list(torch.full((8, max(cap, 1)), -7, dtype=torch.int32, device="cuda").unbind(0))
    dcols = list(torch.full((4, max(cap, 1)), -7.0, dtype=torch.float64, device="cuda").unbind(0))
    ncommon, nrow = C.c_int64(-1), C.c_int64(-1)
    rc = lib.epi_cx_compare_dev(api._engine(0), api._ptr_array([da[k] for k in X.CX]), a["pos"].size, api._ptr_array([db[k] for k in X.CX]),
                                b["pos"].size, min_coverage, api._ptr_array(icols), api._ptr_array(dcols), cap, api._stream(0),
                                C.byref(ncommon), C.byref(nrow))
    torch.cuda.synchronize()
    return rc, ncommon.value, nrow.value, [c.cpu().numpy() for c in icols + dcols], lib.epi_last_error()


def test_join_unsorted_input_is_refused(ea):
    from epialleler_amd import _lib
    swapped = {k: v[[0, 2, 1, 3, 4, 5]] for k, v in BASE.items()}
    strands = X.cx_table([_row(1, 2, 10), _row(1, 1, 10)])
    twice = X.cx_table([_row(1, 1, 10), _row(1, 1, 10)])
    for a, b, which in ((swapped, BASE, b"first"), (BASE, swapped, b"second"), (strands, BASE, b"first"), (BASE, twice, b"second")):
        rc, ncommon, nrow, cols, msg = raw_join(ea, a, b, 1, 16)
        assert rc == _lib.EPI_ERR_ARG and which in msg and b"ascending" in msg
        assert ncommon == 0 and nrow == 0 and all(np.all(c == -7) for c in cols)
    with pytest.raises(ea.EpihipError) as ei:
        gpu_join(ea, swapped, BASE)
    assert ei.value.code == _lib.EPI_ERR_ARG


def test_join_capacity(ea):
    from epialleler_amd import _lib
    want = X.join_np(BASE, OTHER, 1)
    for cap in (0, 2):
        rc, ncommon, nrow, cols, msg = raw_join(ea, BASE, OTHER, 1, cap)
        assert rc == _lib.EPI_ERR_ARG and nrow == 3 and b"3 rows" in msg
        assert all(np.all(c == -7) for c in cols)
    rc, ncommon, nrow, cols, _ = raw_join(ea, BASE, OTHER, 1, 3)
    assert rc == _lib.EPI_OK and (ncommon, nrow) == (3, 3)
    for k, c in zip(X.CMP_INT, cols):
        assert np.array_equal(c, want[k])


# ---- the regions ---------------------------------------------------------------------------------------------------------

def _cmp_table(rows):
    """rows of (rname, pos, delta_beta, p): a comparison table with counts that fit the direction"""
    n = len(rows)
    t = {"rname": np.asarray([r[0] for r in rows], np.int32), "strand": np.asarray([1 + i % 2 for i in range(n)], np.int32),
         "pos": np.asarray([r[1] for r in rows], np.int32), "context": np.full(n, 6, np.int32)}
    up = np.asarray([r[2] > 0 for r in rows], bool)
    t.update(meth_a=np.where(up, 2, 17).astype(np.int32), unmeth_a=np.where(up, 18, 3).astype(np.int32),
             meth_b=np.where(up, 15, 4).astype(np.int32), unmeth_b=np.where(up, 5, 16).astype(np.int32))
    t.update(beta_a=t["meth_a"] / 20.0, beta_b=t["meth_b"] / 20.0, delta_beta=np.asarray([r[2] for r in rows], np.float64),
             p=np.asarray([r[3] for r in rows], np.float64))
    return t


NAN = float("nan")
REGION_CASES = {
    "one_run_is_the_table": (_cmp_table([(1, 10 * i, 0.3 + i / 100, 0.01) for i in range(9)]), (0.05, 0.1, 50, 3)),
    "run_ends_at_the_last_row": (_cmp_table([(1, 10, 0.3, 0.5), (1, 20, -0.3, 0.01), (1, 30, 0.3, 0.01), (1, 40, 0.4, 0.02), (1, 50, 0.5, 0.03)]),
                                 (0.05, 0.1, 50, 3)),
    "min_sites_1": (_cmp_table([(1, 10, 0.3, 0.01), (1, 20, -0.3, 0.01), (1, 30, 0.05, 0.01), (2, 40, 0.3, 0.01), (2, 40, 0.3, 0.01)]),
                    (0.05, 0.1, 0, 1)),
    "nothing_significant": (_cmp_table([(1, 10, 0.3, 0.06), (1, 20, 0.09, 0.01), (1, 30, 0.0, 0.0), (1, 40, -0.0, 0.0)]), (0.05, 0.1, 50, 1)),
    "nan": (_cmp_table([(1, 10, 0.3, NAN), (1, 20, NAN, 0.01), (1, 30, 0.3, 0.01), (1, 40, 0.3, NAN), (1, 50, 0.3, 0.01), (1, 60, 0.3, 0.01)]),
            (1.0, 0.0, 50, 1)),
    "limits_are_inclusive": (_cmp_table([(1, 10, 0.1, 0.05), (1, 60, -0.1, 0.05), (1, 110, -0.1, 0.05), (1, 161, -0.1, 0.05)]), (0.05, 0.1, 50, 1)),
    "min_delta_beta_0_leaves_zero_out": (_cmp_table([(1, 10, 1e-9, 0.0), (1, 11, 0.0, 0.0), (1, 12, 1e-9, 0.0)]), (0.0, 0.0, 5, 1)),
}


@pytest.mark.parametrize("name", sorted(REGION_CASES))
def test_regions_hand_made(ea, name):
    table, args = REGION_CASES[name]
    want = X.regions_np(table, *args)
    assert_regions_equal(gpu_regions(ea, table, *args), want)
    expect = {"one_run_is_the_table": [(0, 80, 9, 1)], "run_ends_at_the_last_row": [(30, 50, 3, 1)],
              "min_sites_1": [(10, 10, 1, 1), (20, 20, 1, -1), (40, 40, 2, 1)], "nothing_significant": [],
              "nan": [(30, 30, 1, 1), (50, 60, 2, 1)], "limits_are_inclusive": [(10, 10, 1, 1), (60, 110, 2, -1), (161, 161, 1, -1)],
              "min_delta_beta_0_leaves_zero_out": [(10, 10, 1, 1), (12, 12, 1, 1)]}[name]
    assert list(zip(want["start"].tolist(), want["end"].tolist(), want["nsites"].tolist(), want["direction"].tolist())) == expect


def test_known_answer_on_the_device(ea):
    """The hand-written pair of tests/cx_compare_np.py through the join and the regions."""
    k = X.KAT_ARGS
    table = gpu_join(ea, X.KAT_A, X.KAT_B, k["min_coverage"])
    assert table.ncommon == X.KAT_NCOMMON
    regions = gpu_regions(ea, table, k["max_p"], k["min_delta_beta"], k["max_gap"], k["min_sites"])
    X.check_kat(table, regions)
    want = X.join_np(X.KAT_A, X.KAT_B, k["min_coverage"])
    assert_join_equal(table, want)
    assert_regions_equal(regions, X.regions_np(want, k["max_p"], k["min_delta_beta"], k["max_gap"], k["min_sites"]))


@pytest.mark.parametrize("args", [(0.05, 0.1, 300, 1), (0.05, 0.1, 40, 3), (1.0, 0.0, 2 ** 31 - 1, 2), (0.02, 0.5, 100, 1)])
def test_regions_random(ea, args):
    """1000 rows whose significance and direction change in stretches of 1 .. 20 rows, NaN in p and delta_beta."""
    table = X.random_comparison(np.random.default_rng(5), 1000)
    want = X.regions_np(table, *args)
    assert want["rname"].size > 10
    assert_regions_equal(gpu_regions(ea, table, *args), want)


def test_regions_arguments_and_capacity(ea):
    import torch
    from epialleler_amd import _lib, api
    lib = _lib.load()
    table, args = REGION_CASES["min_sites_1"]
    rep = dev_report(ea, table, X.CMP_INT + X.CMP_FLOAT)
    cols = [rep[k] for k in X.CMP_INT + X.CMP_FLOAT]

    def raw(max_p, min_delta, max_gap, min_sites, cap):
        icols = list(torch.full((5, max(cap, 1)), -7, dtype=torch.int32, device="cuda").unbind(0))
        dcols = list(torch.full((5, max(cap, 1)), -7.0, dtype=torch.float64, device="cuda").unbind(0))
        n = C.c_int64(-1)
        rc = lib.epi_cx_compare_regions_dev(api._engine(0), api._ptr_array(cols[:8]), api._ptr_array(cols[8:]), 5, max_p, min_delta, max_gap,
                                            min_sites, api._ptr_array(icols), api._ptr_array(dcols), cap, api._stream(0), C.byref(n))
        torch.cuda.synchronize()
        return rc, n.value, [c.cpu().numpy() for c in icols + dcols]

    for bad in ((-0.1, 0.1, 0, 1), (1.1, 0.1, 0, 1), (NAN, 0.1, 0, 1), (0.05, -0.1, 0, 1), (0.05, 1.1, 0, 1), (0.05, NAN, 0, 1),
                (0.05, 0.1, -1, 1), (0.05, 0.1, 0, 0), (0.05, 0.1, 0, -3)):
        rc, n, out = raw(*bad, 5)
        assert rc == _lib.EPI_ERR_ARG and n == 0 and all(np.all(c == -7) for c in out), bad
    rc, n, out = raw(*args, 2)
    assert rc == _lib.EPI_ERR_ARG and n == 3 and all(np.all(c == -7) for c in out) and b"3 regions" in lib.epi_last_error()
    rc, n, out = raw(*args, 3)
    assert rc == _lib.EPI_OK and n == 3 and out[1].tolist() == [10, 20, 40]
    with pytest.raises(ValueError):
        ea.rcpp_cx_compare_regions(rep, max_p=2)


# ---- end to end ----------------------------------------------------------------------------------------------------------

def _sample(seed, raised):
    """300 templates of 80 bases on two sequences and both strands, a CpG every 6 bases and a few CHH calls; methylation
    0.3, in 300 .. 520 of the first sequence 0.15, or 0.95 when `raised`."""
    rng = np.random.default_rng(seed)
    xms, starts, strands, rnames = [], [], [], []
    for _ in range(300):
        st, rn = int(rng.integers(1, 800)), int(rng.integers(1, 3))
        s = []
        for pos in range(st, st + 80):
            level = (0.95 if raised else 0.15) if rn == 1 and 300 <= pos <= 520 else 0.3
            if pos % 6 == 0:
                s.append("Z" if rng.random() < level else "z")
            elif pos % 17 == 0:
                s.append("H" if rng.random() < 0.03 else "h")
            else:
                s.append(".")
        xms.append("".join(s)); starts.append(st); strands.append(int(rng.integers(1, 3))); rnames.append(rn)
    return H.templates_from_xm(xms, starts, strands, rnames)


@pytest.fixture(scope="module")
def samples(ea):
    ta, tb = _sample(11, False), _sample(12, True)
    mk = lambda t: ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"], LEVELS[:2])
    return mk(ta), mk(tb)


def _read_tsv(path):
    with open(path) as f:
        rows = [ln.rstrip("\n").split("\t") for ln in f]
    return rows[0], rows[1:]


def _assert_round_trip(rep, path, int_cols, float_cols, levels):
    head, rows = _read_tsv(path)
    assert head == list(int_cols + float_cols) and len(rows) == rep.nrow
    for j, k in enumerate(head):
        col = [r[j] for r in rows]
        if k in float_cols:
            back = np.asarray([float(v) if v else np.nan for v in col])
            np.testing.assert_allclose(back, rep[k], rtol=1e-14, atol=0, equal_nan=True)
        elif k in levels:
            assert col == [levels[k][v - 1] for v in rep[k].tolist()]
        else:
            assert col == [str(v) for v in rep[k].tolist()]


@pytest.mark.parametrize("threshold_reads", [True, False])
def test_end_to_end(ea, samples, tmp_path, threshold_reads):
    a, b = samples
    kw = dict(threshold_reads=threshold_reads, min_context_sites=2, min_context_beta=0.2, min_coverage=4)
    cx_kw = {k: v for k, v in kw.items() if k != "min_coverage"}
    before = [(ea.generateCytosineReport(x, **cx_kw), ea.generateHeterogeneityReport(x, window_sites=3)) for x in (a, b)]
    cx_a, cx_b = before[0][0], before[1][0]
    assert 200 < cx_a.nrow < 1000 and set(cx_a["rname"].tolist()) == {1, 2} and set(cx_a["strand"].tolist()) == {1, 2}
    assert X.is_sorted(cx_a) and X.is_sorted(cx_b)
    want = X.join_np(cx_a, cx_b, 4)
    assert 100 < want["pos"].size < want["ncommon"]
    got = ea.compareCytosineReports(a, b, **kw)
    assert_join_equal(got, want)
    assert got.levels["rname"] == LEVELS[:2]
    region_kw = dict(max_p=0.05, min_delta_beta=0.2, max_gap=30, min_sites=3)
    want_r = X.regions_np(want, 0.05, 0.2, 30, 3)
    assert want_r["rname"].size >= 1 and np.any((want_r["rname"] == 1) & (want_r["direction"] == 1) & (want_r["start"] >= 300) & (want_r["end"] <= 520))
    got_r = ea.generateDmrReport(a, b, **kw, **region_kw)
    assert got_r.ncommon == want["ncommon"]
    assert_regions_equal(got_r, want_r)
    # device columns on request; files on request
    import torch
    dev = ea.compareCytosineReports(a, b, as_device=True, **kw)
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in dev.values()) and dev.ncommon == got.ncommon
    for k in got:
        assert np.array_equal(dev[k].cpu().numpy(), got[k], equal_nan=True)
    assert ea.compareCytosineReports(a, b, report_file=str(tmp_path / "cmp.tsv"), **kw) is None
    assert ea.generateDmrReport(a, b, report_file=str(tmp_path / "dmr.tsv"), **kw, **region_kw) is None
    lev = {"rname": LEVELS[:2], "strand": ("+", "-"), "context": got.levels["context"]}
    _assert_round_trip(got, str(tmp_path / "cmp.tsv"), X.CMP_INT, X.CMP_FLOAT, lev)
    _assert_round_trip(got_r, str(tmp_path / "dmr.tsv"), X.DMR_INT, X.DMR_FLOAT, lev)
    # the comparison left nothing behind on either batch
    for x, (cx, het) in zip((a, b), before):
        H.assert_reports_equal(ea.generateHeterogeneityReport(x, window_sites=3), het, float_cols=("beta", "epipolymorphism", "entropy", "pdr"))
        H.assert_reports_equal(ea.generateCytosineReport(x, **cx_kw), cx)


# ---- calls in sequence -----------------------------------------------------------------------------------------------------

def _assert_bitwise(got, want):
    assert list(got) == list(want) and got.ncommon == want.ncommon
    for k in got:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), k


def test_joins_in_sequence_keep_no_state(ea, samples):
    """The calls are stateless and give their scratch back: a join of 70 001 x 65 537 rows, a join of 6 x 7 rows at once,
    and the large one again give what they give alone, bit for bit; so do the samples' comparison and a small join."""
    rng = np.random.default_rng(17)
    big_a, big_b = X.random_cx_vec(rng, 70001, 15000), X.random_cx_vec(rng, 65537, 15000)
    first = gpu_join(ea, big_a, big_b, 3)
    small = gpu_join(ea, BASE, OTHER, 1)
    again = gpu_join(ea, big_a, big_b, 3)
    assert first.nrow > 30000 and small.nrow == 3
    _assert_bitwise(again, first)
    assert_join_equal(small, X.join_np(BASE, OTHER, 1))
    assert_join_equal(first, X.join_vec(big_a, big_b, 3))
    a, b = samples
    kw = dict(threshold_reads=False, min_coverage=4)
    alone = ea.compareCytosineReports(a, b, **kw)
    gpu_join(ea, big_a, big_b, 3)
    after_big = ea.compareCytosineReports(a, b, **kw)
    gpu_join(ea, BASE, OTHER, 1)
    _assert_bitwise(after_big, alone)
    _assert_bitwise(ea.compareCytosineReports(a, b, **kw), alone)


def test_a_sample_against_itself_and_swapped(ea, samples):
    """(a, a): every table is (m u / m u), p is exactly 1.0 and delta_beta +0.0.  (b, a) against (a, b): the same rows with
    the two sides exchanged, delta_beta negated bit for bit (0.0 - x: equal betas give +0.0 either way), p within RTOL and
    not bitwise, the table being transposed."""
    a, b = samples
    kw = dict(threshold_reads=False, min_coverage=4)
    same = ea.compareCytosineReports(a, a, **kw)
    assert same.nrow > 100 and same.ncommon == ea.generateCytosineReport(a, threshold_reads=False).nrow
    assert np.all(same["p"] == 1.0) and np.all(bits(same["delta_beta"]) == 0)
    assert np.array_equal(same["meth_a"], same["meth_b"]) and np.array_equal(same["unmeth_a"], same["unmeth_b"])
    assert np.array_equal(bits(same["beta_a"]), bits(same["beta_b"]))
    ab, ba = ea.compareCytosineReports(a, b, **kw), ea.compareCytosineReports(b, a, **kw)
    assert ab.nrow > 100 and ab.ncommon == ba.ncommon
    for k in ("rname", "strand", "pos", "context"):
        assert np.array_equal(ab[k], ba[k]), k
    for k in ("meth", "unmeth", "beta"):
        assert np.array_equal(ab[k + "_a"].view(np.uint8), ba[k + "_b"].view(np.uint8)), k
        assert np.array_equal(ab[k + "_b"].view(np.uint8), ba[k + "_a"].view(np.uint8)), k
    assert np.array_equal(bits(ba["delta_beta"]), bits(0.0 - ab["delta_beta"]))
    X.compare_p(ba["p"], ab["p"], np.stack([ab[k] for k in X.CMP_INT[4:]], 1), RTOL)


def test_comparison_calls_between_other_reports(ea, samples):
    """adjustReport and the regions interleaved with the cytosine, heterogeneity and linkage reports of both batches: those
    are what they were before, and the comparison is what it is alone."""
    a, b = samples
    het_floats, link_floats = ("beta", "epipolymorphism", "entropy", "pdr"), ("cov", "r2", "dprime")

    def others(x):
        return (ea.generateCytosineReport(x, threshold_reads=False), ea.generateHeterogeneityReport(x, window_sites=3),
                ea.generateLinkageReport(x, max_neighbours=2))

    def check(x, before):
        cx, het, link = others(x)
        H.assert_reports_equal(cx, before[0])
        H.assert_reports_equal(het, before[1], float_cols=het_floats)
        H.assert_reports_equal(link, before[2], float_cols=link_floats)

    before = [others(x) for x in (a, b)]
    assert all(r.nrow > 50 for pair in before for r in pair)
    kw = dict(threshold_reads=False, min_coverage=4)
    want = X.join_np(before[0][0], before[1][0], 4)
    want_r = X.regions_np(want, 0.05, 0.2, 30, 3)
    assert want_r["rname"].size >= 1
    table = ea.compareCytosineReports(a, b, as_device=True, **kw)
    check(a, before[0])
    adjusted = ea.adjustReport(table, "BH")
    check(b, before[1])
    regions = ea.rcpp_cx_compare_regions(adjusted, 0.05, 0.2, 30, 3)
    ea.generateLinkageReport(a, max_neighbours=2)
    on_q = ea.rcpp_cx_compare_regions(adjusted, 0.2, 0.2, 30, 3, significance="q")
    check(a, before[0])
    check(b, before[1])
    assert_regions_equal(regions, want_r)
    host = ea.Report({k: v.cpu().numpy() for k, v in table.items()}, table.levels["rname"])
    host.ncommon = table.ncommon
    assert_join_equal(host, want)
    assert np.array_equal(bits(adjusted["q"].cpu().numpy()), bits(ea.adjustPValues(table["p"].cpu().numpy(), "BH")))
    again = ea.rcpp_cx_compare_regions(ea.adjustReport(ea.compareCytosineReports(a, b, as_device=True, **kw), "BH"), 0.2, 0.2, 30, 3,
                                       significance="q")
    assert on_q.nrow >= 1 and list(on_q) == list(again)
    for k in on_q:
        assert np.array_equal(on_q[k].view(np.uint8), again[k].view(np.uint8)), k
