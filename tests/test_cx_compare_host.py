"""compareCytosineReports / generateDmrReport / fisherExact on the host side: the exported symbols, the functions' signatures,
argument checks before any I/O, the sequence-name check before anything touches a device, the loud failure without a
device (join, Fisher test and regions run on the GPU; there is no CPU path), the numpy restatement the GPU tests compare
against on a hand-written table (tests/cx_compare_np.py), that none of the Fisher tables of the GPU test sits so close
to the tie band that a few ulp in P could move a table from one side to the other, the host Fisher test against exact
arithmetic, and the restatements and tables that test_gpu_cx_compare_seams.py relies on."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import cx_compare_np as X
import helpers as H
import epialleler_amd as ea
from epialleler_amd import _lib

NEW_SYMBOLS = ("epi_fisher_exact_dev", "epi_cx_compare_dev", "epi_cx_compare_regions_dev")
EMPTY = inspect.Parameter.empty
CYTOSINE_ARGS = [("bam_a", EMPTY), ("bam_b", EMPTY), ("report_file", None), ("threshold_reads", True), ("threshold_context", None),
                 ("min_context_sites", 2), ("min_context_beta", 0.5), ("max_outofcontext_beta", 0.1), ("report_context", None),
                 ("min_coverage", 1), ("gzip", False), ("verbose", False), ("as_device", False)]


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def _two_rows(levels=None):
    t = H.templates_from_xm(["Z.z.Z.z", "z.Z.z.Z"], [1, 1], [1, 1])
    return ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"], levels)


def test_symbols_declared_exported_and_listed():
    _lib.build()
    with open(os.path.join(H.GOLDEN, "..", "..", "include", "epihip.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(_lib.load(), name)
        assert re.search(r"\bint %s\(epi_engine \*e," % name, hdr)
    with open(os.path.join(_lib.CSRC, "Makefile")) as f:
        assert re.search(r"^SRCS := .*\bcx_compare\.hip\b", f.read(), flags=re.M)


def test_one_copy_of_the_arithmetic():
    """fisher.cpp and cx_compare.hip both take stirlerr, bd0, dbinom_raw, Hyper and fisher_two_sided from fisher_math.hpp."""
    src = {}
    for name in ("fisher.cpp", "cx_compare.hip", "fisher_math.hpp"):
        with open(os.path.join(_lib.CSRC, name)) as f:
            src[name] = f.read()
    for fn in ("stirlerr", "bd0", "dbinom_raw", "fisher_two_sided"):
        assert len(re.findall(r"double %s\(" % fn, src["fisher_math.hpp"])) == 1
        assert not re.search(r"double %s\(" % fn, src["fisher.cpp"] + src["cx_compare.hip"])
    assert "struct Hyper" in src["fisher_math.hpp"] and "struct Hyper" not in src["fisher.cpp"] + src["cx_compare.hip"]
    for name in ("fisher.cpp", "cx_compare.hip"):
        assert '#include "fisher_math.hpp"' in src[name]


def test_signatures_and_defaults():
    p = inspect.signature(ea.compareCytosineReports).parameters
    assert [(k, v.default) for k, v in p.items() if v.kind is not v.VAR_KEYWORD] == CYTOSINE_ARGS
    assert [k for k, v in p.items() if v.kind is v.VAR_KEYWORD] == ["preprocess_args"]
    p = inspect.signature(ea.generateDmrReport).parameters
    assert [(k, v.default) for k, v in p.items() if v.kind is not v.VAR_KEYWORD] == CYTOSINE_ARGS + [
        ("max_p", 0.05), ("min_delta_beta", 0.1), ("max_gap", 500), ("min_sites", 3)]
    assert [k for k, v in p.items() if v.kind is v.VAR_KEYWORD] == ["preprocess_args"]
    q = inspect.signature(ea.rcpp_cx_compare).parameters
    assert [(k, v.default) for k, v in q.items()] == [("rep_a", EMPTY), ("rep_b", EMPTY), ("min_coverage", 1), ("as_device", False)]
    q = inspect.signature(ea.fisherExact).parameters
    assert [(k, v.default) for k, v in q.items()] == [("a", EMPTY), ("b", EMPTY), ("c", EMPTY), ("d", EMPTY), ("as_device", False)]
    # the same cytosine arguments, in the same order, as the report the tables come from
    g = inspect.signature(ea.generateCytosineReport).parameters
    assert [k for k in g if k != "bam"] == [k for k in p if k not in ("bam_a", "bam_b", "min_coverage", "max_p", "min_delta_beta", "max_gap",
                                                                      "min_sites")]


BAD_COMMON = [dict(threshold_context="CpG"), dict(report_context="cg"), dict(min_coverage=-1), dict(min_coverage=1.5),
              dict(min_coverage=True)]
BAD_DMR = [dict(max_p=-0.1), dict(max_p=1.5), dict(max_p=float("nan")), dict(min_delta_beta=-0.01), dict(min_delta_beta=2),
           dict(max_gap=-1), dict(max_gap=0.5), dict(min_sites=0), dict(min_sites=2.5), dict(min_sites=True)]
MESSAGES = {"threshold_context": "'threshold.context' should be one of 'CG', 'CHG', 'CHH', 'CxG', 'CX'",
            "report_context": "'report.context' should be one of 'CG', 'CHG', 'CHH', 'CxG', 'CX'",
            "min_coverage": "'min.coverage' should be an integer from 0 to 2147483647",
            "max_p": "'max.p' should be a number from 0 to 1", "min_delta_beta": "'min.delta.beta' should be a number from 0 to 1",
            "max_gap": "'max.gap' should be an integer from 0 to 2147483647", "min_sites": "'min.sites' should be an integer from 1 to 2147483647"}


@pytest.mark.parametrize("fn,kw", [("compareCytosineReports", kw) for kw in BAD_COMMON] +
                         [("generateDmrReport", kw) for kw in BAD_COMMON + BAD_DMR])
def test_bad_arguments_raise_before_io(fn, kw):
    with pytest.raises(ValueError) as ei:
        getattr(ea, fn)("no-such-file.bam", "no-such-file-either.bam", **kw)    # (opening one would raise "Unable to open BAM file")
    msg = str(ei.value)
    (name,) = kw
    assert MESSAGES[name] in msg
    assert "no-such-file" not in msg and "open" not in msg


def test_good_arguments_reach_the_file():
    for fn, kw in (("compareCytosineReports", dict(min_coverage=0)), ("compareCytosineReports", dict(report_context="CX", threshold_reads=False)),
                   ("generateDmrReport", dict(max_p=0, min_delta_beta=1, max_gap=0, min_sites=1)), ("generateDmrReport", dict(max_p=1))):
        with pytest.raises(Exception) as ei:
            getattr(ea, fn)("no-such-file.bam", "no-such-file-either.bam", **kw)
        assert not isinstance(ei.value, ValueError) or "should be" not in str(ei.value)


@pytest.mark.parametrize("cells", [([1.5], [1], [1], [1]), ([1], [2, 3], [1], [1]), (["x"], [1], [1], [1]), ([2 ** 31], [1], [1], [1])])
def test_fisher_exact_bad_cells_raise_before_the_device(cells):
    with pytest.raises(ValueError) as ei:
        ea.fisherExact(*cells)
    assert "should h" in str(ei.value)


def test_differing_levels_raise_before_the_device():
    """rname codes are comparable under one sequence dictionary only; the check needs no device (without one the call
    would raise EpihipError, with one it would upload)."""
    a, b = _two_rows(["chr1", "chr2"]), _two_rows(["chr2", "chr1"])
    for call in (lambda: ea.compareCytosineReports(a, b), lambda: ea.generateDmrReport(a, b),
                 lambda: ea.compareCytosineReports(a, _two_rows(None)), lambda: ea.generateDmrReport(a, _two_rows(["chr1"])),
                 lambda: ea.rcpp_cx_compare(ea.Report({}, ["chr1"]), ea.Report({}, ["chr2"]))):
        with pytest.raises(ValueError) as ei:
            call()
        assert "levels" in str(ei.value)
    assert a._batch is None and b._batch is None           # nothing was uploaded


def test_null_and_bad_arguments_of_the_library():
    lib = _lib.load()
    n = C.c_int64(-1)
    assert lib.epi_fisher_exact_dev(None, None, None, None, None, 0, None, None) == _lib.EPI_ERR_ARG
    assert lib.epi_cx_compare_dev(None, None, 0, None, 0, 1, None, None, 0, None, C.byref(n), C.byref(n)) == _lib.EPI_ERR_ARG
    assert lib.epi_cx_compare_regions_dev(None, None, None, 0, 0.05, 0.1, 500, 3, None, None, 0, None, C.byref(n)) == _lib.EPI_ERR_ARG
    assert b"NULL" in lib.epi_last_error()


def test_fails_loudly_without_gpu():
    if _has_gpu():
        pytest.skip("GPU present")
    a, b = _two_rows(), _two_rows()
    for call in (lambda: ea.compareCytosineReports(a, b), lambda: ea.generateDmrReport(a, b, threshold_reads=False),
                 lambda: ea.fisherExact([3], [1], [1], [3])):
        with pytest.raises(ea.EpihipError) as ei:
            call()
        assert ei.value.code == 5 and "no CPU fallback" in str(ei.value)


def test_restatement_on_the_hand_written_table():
    """Join and regions of tests/cx_compare_np.py on its hand-written pair of tables: a shared position with differing
    contexts, runs broken by max_gap, by a direction flip, by an rname change and by an insignificant row."""
    assert X.is_sorted(X.KAT_A) and X.is_sorted(X.KAT_B)
    k = X.KAT_ARGS
    table = X.join_np(X.KAT_A, X.KAT_B, k["min_coverage"])
    assert table["ncommon"] == X.KAT_NCOMMON
    regions = X.regions_np(table, k["max_p"], k["min_delta_beta"], k["max_gap"], k["min_sites"])
    X.check_kat(table, regions)
    assert table["p"][9] == pytest.approx(X.KAT_P_3113, rel=1e-12)
    assert X.join_np(X.KAT_A, X.KAT_B, 1)["pos"].tolist() == X.KAT_POS + [700]
    # min_sites = 1: the single significant row at 600 is a region of its own; a wide max_gap joins the first two runs
    assert X.regions_np(table, 0.05, 0.1, 100, 1)["start"].tolist() == [10, 300, 320, 330, 350, 352, 600]
    assert X.regions_np(table, 0.05, 0.1, 250, 2)["nsites"].tolist() == [5, 2, 2, 2, 3]
    assert X.regions_np(table, 0.0, 0.1, 100, 2)["start"].size == 0


def test_restatement_on_random_tables_has_what_the_gpu_tests_need():
    rng = np.random.default_rng(5)
    t = X.random_comparison(rng, 1000)
    r = X.regions_np(t, 0.05, 0.1, 300, 1)
    assert set(range(1, 17)) | {20} <= set(r["nsites"].tolist())          # (neighbouring stretches of one direction merge)
    assert {-1, 1} == set(r["direction"].tolist()) and np.isnan(t["p"]).any() and np.isnan(t["delta_beta"]).any()
    a, b = X.random_cx(rng, 1003, 400), X.random_cx(rng, 997, 400)
    assert X.is_sorted(a) and X.is_sorted(b)
    j = X.join_np(a, b, 25)
    assert 100 < j["pos"].size < j["ncommon"] - 50 and j["ncommon"] < 900


def test_fisher_tables_stay_clear_of_the_tie_band():
    """A table k counts as extreme when P(k) / P(a) <= 1 + 1e-7.  Host and device evaluate P with different lgamma / log /
    exp, a few ulp apart; a ratio within 1e-9 of the band could fall on either side and change p by a whole term.  No table
    of the GPU test has one: the nearest is an exact tie (ratio 1, 1e-7 below the band)."""
    tables = np.concatenate([X.small_tables(), X.LARGE_TABLES])
    worst = min(X.tie_band_distance(t) for t in tables[~X.degenerate(tables)])
    assert worst > 1e-9, worst
    assert worst == pytest.approx(1e-7, rel=1e-6)


def test_fisher_host_values_of_the_listed_tables():
    """The host side of the GPU test's comparison: NaN, exact ones and the underflow are where the test expects them."""
    t, p = X.fisher_cases()
    assert np.array_equal(np.isnan(p), (t < 0).any(axis=1)) and np.isnan(p).sum() == len(X.NEGATIVE_TABLES)
    ok = ~np.isnan(p)
    assert np.all(p[ok & X.degenerate(t)] == 1.0) and np.all((p[ok] >= 0) & (p[ok] <= 1))
    large = dict(zip(map(tuple, X.LARGE_TABLES.tolist()), p[len(X.small_tables()):]))
    assert large[(2000, 0, 0, 2000)] == 0.0 and large[(0, 5000, 5000, 0)] == 0.0
    assert large[(37, 37, 37, 37)] == 1.0 and 0 < large[(2 ** 31 - 1, 3, 5, 4)] < 1 and 0 < large[(1000000, 999000, 998500, 1000000)] < 1
    assert p[np.flatnonzero((t == (3, 1, 1, 3)).all(axis=1))[0]] == pytest.approx(X.KAT_P_3113, rel=1e-12)


def test_fisher_host_against_exact_arithmetic():
    """The host epi_fisher_exact against a 60-digit sum by the same rule (cx_compare_np.exact_fisher: exact fractions for a
    range of at most 400 tables, loggamma and the ratio recurrence beyond) on LARGE_TABLES, three tables with cells near
    2^31 and every 7th table with cells 0 .. 6.  Device and host share fisher_math.hpp, so this is the one place where a
    mistake in the header shows; the scipy pin of test_vcf_host.py stops at cells of 30 000.  Four tables whose exact p is
    below 1e-280 are left out, as there.  Measured: largest relative error 1.002e-13, at (480, 20, 100, 300) with
    p = 9.06e-122 (the exponent scales it); the near-2^31 tables are at 4.9e-15, 7.1e-16 and 2.5e-15.  The bound is 8 times
    the measured figure, 8.02e-13.  With log1p(-x / n) in dbinom_raw's lf, as it was, the near-2^31 tables were off by
    2.1e-9, 1.2e-9 and 1.0e-10."""
    t, _, _ = X.exact_values()
    rel, t = X.worst_exact_error(X.host_fisher(*t.T), "host")
    for row in X.NEAR_INT32_TABLES.tolist():
        i = int(np.flatnonzero((t == row).all(axis=1))[-1])
        print("  %s: %.3e" % (tuple(row), rel[i]))
        assert rel[i] <= X.EXACT_RTOL, (row, rel[i])
    assert rel.max() <= X.EXACT_RTOL, (rel.max(), t[int(rel.argmax())].tolist())


def test_exact_fisher_on_known_values():
    """The reference itself: the hand-computed (3 1 / 1 3), both of its paths on one table, its zero and its one."""
    assert float(X.exact_fisher(3, 1, 1, 3)) == pytest.approx(X.KAT_P_3113, rel=1e-15)
    for row in ((200, 100, 90, 250), (12, 1, 3, 11), (600, 700, 800, 500)):
        by_fractions, by_loggamma = X.exact_fisher(*row, exact_below=10 ** 9), X.exact_fisher(*row, exact_below=0)
        assert abs(by_loggamma / by_fractions - 1) < 1e-40
    assert X.exact_fisher(0, 4, 0, 8) == 1 and X.exact_fisher(37, 37, 37, 37) == 1
    assert X.exact_fisher(3 * X.M31, 0, 0, 3 * X.M31) == 0 and X.exact_fisher(2000, 0, 0, 2000) == 0
    assert all(X.tie_band_distance(row) > 1e-9 for row in X.NEAR_INT32_TABLES)


def test_vectorised_join_equals_the_loop():
    """join_vec (searchsorted on a packed key, one Fisher test per distinct table), which the million-row GPU test compares
    with, against join_np on tables small enough for the loop."""
    rng = np.random.default_rng(41)
    empty = X.cx_table([])
    edge = X.cx_table([(0, 0, 0, 6, 1, 2), (X.M31, 1, X.M31, 6, X.M31, X.M31), (X.M31, 2, X.M31, 5, 0, 0)])
    pairs = [(X.KAT_A, X.KAT_B), (X.KAT_B, X.KAT_A), (empty, X.KAT_A), (X.KAT_A, empty), (empty, empty), (edge, edge), (X.KAT_A, edge),
             (X.random_cx(rng, 1003, 400), X.random_cx(rng, 997, 400)), (X.random_cx_vec(rng, 4097, 3000, depth=7), X.random_cx_vec(rng, 700, 3000, depth=7))]
    for a, b in pairs:
        assert X.is_sorted(a) and X.is_sorted(b)
        for min_coverage in (0, 1, 6, 25, X.M31):
            want, got = X.join_np(a, b, min_coverage), X.join_vec(a, b, min_coverage)
            assert got["ncommon"] == want["ncommon"]
            for k in X.CMP_INT + X.CMP_FLOAT:
                assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k], equal_nan=True), k
    assert X.join_vec(edge, edge, X.M31)["pos"].tolist() == [X.M31]          # coverage 2^32 - 2 is not wrapped


def test_long_stretches_have_what_the_gpu_test_needs():
    """The table of the min_sites = 300 and 5000 test: at least 3 regions reported and at least 3 runs too short for each."""
    t = X.long_stretches_table()
    runs = X.regions_np(t, 0.05, 0.1, 50, 1)
    assert sorted(runs["nsites"].tolist()) == sorted(ln for ln, st in X.LONG_STRETCHES if st)
    for min_sites in X.LONG_MIN_SITES:
        r = X.regions_np(t, 0.05, 0.1, 50, min_sites)
        assert r["rname"].size >= 3 and runs["rname"].size - r["rname"].size >= 3
        assert r["nsites"].tolist() == [v for v in runs["nsites"].tolist() if v >= min_sites]
    starts = np.cumsum([0] + [ln for ln, _ in X.LONG_STRETCHES])
    assert len(set((starts // 256).tolist())) > 10 and len(set((starts // 4096).tolist())) > 5


def test_restatement_on_pooled_cells_beyond_int32():
    """regions_np on the hand-made wide tables: pooled cells of 2^31 and more, p from exact_fisher there, exactly 1 on the
    degenerate run and exactly 0 on the run whose p underflows; a region that fits int32 keeps the host's p."""
    seen = set()
    for name, (t, args) in sorted(X.wide_tables().items()):
        r = X.regions_np(t, *args)
        cells = r["cells"]
        assert cells.dtype == np.int64 and cells.shape[0] >= 4 and np.all(cells.max(axis=1) >= 2 ** 31)
        assert 2 <= r["nsites"].min() and r["nsites"].max() <= 4
        assert r["p"][-2] == 1.0 and bool(X.degenerate(cells)[-2]) and r["p"][-1] == 0.0
        assert np.all((r["p"][:-2] > 1e-30) & (r["p"][:-2] < 1))
        n1, n2, m = cells[:, 0] + cells[:, 1], cells[:, 2] + cells[:, 3], cells[:, 0] + cells[:, 2]
        assert np.all((np.minimum(m, n1) - np.maximum(0, m - n2))[:-1] < 40)
        assert r["beta_a"][0] == cells[0, 0] / (cells[0, 0] + cells[0, 1])
        seen.update(np.rint(cells.max(axis=1) / X.M31).astype(int).tolist())
    assert seen == {2, 3, 4}                               # pooled sums of about 4.3e9, 6.4e9 and 8.6e9
    # below 2^31 nothing changes: the host's p, bit for bit
    small = X.random_comparison(np.random.default_rng(5), 300)
    r = X.regions_np(small, 0.05, 0.1, 300, 1)
    assert np.array_equal(r["p"], X.host_fisher(*r["cells"].T))
