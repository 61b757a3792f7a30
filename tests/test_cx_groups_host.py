"""compareCytosineGroups / generateGroupDmrReport / rcpp_cx_compare_groups / chisqPValues / tTestPValues on the host side:
the exported symbols, the functions' signatures, argument checks before any I/O, the checks that need no device, the loud
failure without one (join and tests run on the GPU; there is no CPU path), epi_cx_groups_scratch_bytes, and the numpy
restatement the GPU tests compare against (tests/cx_groups_np.py) on a hand-written table and against scipy."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import cx_compare_np as X
import cx_groups_np as G
import helpers as H
import epialleler_amd as ea
from epialleler_amd import _lib

NEW_SYMBOLS = ("epi_dist_tail", "epi_dist_tail_dev", "epi_cx_groups_dev", "epi_cx_groups_scratch_bytes")
EMPTY = inspect.Parameter.empty
GROUP_ARGS = [("bams_a", EMPTY), ("bams_b", EMPTY), ("report_file", None), ("threshold_reads", True), ("threshold_context", None),
              ("min_context_sites", 2), ("min_context_beta", 0.5), ("max_outofcontext_beta", 0.1), ("report_context", None),
              ("min_coverage", 1), ("min_samples", None), ("test", "lrt"), ("gzip", False), ("verbose", False), ("as_device", False)]


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
        text = f.read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(_lib.load(), name)
        assert re.search(r"\bint %s\(" % name, hdr)
    for name, value in (("EPI_DIST_CHISQ", 0), ("EPI_DIST_T2", 1), ("EPI_DIST_F1", 2), ("EPI_CXG_FISHER", 0), ("EPI_CXG_LRT", 1),
                        ("EPI_CXG_LRT_MN", 2), ("EPI_CXG_WELCH", 3), ("EPI_CXG_MAX_RNAME", G.MAX_RNAME)):
        assert re.search(r"^#define %s\s+%d$" % (name, value), hdr, flags=re.M), name
    with open(os.path.join(_lib.CSRC, "Makefile")) as f:
        mk = f.read()
    assert re.search(r"^SRCS := .*\bcx_groups\.hip\b", mk, flags=re.M) and re.search(r"^HOST_SRCS := .*\bdist\.cpp\b", mk, flags=re.M)
    assert ea.GROUP_COMPARE_COLUMNS == G.GROUP_COLUMNS and ea.GROUP_TESTS == ("lrt", "lrt_mn", "welch", "fisher")
    # the names adjustReport and rcpp_cx_compare_regions read are those of the two-sample table
    assert set(ea.api.CX_COMPARE_COLUMNS) <= set(ea.GROUP_COMPARE_COLUMNS)


def test_signatures_and_defaults():
    p = inspect.signature(ea.compareCytosineGroups).parameters
    assert [(k, v.default) for k, v in p.items() if v.kind is not v.VAR_KEYWORD] == GROUP_ARGS
    assert [k for k, v in p.items() if v.kind is v.VAR_KEYWORD] == ["preprocess_args"]
    p = inspect.signature(ea.generateGroupDmrReport).parameters
    assert [(k, v.default) for k, v in p.items() if v.kind is not v.VAR_KEYWORD] == GROUP_ARGS + [
        ("max_q", 0.05), ("min_delta_beta", 0.1), ("max_gap", 500), ("min_sites", 3), ("p_adjust", "BH")]
    assert [k for k, v in p.items() if v.kind is v.VAR_KEYWORD] == ["preprocess_args"]
    q = inspect.signature(ea.rcpp_cx_compare_groups).parameters
    assert [(k, v.default) for k, v in q.items()] == [("reps_a", EMPTY), ("reps_b", EMPTY), ("min_coverage", 1), ("min_samples_a", None),
                                                      ("min_samples_b", None), ("test", "lrt"), ("as_device", False)]
    for fn, first in ((ea.chisqPValues, "stat"), (ea.tTestPValues, "t")):
        q = inspect.signature(fn).parameters
        assert [(k, v.default) for k, v in q.items()] == [(first, EMPTY), ("df", EMPTY), ("as_device", False)]
    # the thresholding arguments and defaults of compareCytosineReports, in its order
    c = inspect.signature(ea.compareCytosineReports).parameters
    shared = [k for k in c if k not in ("bam_a", "bam_b")]
    assert [(k, p[k].default) for k in shared] == [(k, c[k].default) for k in shared]
    # generateAdjustedDmrReport's region arguments
    a = inspect.signature(ea.generateAdjustedDmrReport).parameters
    for k in ("max_q", "min_delta_beta", "max_gap", "min_sites", "p_adjust"):
        assert p[k].default == a[k].default


BAD_COMMON = [dict(threshold_context="CpG"), dict(report_context="cg"), dict(min_coverage=-1), dict(min_coverage=1.5), dict(min_coverage=True),
              dict(test="t"), dict(test="LRT"), dict(min_samples=0), dict(min_samples=3), dict(min_samples=(1, 3)), dict(min_samples=(0, 1)),
              dict(min_samples=1.5), dict(min_samples=True), dict(min_samples=(1, 1, 1))]
BAD_DMR = [dict(max_q=-0.1), dict(max_q=1.5), dict(max_q=float("nan")), dict(min_delta_beta=-0.01), dict(min_delta_beta=2),
           dict(max_gap=-1), dict(max_gap=0.5), dict(min_sites=0), dict(min_sites=2.5), dict(min_sites=True), dict(p_adjust="hommel"),
           dict(p_adjust="bh")]
MESSAGES = {"threshold_context": "'threshold.context' should be one of 'CG', 'CHG', 'CHH', 'CxG', 'CX'",
            "report_context": "'report.context' should be one of 'CG', 'CHG', 'CHH', 'CxG', 'CX'",
            "min_coverage": "'min.coverage' should be an integer from 0 to 2147483647",
            "test": "'test' should be one of 'lrt', 'lrt_mn', 'welch', 'fisher'",
            "min_samples": "'min.samples' should be an integer",
            "max_q": "'max.q' should be a number from 0 to 1", "min_delta_beta": "'min.delta.beta' should be a number from 0 to 1",
            "max_gap": "'max.gap' should be an integer from 0 to 2147483647", "min_sites": "'min.sites' should be an integer from 1 to 2147483647",
            "p_adjust": "'p.adjust' should be one of 'holm', 'hochberg', 'bonferroni', 'BH', 'BY', 'fdr', 'none'"}
FILES = (["no-such-file.bam", "no-such-file-2.bam"], ["no-such-file-either.bam", "no-such-file-4.bam"])


@pytest.mark.parametrize("fn,kw", [("compareCytosineGroups", kw) for kw in BAD_COMMON] +
                         [("generateGroupDmrReport", kw) for kw in BAD_COMMON + BAD_DMR])
def test_bad_arguments_raise_before_io(fn, kw):
    with pytest.raises(ValueError) as ei:
        getattr(ea, fn)(*FILES, **kw)                       # (opening one would raise "Unable to open BAM file")
    msg = str(ei.value)
    (name,) = kw
    assert MESSAGES[name] in msg
    assert "no-such-file" not in msg and "open" not in msg


@pytest.mark.parametrize("groups", [([], ["b.bam"]), (["a.bam"], []), (["a.bam"] * 33, ["b.bam"]), (["a.bam"], ["b.bam"] * 33),
                                    ("a.bam", ["b.bam"]), (["a.bam"], "b.bam")])
def test_bad_groups_raise_before_io(groups):
    for fn in (ea.compareCytosineGroups, ea.generateGroupDmrReport):
        with pytest.raises(ValueError) as ei:
            fn(*groups)
        assert "1 to 32 inputs" in str(ei.value) and "open" not in str(ei.value)


def test_good_arguments_reach_the_file():
    for fn, kw in (("compareCytosineGroups", dict(min_coverage=0)), ("compareCytosineGroups", dict(min_samples=1, test="welch")),
                   ("compareCytosineGroups", dict(min_samples=(2, 1), test="fisher", report_context="CX", threshold_reads=False)),
                   ("compareCytosineGroups", dict(min_samples=2, test="lrt_mn")), ("compareCytosineGroups", dict(test=None)),
                   ("generateGroupDmrReport", dict(max_q=0, min_delta_beta=1, max_gap=0, min_sites=1, p_adjust="none")),
                   ("generateGroupDmrReport", dict(max_q=1, p_adjust="BY"))):
        with pytest.raises(Exception) as ei:
            getattr(ea, fn)(*FILES, **kw)
        assert not isinstance(ei.value, ValueError) or "should be" not in str(ei.value)


def test_group_checks_need_no_device():
    """Differing levels, an empty group, 33 reports and a minimum outside its group raise before anything touches a device
    (without one the call would raise EpihipError, with one it would upload)."""
    a, b = _two_rows(["chr1", "chr2"]), _two_rows(["chr2", "chr1"])
    for call in (lambda: ea.compareCytosineGroups([a, a], [a, b]), lambda: ea.generateGroupDmrReport([a], [_two_rows(None)]),
                 lambda: ea.rcpp_cx_compare_groups([ea.Report({}, ["chr1"])], [ea.Report({}, ["chr1"]), ea.Report({}, ["chr2"])])):
        with pytest.raises(ValueError) as ei:
            call()
        assert "levels" in str(ei.value)
    assert a._batch is None and b._batch is None           # nothing was uploaded
    r = ea.Report({}, ["chr1"])
    for kw, text in ((dict(reps_a=[], reps_b=[r]), "'reps_a' should hold 1 to 32 reports"), (dict(reps_a=[r], reps_b=[r] * 33), "'reps_b' should hold 1 to 32 reports"),
                     (dict(reps_a=[r], reps_b=[r], min_samples_a=2), "'min.samples.a' should be an integer from 1 to 1"),
                     (dict(reps_a=[r], reps_b=[r, r], min_samples_b=0), "'min.samples.b' should be an integer from 1 to 2"),
                     (dict(reps_a=[r], reps_b=[r], test="wald"), "'test' should be one of"),
                     (dict(reps_a=[r], reps_b=[r], min_coverage=-1), "'min.coverage' should be")):
        with pytest.raises(ValueError) as ei:
            ea.rcpp_cx_compare_groups(**kw)
        assert text in str(ei.value)
    with pytest.raises(TypeError):                          # host tables are no device Reports
        ea.rcpp_cx_compare_groups([ea.Report(G.KAT_A[0], ["chr1", "chr2"])], [ea.Report(G.KAT_B[0], ["chr1", "chr2"])])


@pytest.mark.parametrize("fn", ["chisqPValues", "tTestPValues"])
def test_tail_bad_values_raise_before_the_device(fn):
    for args in ((["x"], [1]), ([1.0, 2.0], [1.0, 2.0, 3.0]), ([1.0], ["y"]), ([1.0], [])):
        with pytest.raises(ValueError) as ei:
            getattr(ea, fn)(*args)
        assert "should" in str(ei.value)


def test_null_and_bad_arguments_of_the_library():
    lib = _lib.load()
    n = C.c_int64(-1)
    rows = (C.c_int64 * 2)(0, 0)
    tabs = (C.c_void_p * 12)()
    assert lib.epi_cx_groups_dev(None, tabs, rows, 1, 1, 1, 1, 1, 1, None, None, 0, None, C.byref(n), C.byref(n)) == _lib.EPI_ERR_ARG
    assert b"NULL" in lib.epi_last_error()
    assert lib.epi_dist_tail_dev(None, 0, None, None, 0, None, None) == _lib.EPI_ERR_ARG


def test_scratch_bytes():
    lib = _lib.load()
    out = C.c_int64(-1)
    want = lambda n: 0 if n == 0 else 32 * n + ((n + 4095) // 4096) * 2048 + ((n + 4095) // 4096) * 4 + 64
    for n in (0, 1, 4096, 4097, 2 ** 32 - 1):
        assert lib.epi_cx_groups_scratch_bytes(n, C.byref(out)) == _lib.EPI_OK and out.value == want(n), n
    assert want(1) == 32 + 2048 + 4 + 64 and want(2 ** 32 - 1) > 2 ** 37
    for n in (2 ** 32, -1):
        assert lib.epi_cx_groups_scratch_bytes(n, C.byref(out)) == _lib.EPI_ERR_ARG and out.value == 0
    assert lib.epi_cx_groups_scratch_bytes(1, None) == _lib.EPI_ERR_ARG


def test_fails_loudly_without_gpu():
    if _has_gpu():
        pytest.skip("GPU present")
    a, b = _two_rows(), _two_rows()
    for call in (lambda: ea.compareCytosineGroups([a], [b]), lambda: ea.generateGroupDmrReport([a, a], [b], threshold_reads=False),
                 lambda: ea.chisqPValues([3.84], 1), lambda: ea.tTestPValues([2.0], [5.0])):
        with pytest.raises(ea.EpihipError) as ei:
            call()
        assert ei.value.code == 5 and "no CPU fallback" in str(ei.value)


# ---- the restatement ---------------------------------------------------------------------------------------------------

def test_restatement_on_the_hand_written_table():
    """2 + 3 samples, min_coverage 4: site 100 in every sample; (1, 200, -) missing from a's second sample; at 300 b's third
    sample is below the coverage; at 400 a's first sample has another context, which makes two sites; 500 all-methylated;
    600 with zero variance in either group."""
    for t in G.KAT_A + G.KAT_B:
        assert X.is_sorted(t)
    full = G.groups_np(G.KAT_A, G.KAT_B, G.KAT_MIN_COVERAGE, test="lrt")
    assert full["nsites"] == 7                                          # 100, 200, 300, 400 (CHG), 400 (CG), 500, 600
    assert full["pos"].tolist() == [100, 500, 600] and full["rname"].tolist() == [1, 1, 2]
    assert full["nsamples_a"].tolist() == [2] * 3 and full["nsamples_b"].tolist() == [3] * 3 and full["df"].tolist() == [1.0] * 3
    some = G.groups_np(G.KAT_A, G.KAT_B, G.KAT_MIN_COVERAGE, 1, 2, test="lrt_mn")
    assert some["nsites"] == 7 and some["pos"].tolist() == [100, 200, 300, 400, 500, 600] and some["context"].tolist() == [7] * 6
    assert some["strand"].tolist() == [1, 2, 1, 1, 1, 1]
    assert some["nsamples_a"].tolist() == [2, 1, 2, 1, 2, 2] and some["nsamples_b"].tolist() == [3, 3, 2, 3, 3, 3]
    assert some["df"].tolist() == [3.0, 2.0, 2.0, 2.0, 3.0, 3.0]
    assert (some["meth_b"][2], some["unmeth_b"][2]) == (17, 3)          # 300: b's third sample (2, 1) is left out of the pool
    assert (some["meth_a"][3], some["unmeth_a"][3]) == (5, 5)           # 400: a's first sample has another context
    assert (some["meth_a"][0], some["unmeth_a"][0], some["meth_b"][0], some["unmeth_b"][0]) == (14, 6, 6, 24)
    assert some["beta_a"][0] == 14 / 20 and some["mean_beta_a"][0] == (0.8 + 0.6) / 2 and some["mean_beta_b"][0] == (0.2 + 0.1 + 0.3) / 3
    assert some["var_a"][0] == pytest.approx(0.02, rel=1e-14) and some["var_b"][0] == pytest.approx(0.01, rel=1e-14)
    assert np.isnan(some["var_a"][1]) and not np.isnan(some["var_b"][1])
    assert np.all(some["phi"] >= 1.0) and np.all((some["p"] >= 0) & (some["p"] <= 1))
    # all-methylated: G = 0, p = 1 exactly
    i500, i600 = 4, 5
    for test in ("lrt", "lrt_mn"):
        r = G.groups_np(G.KAT_A, G.KAT_B, G.KAT_MIN_COVERAGE, 1, 2, test=test)
        assert r["stat"][i500] == 0.0 and r["p"][i500] == 1.0 and r["beta_a"][i500] == 1.0 and r["delta_beta"][i500] == 0.0
    f = G.groups_np(G.KAT_A, G.KAT_B, G.KAT_MIN_COVERAGE, 1, 2, test="fisher")
    assert f["p"][i500] == 1.0 and np.isnan(f["stat"]).all() and np.isnan(f["df"]).all() and np.isnan(f["phi"]).all()
    w = G.groups_np(G.KAT_A, G.KAT_B, G.KAT_MIN_COVERAGE, 1, 2, test="welch")
    assert np.isnan(w["stat"][i500]) and np.isnan(w["p"][i500]) and w["var_a"][i500] == 0.0          # s2 == 0
    # 600: betas 0.25, 0.25 against 0.75, 0.75, 0.75
    assert w["var_a"][i600] == 0.0 and w["var_b"][i600] == 0.0 and np.isnan(w["p"][i600]) and w["delta_beta"][i600] == 0.5
    assert np.isnan(w["stat"][1]) and np.isnan(w["df"][1]) and np.isnan(w["p"][1])                   # 200: one sample in a
    assert np.isnan(w["phi"]).all() and 0.05 < w["p"][0] < 0.1 and w["stat"][0] < 0 and 1 < w["df"][0] < 3
    # n = 2 with lrt_mn: no residual degree of freedom
    one = G.groups_np(G.KAT_A[:1], G.KAT_B[:1], 1, test="lrt_mn")
    assert one["pos"].size == 5 and np.all(one["df"] == 0.0) and np.isnan(one["stat"]).all() and np.isnan(one["phi"]).all() and np.isnan(one["p"]).all()
    # min_coverage 1 brings b's third sample back at 300
    assert G.groups_np(G.KAT_A, G.KAT_B, 1, test="welch")["pos"].tolist() == [100, 300, 500, 600]
    assert G.groups_np(G.KAT_A, G.KAT_B, 1, 1, 2, test="lrt")["meth_b"][2] == 19


@pytest.mark.filterwarnings("ignore:Precision loss occurred")          # (scipy, on a site whose betas are all equal)
def test_restatement_against_scipy():
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(11)
    a, b = G.random_groups(rng, 3, 4, 300, 400, depth=40)
    w = G.groups_np(a, b, 2, 2, 2, test="welch")
    lrt = G.groups_np(a, b, 2, 2, 2, test="lrt")
    mn = G.groups_np(a, b, 2, 2, 2, test="lrt_mn")
    assert w["pos"].size > 200 and np.array_equal(w["pos"], lrt["pos"]) and np.array_equal(w["pos"], mn["pos"])
    for k in G.GROUP_INT + G.GROUP_FLOAT[:7]:
        assert np.array_equal(w[k], lrt[k], equal_nan=True) and np.array_equal(w[k], mn[k], equal_nan=True), k
    # per-site samples, for scipy
    tabs = a + b
    lookup = [{G.site_key(t, i): (int(t["meth"][i]), int(t["unmeth"][i])) for i in range(t["pos"].size)} for t in tabs]
    checked = dict(welch=0, g=0, f=0)
    for r in range(w["pos"].size):
        key = (int(w["rname"][r]), int(w["pos"][r]), int(w["strand"][r]), int(w["context"][r]))
        betas = [[], []]
        for k, d in enumerate(lookup):
            if key in d and sum(d[key]) >= 2:
                betas[k >= 3].append(d[key][0] / sum(d[key]))
        assert (len(betas[0]), len(betas[1])) == (w["nsamples_a"][r], w["nsamples_b"][r])
        if not np.isnan(w["p"][r]):
            t, p = stats.ttest_ind(betas[1], betas[0], equal_var=False)
            assert w["stat"][r] == pytest.approx(t, rel=1e-10, abs=1e-13) and w["p"][r] == pytest.approx(p, rel=1e-9)
            checked["welch"] += 1
        cells = np.asarray([[lrt["meth_a"][r], lrt["unmeth_a"][r]], [lrt["meth_b"][r], lrt["unmeth_b"][r]]], np.float64)
        if (cells.sum(0) > 0).all():
            g, p, dof, _ = stats.chi2_contingency(cells, correction=False, lambda_="log-likelihood")
            assert dof == 1 and lrt["stat"][r] == pytest.approx(g, rel=1e-10, abs=1e-12) and lrt["p"][r] == pytest.approx(p, rel=1e-9)
            checked["g"] += 1
        else:
            assert lrt["stat"][r] == 0.0 and lrt["p"][r] == 1.0
        n = mn["nsamples_a"][r] + mn["nsamples_b"][r]
        assert mn["df"][r] == n - 2 and mn["phi"][r] >= 1.0 and mn["stat"][r] == lrt["stat"][r] / mn["phi"][r]
        assert mn["p"][r] == pytest.approx(stats.f.sf(mn["stat"][r], 1, n - 2), rel=1e-9)
        checked["f"] += 1
    assert min(checked.values()) > 100 and (mn["phi"] > 1.0).sum() > 20 and (mn["phi"] == 1.0).sum() > 20
    # a zero cell: the formula's own term, against scipy's G-test
    g, p, _, _ = stats.chi2_contingency([[0, 9], [7, 5]], correction=False, lambda_="log-likelihood")
    assert G.g_statistic(0, 9, 7, 5) == pytest.approx(g, rel=1e-13)
    assert G.g_statistic(5, 0, 9, 0) == 0.0 and G.g_statistic(0, 4, 0, 8) == 0.0


def test_fisher_with_one_sample_a_side_is_the_two_sample_join():
    rng = np.random.default_rng(5)
    a, b = X.random_cx(rng, 503, 300), X.random_cx(rng, 497, 300)
    for min_coverage in (0, 1, 25):
        want, got = X.join_np(a, b, min_coverage), G.groups_np([a], [b], min_coverage, test="fisher")
        for k in X.CMP_INT + X.CMP_FLOAT:
            assert np.array_equal(got[k], want[k], equal_nan=True), k
        assert got["pos"].size > 20


def test_random_groups_have_what_the_gpu_tests_need():
    rng = np.random.default_rng(2)
    a, b = G.random_groups(rng, 2, 1, 257, 400)
    r = G.groups_np(a, b, 3, 1, 1, test="lrt_mn")
    assert r["nsites"] > r["pos"].size > 50 and set(r["nsamples_a"].tolist()) == {1, 2} and set(r["strand"].tolist()) == {1, 2}
    assert (r["stat"] == 0).any() and np.isnan(r["p"]).any() and (r["df"] == 0).any() and (r["df"] == 1).any()
    assert len(set(r["context"].tolist())) >= 2 and len(set(r["rname"].tolist())) >= 2
    w = G.groups_np(*G.random_groups(rng, 3, 3, 200, 300), 1, 2, 2, test="welch")
    assert np.isnan(w["p"]).any() and (~np.isnan(w["p"])).sum() > 50
    d = G.groups_np(*G.random_groups(rng, 2, 1, 100, 200, disjoint=True), 1, 1, 1, test="lrt")
    assert d["pos"].size == 0 and d["nsites"] > 200
