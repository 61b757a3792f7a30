"""adjustPValues / adjustReport / generateAdjustedDmrReport on the host side: the exported symbol, the functions' signatures,
argument checks before any I/O or device, the loud failure without a device (keys, sort, scan and scatter run on the GPU;
there is no CPU path), the library's NULL and range checks, and the numpy restatement the GPU tests compare against
(tests/padjust_np.py): known answers, invariance under permutation bit for bit, agreement with brute-force definitions."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import helpers as H
import padjust_np as P
import epialleler_amd as ea
from epialleler_amd import _lib

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


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def test_symbol_declared_exported_and_listed():
    _lib.build()
    with open(os.path.join(H.GOLDEN, "..", "..", "include", "epihip.h")) as f:
        text = f.read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert "epi_p_adjust_dev" in _lib.EXPORTED_SYMBOLS and hasattr(_lib.load(), "epi_p_adjust_dev")
    assert re.search(r"\bint epi_p_adjust_dev\(epi_engine \*e, const double \*d_p, int64_t n, int32_t method, int64_t n_tests,", hdr)
    for name, code in P.CODES.items():
        assert re.search(r"#define EPI_PADJ_%s\s+%d\b" % (name.upper(), code), hdr)
        assert ea.api._P_ADJUST_CODES[name] == code
    assert ea.api._P_ADJUST_CODES["fdr"] == P.CODES["BH"]
    assert "No p-value is adjusted" not in text and "hommel" in text
    with open(os.path.join(_lib.CSRC, "Makefile")) as f:
        assert re.search(r"^SRCS := .*\bp_adjust\.hip\b", f.read(), flags=re.M)


def test_signatures_and_defaults():
    q = inspect.signature(ea.adjustPValues).parameters
    assert [(k, v.default) for k, v in q.items()] == [("p", EMPTY), ("method", "BH"), ("n_tests", None), ("as_device", False)]
    q = inspect.signature(ea.adjustReport).parameters
    assert [(k, v.default) for k, v in q.items()] == [("report", EMPTY), ("method", "BH"), ("column", "p"), ("name", "q"), ("n_tests", None)]
    q = inspect.signature(ea.rcpp_cx_compare_regions).parameters
    assert [(k, v.default) for k, v in q.items()] == [("rep", EMPTY), ("max_p", 0.05), ("min_delta_beta", 0.1), ("max_gap", 500), ("min_sites", 3),
                                                       ("as_device", False), ("significance", "p")]
    p = inspect.signature(ea.generateAdjustedDmrReport).parameters
    assert [(k, v.default) for k, v in p.items() if v.kind is not v.VAR_KEYWORD] == CYTOSINE_ARGS + [
        ("max_q", 0.05), ("min_delta_beta", 0.1), ("max_gap", 500), ("min_sites", 3), ("p_adjust", "BH")]
    assert [k for k, v in p.items() if v.kind is v.VAR_KEYWORD] == ["preprocess_args"]
    # generateDmrReport's arguments in its order, max_p renamed
    d = inspect.signature(ea.generateDmrReport).parameters
    assert [("max_q" if k == "max_p" else k) for k in d] == [k for k in p if k != "p_adjust"]
    assert ea.P_ADJUST_METHODS == ("holm", "hochberg", "bonferroni", "BH", "BY", "fdr", "none")


BAD_DMR = [dict(threshold_context="CpG"), dict(report_context="cg"), dict(min_coverage=-1), dict(max_q=-0.1), dict(max_q=1.5),
           dict(max_q=float("nan")), dict(min_delta_beta=2), dict(max_gap=-1), dict(min_sites=0), dict(p_adjust="hommel"), dict(p_adjust="bh"),
           dict(p_adjust=3)]
MESSAGES = {"threshold_context": "'threshold.context' should be one of", "report_context": "'report.context' should be one of",
            "min_coverage": "'min.coverage' should be an integer from 0 to 2147483647", "max_q": "'max.q' should be a number from 0 to 1",
            "min_delta_beta": "'min.delta.beta' should be a number from 0 to 1", "max_gap": "'max.gap' should be an integer from 0 to 2147483647",
            "min_sites": "'min.sites' should be an integer from 1 to 2147483647",
            "p_adjust": "'p.adjust' should be one of 'holm', 'hochberg', 'bonferroni', 'BH', 'BY', 'fdr', 'none'"}


@pytest.mark.parametrize("kw", BAD_DMR)
def test_bad_arguments_raise_before_io(kw):
    with pytest.raises(ValueError) as ei:
        ea.generateAdjustedDmrReport("no-such-file.bam", "no-such-file-either.bam", **kw)
    msg = str(ei.value)
    (name,) = kw
    assert MESSAGES[name] in msg
    assert "no-such-file" not in msg and "open" not in msg


def test_good_arguments_reach_the_file():
    for kw in (dict(max_q=0, p_adjust="none"), dict(max_q=1, p_adjust="fdr"), dict(p_adjust="BY", min_sites=1)):
        with pytest.raises(Exception) as ei:
            ea.generateAdjustedDmrReport("no-such-file.bam", "no-such-file-either.bam", **kw)
        assert not isinstance(ei.value, ValueError) or "should be" not in str(ei.value)


def _report():
    return ea.Report({"pos": np.arange(3, dtype=np.int32), "p": np.asarray([0.01, 0.5, np.nan])}, ["chr1"])


@pytest.mark.parametrize("call", [
    lambda: ea.adjustPValues([0.1], method="hommel"), lambda: ea.adjustPValues([0.1], method="bh"), lambda: ea.adjustPValues([0.1], n_tests=0),
    lambda: ea.adjustPValues([0.1], n_tests=1.5), lambda: ea.adjustPValues([0.1], n_tests=True), lambda: ea.adjustPValues([0.1], n_tests=2 ** 31),
    lambda: ea.adjustPValues([0.1], n_tests=float("inf")), lambda: ea.adjustPValues([0.1], n_tests="many"), lambda: ea.adjustPValues(["a", "b"]),
    lambda: ea.adjustPValues([0.1 + 1j]), lambda: ea.adjustPValues(None), lambda: ea.adjustReport(_report(), column="pvalue"),
    lambda: ea.adjustReport(_report(), name="pos"), lambda: ea.adjustReport(_report(), name=""), lambda: ea.adjustReport(_report(), method="x"),
    lambda: ea.adjustReport({"p": np.zeros(2)}), lambda: ea.adjustReport(_report(), n_tests=-3),
    lambda: ea.rcpp_cx_compare_regions(_report(), significance="fdr"), lambda: ea.rcpp_cx_compare_regions(_report(), max_p=2, significance="q")])
def test_bad_arguments_raise_before_the_device(call):
    """(without a device a call that reached it would raise EpihipError, not ValueError)"""
    with pytest.raises(ValueError) as ei:
        call()
    assert "should" in str(ei.value)


def test_null_and_bad_arguments_of_the_library():
    lib = _lib.load()
    n = C.c_int64(-1)
    assert lib.epi_p_adjust_dev(None, None, 0, 4, 0, None, None, None, C.byref(n)) == _lib.EPI_ERR_ARG
    assert b"NULL" in lib.epi_last_error()
    fake = C.c_void_p(16)                                   # an engine that is never dereferenced: the checks come first
    assert lib.epi_p_adjust_dev(fake, None, 0, 4, 0, None, None, None, None) == _lib.EPI_ERR_ARG
    for method in (-1, 6):
        assert lib.epi_p_adjust_dev(fake, None, 0, method, 0, None, None, None, C.byref(n)) == _lib.EPI_ERR_ARG and n.value == 0
        assert b"method" in lib.epi_last_error()
    assert lib.epi_p_adjust_dev(fake, None, -1, 4, 0, None, None, None, C.byref(n)) == _lib.EPI_ERR_ARG
    assert lib.epi_p_adjust_dev(fake, None, 2 ** 31, 4, 0, None, None, None, C.byref(n)) == _lib.EPI_ERR_ARG
    assert lib.epi_p_adjust_dev(fake, None, 0, 4, 2 ** 31, None, None, None, C.byref(n)) == _lib.EPI_ERR_ARG
    assert lib.epi_p_adjust_dev(fake, None, 5, 4, 0, None, None, None, C.byref(n)) == _lib.EPI_ERR_ARG
    assert b"NULL column" in lib.epi_last_error()
    n.value = -1
    assert lib.epi_p_adjust_dev(fake, None, 0, 4, 0, None, None, None, C.byref(n)) == _lib.EPI_OK and n.value == 0   # n == 0: nothing to do


def test_fails_loudly_without_gpu():
    if _has_gpu():
        pytest.skip("GPU present")
    t = H.templates_from_xm(["Z.z.Z.z", "z.Z.z.Z"], [1, 1], [1, 1])
    a, b = [ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"]) for _ in range(2)]
    for call in (lambda: ea.adjustPValues([0.01, 0.02]), lambda: ea.adjustPValues([], method="holm"), lambda: ea.adjustReport(_report()),
                 lambda: ea.generateAdjustedDmrReport(a, b, threshold_reads=False)):
        with pytest.raises(ea.EpihipError) as ei:
            call()
        assert ei.value.code == 5 and "no CPU fallback" in str(ei.value)


# ---- the restatement -------------------------------------------------------------------------------------------------------

def test_known_answers():
    p = [.01, .02, .03, .04, .05]
    np.testing.assert_allclose(P.adjust_np(p, "BH")[0], [.05] * 5, rtol=1e-15)
    np.testing.assert_allclose(P.adjust_np(p, "holm")[0], [.05, .08, .09, .09, .09], rtol=1e-15)
    np.testing.assert_allclose(P.adjust_np(p, "hochberg")[0], [.05] * 5, rtol=1e-15)
    np.testing.assert_allclose(P.adjust_np(p, "bonferroni")[0], [.05, .1, .15, .2, .25], rtol=1e-15)
    np.testing.assert_allclose(P.adjust_np(p, "BY")[0], [.05 * (1 + 1 / 2 + 1 / 3 + 1 / 4 + 1 / 5)] * 5, rtol=1e-15)
    assert np.array_equal(P.adjust_np(p, "none")[0], p)
    assert np.all(P.adjust_np([0.5, 0.9, 1.0], "bonferroni")[0] == 1.0)
    # R: p.adjust(c(.01, .02, .03), "BH", n = 10)
    np.testing.assert_allclose(P.adjust_np([.03, .01, .02], "BH", n_tests=10)[0], [.1, .1, .1], rtol=1e-15)
    np.testing.assert_allclose(P.adjust_np([.03, .01, .02], "holm", n_tests=10)[0], [.24, .1, .18], rtol=1e-15)


def test_na_zero_order_and_refusals():
    p = np.asarray([0.5, np.nan, -0.0, 0.5, 0.0, 1.0, np.nan, 0.25])
    q, order, m = P.adjust_np(p, "BH")
    assert m == 6 and order.tolist() == [2, 4, 7, 0, 3, 5, 1, 6]              # stable among the ties, -0.0 as 0.0, NaN last
    assert np.isnan(q[[1, 6]]).all() and q[2] == 0.0 and q[4] == 0.0 and not np.signbit(q[2])
    assert q[0] == q[3] == 0.6 and q[5] == 1.0 and q[7] == 0.5
    q, order, m = P.adjust_np([np.nan, np.nan], "holm")
    assert m == 0 and np.isnan(q).all() and order.tolist() == [0, 1]
    q, order, m = P.adjust_np([], "BY")
    assert m == 0 and q.size == 0 and order.size == 0
    for bad in ([0.1, 1.5], [-1e-9], [np.inf, 0.2], [0.3, -np.inf]):
        with pytest.raises(ValueError):
            P.adjust_np(bad, "BH")
    with pytest.raises(ValueError):
        P.adjust_np([0.1, 0.2, np.nan, 0.3], "BH", n_tests=2)
    assert P.adjust_np([0.1, 0.2, np.nan, 0.3], "BH", n_tests=3)[2] == 3
    assert P.harmonic(4) == ((1.0 + 0.5) + 1.0 / 3) + 0.25 and P.harmonic(0) == 0.0


@pytest.mark.parametrize("method", P.METHODS)
def test_invariant_under_permutation_bit_for_bit(method):
    rng = np.random.default_rng(7)
    for p in (rng.random(2000), np.round(rng.random(2000), 2), rng.random(2000) ** 8, np.where(rng.random(2000) < 0.1, np.nan, rng.random(2000))):
        q = P.adjust_np(p, method)[0]
        perm = rng.permutation(p.size)
        assert np.array_equal(bits(P.adjust_np(p[perm], method)[0]), bits(q[perm]))
        ok = ~np.isnan(p)
        assert np.array_equal(np.isnan(q), ~ok) and np.all((q[ok] >= p[ok]) & (q[ok] <= 1.0))
        o = np.argsort(p[ok], kind="stable")
        assert np.all(np.diff(q[ok][o]) >= 0)                                  # monotone in p


def test_agrees_with_brute_force_definitions():
    rng = np.random.default_rng(8)
    for p in (rng.random(300), np.round(rng.random(300), 2), rng.random(300) ** 8):
        for method in ("BH", "holm"):
            np.testing.assert_allclose(P.adjust_np(p, method)[0], P.brute_np(p, method), rtol=1e-13, atol=0)


def test_digit_passes():
    assert P.digit_passes(np.full(10, 0.25)) == 0 and P.digit_passes([np.nan, np.nan]) == 0 and P.digit_passes([]) == 0
    assert P.digit_passes([0.25, 0.5]) == 1 and P.digit_passes([0.25, 2.0 ** -300]) == 2 and P.digit_passes([0.25, np.nan]) == 8
    assert P.digit_passes(np.random.default_rng(1).random(1000)) >= 7
