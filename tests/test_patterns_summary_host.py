"""summarisePatterns / selectPatterns on the host side: the exported symbols, selectPatterns (host Python only) on
hand-made summaries, argument checks before any I/O, and the loud failure without a device (the patterns are grouped on
the GPU; there is no CPU path)."""
import inspect
import os

import numpy as np
import pytest

import helpers as H
import epialleler_amd as ea
from epialleler_amd import _lib

BAM = os.path.join(H.GOLDEN, "bam")
NEW_SYMBOLS = ("epi_pattern_summary_free", "epi_batch_summarise_patterns_multi", "epi_batch_summarise_patterns_stats")


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_symbols_exported():
    with open(os.path.join(H.GOLDEN, "..", "..", "include", "epihip.h")) as f:
        hdr = f.read()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(_lib.load(), name)
        assert " %s(" % name in hdr
    assert "} epi_pattern_summary;" in hdr
    assert [f[0] for f in _lib.PatternSummary._fields_] == ["nuniq", "npat", "ncol", "positions", "fnv", "count", "cells"]


def test_functions_exported_with_the_bed_call_s_arguments():
    p = inspect.signature(ea.summarisePatterns).parameters
    many = inspect.signature(ea.extractPatternsBed).parameters
    assert [k for k in p if k != "bin_context"] == list(many)
    assert all(p[k].default == many[k].default for k in many) and p["bin_context"].default is None
    q = inspect.signature(ea.selectPatterns).parameters
    assert [(k, v.default) for k, v in q.items()][1:] == [("order_by", "beta"), ("beta_range", (0, 1)), ("nbins", 10),
                                                          ("npatterns_per_bin", 2)]
    assert callable(ea.rcpp_summarise_patterns_multi)


# ---- selectPatterns ------------------------------------------------------------------------------------------------------

BETA = [0.0, 0.05, 0.1, 0.5, 1.0, 0.55, 0.52, 0.95]      # bins of ten over [0, 1]: 1, 1, 2 (an edge), 6 (an edge), 10 (the end), 6, 6, 10
COUNT = [5, 9, 5, 7, 5, 7, 1, 2]


def summary(beta=BETA, count=COUNT):
    n = len(beta)
    rep = ea.Report({"pattern": np.asarray(["%016X" % i for i in range(n)], object), "100": np.arange(n, dtype=np.int32) + 1,
                     "count": np.asarray(count, np.int32), "beta": np.asarray(beta, np.float64)}, ("chrA",))
    rep.bed = "chrA:1-200"
    rep.pattern_levels = ("a", "b")
    return rep


def rows_of(sel):
    return [int(p, 16) for p in sel["pattern"]]


def test_select_default_two_per_bin():
    sel = ea.selectPatterns(summary())
    # by count, descending and stable: rows 1, 3, 5, 0, 2, 4, 7, 6 -> bins 1, 6, 6, 1, 2, 10, 10, 6; two per bin, the bins
    # in that order of appearance
    assert rows_of(sel) == [1, 0, 3, 5, 2, 4, 7]
    assert list(sel.keys()) == ["pattern", "100", "count", "beta", "bin", "I"]
    assert sel["bin"].tolist() == [1, 1, 6, 6, 2, 10, 10]
    assert sel["100"].tolist() == [2, 1, 4, 6, 3, 5, 8] and sel["count"].tolist() == [9, 5, 7, 7, 5, 5, 2]
    assert sel["I"].tolist() == [1, 0, 3, 4, 2, 6, 5]             # 7 - rank by decreasing beta
    assert np.array_equal(sel.bins, np.linspace(0, 1, 11)) and sel.bed == "chrA:1-200" and sel.pattern_levels == ("a", "b")


def test_select_count_ties_keep_table_order():
    sel = ea.selectPatterns(summary(), npatterns_per_bin=1)
    assert rows_of(sel) == [1, 3, 2, 4]                            # bin 6: row 3 before row 5 (both 7); bin 10: row 4 before 7
    same = ea.selectPatterns(summary([0.3, 0.3, 0.3], [2, 2, 2]))
    assert rows_of(same) == [0, 1] and same["I"].tolist() == [1, 0]            # equal keys: rank in table order


def test_select_order_by_count():
    sel = ea.selectPatterns(summary(), order_by="count")
    assert rows_of(sel) == [1, 0, 3, 5, 2, 4, 7]
    assert sel["I"].tolist() == [6, 1, 4, 5, 2, 3, 0]             # decreasing (count, beta): 1 | 5, 3 | 4, 2, 0 | 7


def test_select_beta_range_edges_and_outside():
    sel = ea.selectPatterns(summary(), beta_range=(0.1, 0.5), nbins=2)
    assert rows_of(sel) == [3, 2]                                  # 0.1 and 0.5 are inside the closed range, all others outside
    assert sel["bin"].tolist() == [2, 1] and sel["I"].tolist() == [1, 0]
    assert np.array_equal(sel.bins, np.linspace(0.1, 0.5, 3))
    one = ea.selectPatterns(summary(), beta_range=(0.5, 0.5), nbins=1)
    assert rows_of(one) == [3] and one["bin"].tolist() == [1]
    none = ea.selectPatterns(summary(), beta_range=(0.2, 0.3))
    assert rows_of(none) == [] and none["I"].size == 0 and list(none.keys()) == ["pattern", "100", "count", "beta", "bin", "I"]


def test_select_npatterns_per_bin_forms():
    assert rows_of(ea.selectPatterns(summary(), npatterns_per_bin=[1, 3])) == [1, 3, 5, 6, 2, 4, 7]      # 1, 3, 1, 3, ...: bins 2, 6, 10 take 3
    assert rows_of(ea.selectPatterns(summary(), npatterns_per_bin=float("inf"))) == [1, 0, 3, 5, 6, 2, 4, 7]
    assert rows_of(ea.selectPatterns(summary(), npatterns_per_bin=0)) == []
    assert rows_of(ea.selectPatterns(summary(), nbins=1, npatterns_per_bin=3)) == [1, 3, 5]


def test_select_empty_summary():
    sel = ea.selectPatterns(ea.Report({}, ("chrA",)))
    assert not sel and sel.nrow == 0 and sel.bins.size == 11


@pytest.mark.parametrize("kw", [dict(order_by="pattern"), dict(order_by=None), dict(nbins=0), dict(nbins=-3), dict(beta_range=(1, 0)),
                                dict(beta_range=(0.5, 0.4999))])
def test_select_bad_arguments(kw):
    with pytest.raises(ValueError):
        ea.selectPatterns(summary(), **kw)


# ---- summarisePatterns' arguments ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [dict(extract_context="cg"), dict(bin_context="CpG"), dict(bin_context=1)])
def test_bad_context_raises_before_io(kw):
    with pytest.raises(ValueError) as ei:
        ea.summarisePatterns("no-such-file.bam", "no-such-file.bed", **kw)
    assert "should be one of 'CG', 'CHG', 'CHH', 'CxG', 'CX'" in str(ei.value)


@pytest.mark.parametrize("bad", ["1", [1, "2"], 1.5, [1, 2.0], [None], True])
def test_bad_bed_rows_raise_before_io(bad):
    with pytest.raises(ValueError) as ei:
        ea.summarisePatterns("no-such-file.bam", "no-such-file.bed", bed_rows=bad)
    assert "bed.rows" in str(ei.value)


def test_fails_loudly_without_gpu():
    if _has_gpu():
        pytest.skip("GPU present")
    with pytest.raises(ea.EpihipError) as ei:
        ea.summarisePatterns(os.path.join(BAM, "capture.bam"), os.path.join(BAM, "capture.bed"))
    assert ei.value.code == _lib.EPI_ERR_NODEVICE
    t = H.templates_from_xm(["Zz"], [1], [1])
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"])
    with pytest.raises(ea.EpihipError) as ei:
        ea.rcpp_summarise_patterns_multi(bam, [(1, 1, 2)], 1, "Zz", 0.01, False, 0)
    assert ei.value.code == _lib.EPI_ERR_NODEVICE
