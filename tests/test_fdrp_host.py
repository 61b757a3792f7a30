"""generateFdrpReport on the host side: the exported symbols, the functions' signatures, argument checks before any I/O,
the pair list's limit as a function of its own, the loud failure without a device (the pairs are compared on the GPU; there
is no CPU path), and the restatement of the definitions (tests/fdrp_np.py) against the closed form that FDRP has without
flanking sites."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import fdrp_np
import helpers as H
import epialleler_amd as ea
from epialleler_amd import _lib

NEW_SYMBOLS = ("epi_batch_fdrp_report_dev", "epi_batch_fdrp_fetch_dev", "epi_fdrp_pair_bytes")
EMPTY = inspect.Parameter.empty


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_symbols_declared_exported_and_listed():
    _lib.build()
    with open(os.path.join(H.GOLDEN, "..", "..", "include", "epihip.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(_lib.load(), name)
        assert re.search(r"\bint %s\(" % name, hdr)
    assert ea.FDRP_COLUMNS == ("rname", "strand", "pos", "context", "coverage", "nreads", "npairs", "ndiscordant", "fdrp", "qfdrp")


def test_signatures_and_defaults():
    p = inspect.signature(ea.generateFdrpReport).parameters
    assert [(k, v.default) for k, v in p.items() if v.kind is not v.VAR_KEYWORD] == [
        ("bam", EMPTY), ("report_file", None), ("fdrp_context", None), ("flank_sites", 8), ("max_reads", 40), ("min_overlap", 1),
        ("max_distance", 0), ("min_reads", 2), ("max_outofcontext_beta", 0.1), ("gzip", False), ("verbose", False), ("as_device", False)]
    assert [k for k, v in p.items() if v.kind is v.VAR_KEYWORD] == ["preprocess_args"]
    q = inspect.signature(ea.rcpp_fdrp_report).parameters
    assert [(k, v.default) for k, v in q.items()] == [
        ("df", EMPTY), ("ctx", EMPTY), ("flank_sites", EMPTY), ("max_reads", EMPTY), ("min_overlap", EMPTY), ("max_distance", EMPTY),
        ("max_ooctx_meth_frac", EMPTY), ("min_reads", 2), ("as_device", False)]


BAD = [dict(flank_sites=-1), dict(flank_sites=32), dict(flank_sites=2.5), dict(max_reads=1), dict(max_reads=65),
       dict(min_overlap=0), dict(min_overlap=18), dict(flank_sites=0, min_overlap=2), dict(flank_sites=31, min_overlap=64),
       dict(max_distance=-1), dict(fdrp_context="CpG"), dict(fdrp_context="cg")]
R_NAME = {"flank_sites": "flank.sites", "max_reads": "max.reads", "min_overlap": "min.overlap", "max_distance": "max.distance"}


@pytest.mark.parametrize("kw", BAD)
def test_bad_arguments_raise_before_io(kw):
    with pytest.raises(ValueError) as ei:
        ea.generateFdrpReport("no-such-file.bam", **kw)      # (opening it would raise "Unable to open BAM file")
    msg = str(ei.value)
    name = list(kw)[-1]                                      # (min_overlap 2W + 2: the last key is the one that is wrong)
    if name == "fdrp_context":
        assert "'fdrp.context' should be one of 'CG', 'CHG', 'CHH', 'CxG', 'CX'" in msg
    else:
        assert "'%s' should be" % R_NAME[name] in msg
    assert "no-such-file" not in msg and "open" not in msg


def test_good_arguments_reach_the_file():
    for kw in (dict(flank_sites=0), dict(flank_sites=31, min_overlap=63), dict(max_reads=2), dict(max_reads=64, fdrp_context="CX"),
               dict(min_overlap=17), dict(max_distance=0), dict(max_distance=500)):
        with pytest.raises(Exception) as ei:
            ea.generateFdrpReport("no-such-file.bam", **kw)
        assert not isinstance(ei.value, ValueError) or "should be" not in str(ei.value)


def test_pair_bytes():
    """24 bytes per call for the two (key, row) buffers; 2^32 calls or more do not fit the sort's 32-bit indices."""
    lib = _lib.load()
    out = C.c_int64(-1)
    for ncalls in (0, 1, 2 ** 32 - 1):
        assert lib.epi_fdrp_pair_bytes(ncalls, C.byref(out)) == _lib.EPI_OK and out.value == 24 * ncalls
    for ncalls in (2 ** 32, 2 ** 40, -1):
        assert lib.epi_fdrp_pair_bytes(ncalls, C.byref(out)) == _lib.EPI_ERR_ARG and out.value == 0, ncalls
    assert b"calls" in lib.epi_last_error()
    assert lib.epi_fdrp_pair_bytes(1, None) == _lib.EPI_ERR_ARG


def test_fails_loudly_without_gpu():
    if _has_gpu():
        pytest.skip("GPU present")
    t = H.templates_from_xm(["Z.z.Z.z", "z.Z.z.Z"], [1, 1], [1, 1])
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"])
    for call in (lambda: ea.generateFdrpReport(bam, flank_sites=2), lambda: ea.rcpp_fdrp_report(bam, "Zz", 2, 40, 1, 0, 0.1)):
        with pytest.raises(ea.EpihipError) as ei:
            call()
        assert ei.value.code == 5 and "no CPU fallback" in str(ei.value)


def closed_form_templates(seed=5, nrow=60, length=40):
    """Reads of Z, z and '.' only (no out-of-context call: the read rule keeps every row, so the cytosine report's counts
    are the coverage), both strands, ragged starts."""
    rng = np.random.default_rng(seed)
    xms, starts, strands = [], [], []
    for _ in range(nrow):
        L = int(rng.integers(5, length))
        st = int(rng.integers(1, 30))
        # CpG positions are the even ones: a position has one context whatever read covers it
        xms.append("".join(("Z" if rng.random() < 0.5 else "z") if (st + j) % 2 == 0 and rng.random() < 0.8 else "." for j in range(L)))
        starts.append(st)
        strands.append(int(rng.integers(1, 3)))
    return H.templates_from_xm(xms, starts, strands)


def test_restatement_matches_closed_form_without_flanks():
    """flank_sites = 0: a pair is discordant when its two calls at the site differ, so npairs = c (c - 1) / 2,
    ndiscordant = meth * unmeth of the cytosine report's row, and qfdrp == fdrp (o = 1 for every pair)."""
    t = closed_form_templates()
    m = 64
    rep = fdrp_np.restate(t, "CG", flank_sites=0, max_reads=m, min_overlap=1, min_reads=2)
    s = rep["sites"]
    cov = (s["meth"] + s["unmeth"]).astype(np.int64)
    assert cov.max() <= m and (cov >= 2).sum() > 10 and len(set(s["strand"].tolist())) == 2
    want = cov >= 2
    for q in ("rname", "strand", "pos", "context"):
        assert np.array_equal(rep[q], s[q][want])
    c = cov[want]
    assert np.array_equal(rep["coverage"], c) and np.array_equal(rep["nreads"], c)
    assert np.array_equal(rep["npairs"], c * (c - 1) // 2)
    assert np.array_equal(rep["ndiscordant"], s["meth"][want].astype(np.int64) * s["unmeth"][want])
    assert rep["ndiscordant"].max() > 0
    assert np.array_equal(rep["qfdrp"], rep["fdrp"])
    assert np.array_equal(rep["fdrp"], rep["ndiscordant"].astype(np.float64) / rep["npairs"].astype(np.float64))


def test_selection_ranks():
    """floor(j c / m): all rows when c <= m, otherwise m distinct ranks spread from the first row on."""
    assert fdrp_np.selected_ranks(5, 7) == [0, 1, 2, 3, 4] and fdrp_np.selected_ranks(7, 7) == list(range(7))
    assert fdrp_np.selected_ranks(8, 7) == [0, 1, 2, 3, 4, 5, 6]
    assert fdrp_np.selected_ranks(100, 7) == [0, 14, 28, 42, 57, 71, 85]
    r = fdrp_np.selected_ranks(65, 64)
    assert r[0] == 0 and r[-1] == 63 and len(set(r)) == 64
    r = fdrp_np.selected_ranks(100, 40)
    assert r == [(5 * j) // 2 for j in range(40)] and len(set(r)) == 40
