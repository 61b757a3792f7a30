"""compareHeterogeneity on the host side: the exported symbols, the functions' signatures, argument checks before any I/O,
the sequence-name check before anything touches a device, the counter cap as a function of its own, and the loud failure
without a device (the histograms are counted on the GPU; there is no CPU path)."""
import ctypes as C
import inspect
import os
import re

import pytest

import helpers as H
import epialleler_amd as ea
from epialleler_amd import _lib

NEW_SYMBOLS = ("epi_batch_heterogeneity_compare_dev", "epi_batch_heterogeneity_compare_fetch_dev")
EMPTY = inspect.Parameter.empty


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
    for name in NEW_SYMBOLS + ("epi_heterogeneity_counter_bytes",):
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(_lib.load(), name)
        assert re.search(r"\bint %s\(" % name, hdr)


def test_signatures_and_defaults():
    p = inspect.signature(ea.compareHeterogeneity).parameters
    assert [(k, v.default) for k, v in p.items() if v.kind is not v.VAR_KEYWORD] == [
        ("bam_a", EMPTY), ("bam_b", EMPTY), ("report_file", None), ("window_context", None), ("window_sites", 4), ("min_reads", 1),
        ("max_window_span", 0), ("max_outofcontext_beta", 0.1), ("gzip", False), ("verbose", False), ("as_device", False)]
    assert [k for k, v in p.items() if v.kind is v.VAR_KEYWORD] == ["preprocess_args"]
    q = inspect.signature(ea.rcpp_heterogeneity_compare).parameters
    assert [(k, v.default) for k, v in q.items()] == [
        ("df_a", EMPTY), ("df_b", EMPTY), ("ctx", EMPTY), ("k", EMPTY), ("max_ooctx_meth_frac", EMPTY), ("min_reads", 1),
        ("max_window_span", 0), ("as_device", False), ("with_counts", False)]


@pytest.mark.parametrize("kw", [dict(window_sites=1), dict(window_sites=7), dict(window_sites=2.5), dict(window_sites=True),
                                dict(window_context="CpG"), dict(window_context="cg")])
def test_bad_arguments_raise_before_io(kw):
    with pytest.raises(ValueError) as ei:
        ea.compareHeterogeneity("no-such-file.bam", "no-such-file-either.bam", **kw)    # (opening one would raise "Unable to open BAM file")
    msg = str(ei.value)
    (name,) = kw
    if name == "window_context":
        assert "'window.context' should be one of 'CG', 'CHG', 'CHH', 'CxG', 'CX'" in msg
    else:
        assert "'window.sites' should be an integer from 2 to 6" in msg
    assert "no-such-file" not in msg and "open" not in msg


def test_good_arguments_reach_the_file():
    for kw in (dict(window_sites=2), dict(window_sites=6, window_context="CX")):
        with pytest.raises(Exception) as ei:
            ea.compareHeterogeneity("no-such-file.bam", "no-such-file-either.bam", **kw)
        assert not isinstance(ei.value, ValueError) or "should be" not in str(ei.value)


def test_differing_levels_raise_before_the_device():
    """rname codes are comparable under one sequence dictionary only; the check needs no device (without one the call
    would raise EpihipError, with one it would upload)."""
    a, b = _two_rows(["chr1", "chr2"]), _two_rows(["chr2", "chr1"])
    for call in (lambda: ea.compareHeterogeneity(a, b), lambda: ea.rcpp_heterogeneity_compare(a, b, "Zz", 2, 0.1),
                 lambda: ea.compareHeterogeneity(a, _two_rows(None)), lambda: ea.compareHeterogeneity(a, _two_rows(["chr1"]))):
        with pytest.raises(ValueError) as ei:
            call()
        assert "levels" in str(ei.value)
    assert a._batch is None and b._batch is None           # nothing was uploaded


def test_counter_cap():
    """ncommon * 2^k * 4 bytes of counters per side, refused above 4 GiB: the check a comparison makes before it allocates
    either array."""
    lib = _lib.load()
    out = C.c_int64(-1)
    cap = 4 << 30
    for nsites, k in ((0, 2), (128, 4), (cap // 16, 2), (cap // 256, 6), (cap // 64, 4)):
        assert lib.epi_heterogeneity_counter_bytes(nsites, k, C.byref(out)) == _lib.EPI_OK and out.value == (nsites << k) * 4
    for nsites, k in ((cap // 16 + 1, 2), (cap // 256 + 1, 6), (cap // 64 + 1, 4), (2 ** 31, 2), (2 ** 40, 6), (-1, 4), (100, 1), (100, 7)):
        assert lib.epi_heterogeneity_counter_bytes(nsites, k, C.byref(out)) == _lib.EPI_ERR_ARG and out.value == 0, (nsites, k)
    assert b"counters" in lib.epi_last_error() or b"k = " in lib.epi_last_error()


def test_null_arguments():
    lib = _lib.load()
    n = C.c_int64(0)
    assert lib.epi_batch_heterogeneity_compare_dev(None, None, b"Zz", 4, 0.1, 1, 0, None, C.byref(n), C.byref(n)) == _lib.EPI_ERR_ARG
    assert lib.epi_batch_heterogeneity_compare_fetch_dev(None, None, None, None, None, None) == _lib.EPI_ERR_ARG


def test_fails_loudly_without_gpu():
    if _has_gpu():
        pytest.skip("GPU present")
    a, b = _two_rows(), _two_rows()
    for call in (lambda: ea.compareHeterogeneity(a, b, window_sites=2), lambda: ea.rcpp_heterogeneity_compare(a, b, "Zz", 2, 0.1)):
        with pytest.raises(ea.EpihipError) as ei:
            call()
        assert ei.value.code == 5 and "no CPU fallback" in str(ei.value)
