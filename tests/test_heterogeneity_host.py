"""generateHeterogeneityReport on the host side: the two exported symbols, the function's signature, argument checks
before any I/O, and the loud failure without a device (the windows are counted on the GPU; there is no CPU path)."""
import inspect
import os
import re

import pytest

import helpers as H
import epialleler_amd as ea
from epialleler_amd import _lib

NEW_SYMBOLS = ("epi_batch_heterogeneity_report_dev", "epi_batch_heterogeneity_fetch_dev")


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


def test_signature_and_defaults():
    p = inspect.signature(ea.generateHeterogeneityReport).parameters
    assert [(k, v.default) for k, v in p.items() if v.kind is not v.VAR_KEYWORD] == [
        ("bam", inspect.Parameter.empty), ("report_file", None), ("window_context", None), ("window_sites", 4), ("min_reads", 1),
        ("max_window_span", 0), ("max_outofcontext_beta", 0.1), ("gzip", False), ("verbose", False), ("as_device", False)]
    assert [k for k, v in p.items() if v.kind is v.VAR_KEYWORD] == ["preprocess_args"]
    q = inspect.signature(ea.rcpp_heterogeneity_report).parameters
    assert [(k, v.default) for k, v in q.items()] == [
        ("df", inspect.Parameter.empty), ("ctx", inspect.Parameter.empty), ("k", inspect.Parameter.empty),
        ("max_ooctx_meth_frac", inspect.Parameter.empty), ("min_reads", 1), ("max_window_span", 0), ("as_device", False),
        ("with_counts", False)]


@pytest.mark.parametrize("kw", [dict(window_sites=1), dict(window_sites=7), dict(window_sites=2.5), dict(window_context="CpG"),
                                dict(window_context="cg")])
def test_bad_arguments_raise_before_io(kw):
    with pytest.raises(ValueError) as ei:
        ea.generateHeterogeneityReport("no-such-file.bam", **kw)        # (opening it would raise "Unable to open BAM file")
    msg = str(ei.value)
    assert ("window.sites" in msg) if "window_sites" in kw else ("should be one of 'CG', 'CHG', 'CHH', 'CxG', 'CX'" in msg)
    assert "no-such-file" not in msg and "open" not in msg


def test_fails_loudly_without_gpu():
    if _has_gpu():
        pytest.skip("GPU present")
    t = H.templates_from_xm(["Z.z.Z.z", "z.Z.z.Z"], [1, 1], [1, 1])
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"])
    with pytest.raises(ea.EpihipError) as ei:
        ea.generateHeterogeneityReport(bam, window_sites=2)
    assert ei.value.code == 5 and "no CPU fallback" in str(ei.value)
    with pytest.raises(ea.EpihipError) as ei:
        ea.rcpp_heterogeneity_report(bam, "Zz", 2, 0.1)
    assert ei.value.code == 5 and "no CPU fallback" in str(ei.value)
