"""generateLinkageReport and generateHaplotypeBlocks on the host side: the exported symbols, the functions' signatures,
argument checks before any I/O, the counter cap as a function of its own, and the loud failure without a device (the pairs
are counted on the GPU; there is no CPU path)."""
import ctypes as C
import inspect
import os
import re

import pytest

import helpers as H
import epialleler_amd as ea
from epialleler_amd import _lib

NEW_SYMBOLS = ("epi_batch_linkage_report_dev", "epi_batch_linkage_fetch_dev", "epi_batch_linkage_blocks_dev",
               "epi_batch_linkage_blocks_fetch_dev")
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
    for name in NEW_SYMBOLS + ("epi_linkage_counter_bytes",):
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(_lib.load(), name)
        assert re.search(r"\bint %s\(" % name, hdr)


def test_signatures_and_defaults():
    shared = [("bam", EMPTY), ("report_file", None), ("linkage_context", None), ("max_neighbours", 4), ("max_distance", 0)]
    tail = [("gzip", False), ("verbose", False), ("as_device", False)]
    p = inspect.signature(ea.generateLinkageReport).parameters
    assert [(k, v.default) for k, v in p.items() if v.kind is not v.VAR_KEYWORD] == \
        shared + [("min_reads", 1), ("max_outofcontext_beta", 0.1)] + tail
    assert [k for k, v in p.items() if v.kind is v.VAR_KEYWORD] == ["preprocess_args"]
    p = inspect.signature(ea.generateHaplotypeBlocks).parameters
    assert [(k, v.default) for k, v in p.items() if v.kind is not v.VAR_KEYWORD] == \
        shared + [("min_reads", 10), ("max_outofcontext_beta", 0.1), ("min_r2", 0.5), ("min_sites", 3)] + tail
    assert [k for k, v in p.items() if v.kind is v.VAR_KEYWORD] == ["preprocess_args"]
    q = inspect.signature(ea.rcpp_linkage_report).parameters
    assert [(k, v.default) for k, v in q.items()] == [
        ("df", EMPTY), ("ctx", EMPTY), ("max_neighbours", EMPTY), ("max_distance", EMPTY), ("max_ooctx_meth_frac", EMPTY),
        ("min_reads", 1), ("as_device", False)]
    q = inspect.signature(ea.rcpp_linkage_blocks).parameters
    assert [(k, v.default) for k, v in q.items()] == [
        ("df", EMPTY), ("ctx", EMPTY), ("max_neighbours", EMPTY), ("max_distance", EMPTY), ("max_ooctx_meth_frac", EMPTY),
        ("min_reads", EMPTY), ("min_r2", EMPTY), ("min_sites", EMPTY), ("as_device", False)]


BAD_SHARED = [dict(max_neighbours=0), dict(max_neighbours=17), dict(max_neighbours=2.5), dict(max_neighbours=True),
              dict(max_distance=-1), dict(max_distance=0.5), dict(linkage_context="CpG"), dict(linkage_context="cg")]
BAD_BLOCKS = [dict(min_sites=1), dict(min_sites=2.5), dict(min_r2=-0.1), dict(min_r2=1.5), dict(min_r2=float("nan"))]
R_NAME = {"max_neighbours": "max.neighbours", "max_distance": "max.distance", "min_sites": "min.sites", "min_r2": "min.r2"}


def _raises_before_io(fn, kw):
    with pytest.raises(ValueError) as ei:
        fn("no-such-file.bam", **kw)                     # (opening it would raise "Unable to open BAM file")
    msg = str(ei.value)
    (name,) = kw
    if name == "linkage_context":
        assert "'linkage.context' should be one of 'CG', 'CHG', 'CHH', 'CxG', 'CX'" in msg
    else:
        assert "'%s' should be" % R_NAME[name] in msg
    assert "no-such-file" not in msg and "open" not in msg


@pytest.mark.parametrize("kw", BAD_SHARED)
def test_bad_arguments_raise_before_io(kw):
    _raises_before_io(ea.generateLinkageReport, kw)
    _raises_before_io(ea.generateHaplotypeBlocks, kw)


@pytest.mark.parametrize("kw", BAD_BLOCKS)
def test_bad_block_arguments_raise_before_io(kw):
    _raises_before_io(ea.generateHaplotypeBlocks, kw)


def test_good_arguments_reach_the_file():
    for fn, kw in ((ea.generateLinkageReport, dict(max_neighbours=16, max_distance=0)),
                   (ea.generateLinkageReport, dict(max_neighbours=1, linkage_context="CX")),
                   (ea.generateHaplotypeBlocks, dict(min_sites=2, min_r2=0)), (ea.generateHaplotypeBlocks, dict(min_r2=1))):
        with pytest.raises(Exception) as ei:
            fn("no-such-file.bam", **kw)
        assert not isinstance(ei.value, ValueError) or "should be" not in str(ei.value)


def test_counter_cap():
    """nsites * D * 16 bytes of counters, refused above 4 GiB: the check a report makes before it allocates anything."""
    lib = _lib.load()
    out = C.c_int64(-1)
    cap = 4 << 30
    for nsites, d in ((0, 1), (15408, 16), (cap // 16, 1), (cap // 256, 16), (cap // 64, 4)):
        assert lib.epi_linkage_counter_bytes(nsites, d, C.byref(out)) == _lib.EPI_OK and out.value == nsites * d * 16
    for nsites, d in ((cap // 16 + 1, 1), (cap // 256 + 1, 16), (cap // 64 + 1, 4), (2 ** 31, 1), (2 ** 40, 16), (-1, 4),
                      (100, 0), (100, 17)):
        assert lib.epi_linkage_counter_bytes(nsites, d, C.byref(out)) == _lib.EPI_ERR_ARG and out.value == 0, (nsites, d)
    assert b"counters" in lib.epi_last_error() or b"neighbours" in lib.epi_last_error()


def test_fails_loudly_without_gpu():
    if _has_gpu():
        pytest.skip("GPU present")
    t = H.templates_from_xm(["Z.z.Z.z", "z.Z.z.Z"], [1, 1], [1, 1])
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"])
    for call in (lambda: ea.generateLinkageReport(bam, max_neighbours=2), lambda: ea.generateHaplotypeBlocks(bam, min_reads=1),
                 lambda: ea.rcpp_linkage_report(bam, "Zz", 2, 0, 0.1), lambda: ea.rcpp_linkage_blocks(bam, "Zz", 2, 0, 0.1, 1, 0.5, 2)):
        with pytest.raises(ea.EpihipError) as ei:
            call()
        assert ei.value.code == 5 and "no CPU fallback" in str(ei.value)
