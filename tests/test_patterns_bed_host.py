"""extractPatternsBed on the host side: the exported names, argument checks before any I/O, and the loud failure without
a device (the patterns are extracted on the GPU; there is no CPU path)."""
import inspect
import os

import numpy as np
import pytest

import helpers as H
import epialleler_amd as ea
from epialleler_amd import _lib

BAM = os.path.join(H.GOLDEN, "bam")


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_symbols_exported():
    for name in ("epi_batch_extract_patterns_multi", "epi_batch_extract_patterns_multi_stats"):
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(_lib.load(), name)
        with open(os.path.join(H.GOLDEN, "..", "..", "include", "epihip.h")) as f:
            assert "int %s(" % name in f.read()


def test_function_exported_and_bed_rows_defaults_to_none():
    p = inspect.signature(ea.extractPatternsBed).parameters
    assert "bed_rows" in p and p["bed_rows"].default is None
    single = inspect.signature(ea.extractPatterns).parameters
    assert [k for k in p if k != "bed_rows"] == [k for k in single if k != "bed_row"]
    assert all(p[k].default == single[k].default for k in p if k != "bed_rows")
    assert callable(ea.rcpp_extract_patterns_multi)


@pytest.mark.parametrize("bad", ["cg", "CpG", "", 1])
def test_bad_context_raises_before_io(bad):
    with pytest.raises(ValueError) as ei:
        ea.extractPatternsBed("no-such-file.bam", "no-such-file.bed", extract_context=bad)
    assert "'extract.context' should be one of 'CG', 'CHG', 'CHH', 'CxG', 'CX'" in str(ei.value)


@pytest.mark.parametrize("bad", ["1", [1, "2"], 1.5, [1, 2.0], [None], True, [1, np.float64(3)]])
def test_bad_bed_rows_raise_before_io(bad):
    with pytest.raises(ValueError) as ei:
        ea.extractPatternsBed("no-such-file.bam", "no-such-file.bed", bed_rows=bad)
    assert "bed.rows" in str(ei.value)


def test_integer_bed_rows_pass_validation():
    # (numpy integers and plain ints are row numbers; the missing files are what fails then)
    for rows in ([1, 2], np.arange(1, 3), np.int32(1), (), [0, -5, 10 ** 6]):
        with pytest.raises(Exception) as ei:
            ea.extractPatternsBed("no-such-file.bam", "no-such-file.bed", bed_rows=rows)
        assert "bed.rows" not in str(ei.value)


def test_fails_loudly_without_gpu():
    if _has_gpu():
        pytest.skip("GPU present")
    with pytest.raises(ea.EpihipError) as ei:
        ea.extractPatternsBed(os.path.join(BAM, "capture.bam"), os.path.join(BAM, "capture.bed"))
    assert ei.value.code == _lib.EPI_ERR_NODEVICE
    t = H.templates_from_xm(["Zz"], [1], [1])
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"])
    with pytest.raises(ea.EpihipError) as ei:
        ea.rcpp_extract_patterns_multi(bam, [(1, 1, 2)], 1, "Zz", 0.01, False, 0)
    assert ei.value.code == _lib.EPI_ERR_NODEVICE
