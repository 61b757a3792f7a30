"""preprocessBam(mates=...) on the host side: argument checks before any I/O, the exported entry point, and the loud
failure without a device (the templates are merged on the GPU; there is no CPU path)."""
import inspect
import os

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


def test_signature_default_is_adjacent():
    p = inspect.signature(ea.preprocessBam).parameters
    assert "mates" in p and p["mates"].default is None


@pytest.mark.parametrize("bad", ["any", "Anywhere", "", 1, True])
def test_bad_mates_value_raises_before_io(bad):
    with pytest.raises(ValueError) as ei:
        ea.preprocessBam("no-such-file.bam", mates=bad)       # (the file would give "Unable to open")
    assert "'mates' should be one of 'adjacent', 'anywhere'" in str(ei.value)


def test_mates_anywhere_with_genome_raises():
    with pytest.raises(ValueError) as ei:
        ea.preprocessBam(os.path.join(BAM, "dragen-pe-unsort-xg-xm.bam"), mates="anywhere", genome="no such genome.fa")
    assert "mates" in str(ei.value) and "genome" in str(ei.value)
    # (through **preprocess_args too)
    with pytest.raises(ValueError):
        ea.generateCytosineReport(os.path.join(BAM, "dragen-pe-unsort-xg-xm.bam"), mates="nowhere")


def test_adjacent_is_the_default_behaviour():
    with pytest.raises(ValueError) as ei:
        ea.preprocessBam(os.path.join(BAM, "dragen-pe-unsort-xg-xm.bam"), mates="adjacent")
    assert "not sorted by name" in str(ei.value)
    a = ea.preprocessBam(os.path.join(BAM, "dragen-pe-namesort-xg-xm.bam"), mates="adjacent")
    b = ea.preprocessBam(os.path.join(BAM, "dragen-pe-namesort-xg-xm.bam"))
    assert (a.n, a.nbytes, a.nrecs) == (b.n, b.nbytes, b.nrecs)


def test_symbol_exported():
    assert "epi_preprocess_bam_anyorder" in _lib.EXPORTED_SYMBOLS
    assert hasattr(_lib.load(), "epi_preprocess_bam_anyorder")
    with open(os.path.join(H.GOLDEN, "..", "..", "include", "epihip.h")) as f:
        assert "int epi_preprocess_bam_anyorder(" in f.read()


def test_anywhere_fails_loudly_without_gpu():
    if _has_gpu():
        pytest.skip("GPU present")
    with pytest.raises(ea.EpihipError) as ei:
        ea.preprocessBam(os.path.join(BAM, "dragen-pe-unsort-xg-xm.bam"), mates="anywhere")
    assert ei.value.code == _lib.EPI_ERR_NODEVICE
    # the device is looked for before the file is opened
    with pytest.raises(ea.EpihipError):
        ea.preprocessBam("no-such-file.bam", mates="anywhere")
