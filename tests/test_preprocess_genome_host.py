"""preprocessBam(genome=) without a GPU: the entry point is exported, the Python signature takes the genome, and a
machine without a device gets an error -- the genome is never silently ignored (there is no CPU path)."""
import inspect
import os

import numpy as np
import pytest

import epialleler_amd as ea
from epialleler_amd import _lib
from helpers import GOLDEN

BAMS = os.path.join(GOLDEN, "bam")
FASTA = os.path.join(BAMS, "reference.fasta.gz")


def _have_device():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_symbol_exported():
    assert "epi_preprocess_bam_genome" in _lib.EXPORTED_SYMBOLS
    assert hasattr(_lib.load(), "epi_preprocess_bam_genome")
    with open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "epihip.h")) as f:
        assert "int epi_preprocess_bam_genome(" in f.read()


def test_signature_accepts_genome():
    p = inspect.signature(ea.preprocessBam).parameters
    assert "genome" in p and p["genome"].default is None


def test_preprocessed_input_ignores_genome():
    bam = {"xm": np.full(4, 0xFB, np.uint8), "off": np.array([0, 4], np.int64), "rname": np.array([1], np.int32),
           "strand": np.array([1], np.int32), "start": np.array([1], np.int32)}
    p = ea.preprocessBam(bam, genome="no such genome.fa")
    assert p.n == 1 and p.ncalled == 0
    assert ea.preprocessBam(p, genome="no such genome.fa") is p


def test_without_genome_ncalled_is_zero():
    p = ea.preprocessBam(os.path.join(BAMS, "dragen-se-unsort-xg-xm.bam"))
    assert p.n > 0 and p.ncalled == 0


@pytest.mark.skipif(_have_device(), reason="needs a machine without a GPU")
def test_no_device_raises():
    g = ea.preprocessGenome(FASTA, verbose=False)
    src = os.path.join(BAMS, "bwameth-se-unsort-yd.bam")
    with pytest.raises(ea.EpihipError):
        ea.preprocessBam(src, genome=g)
    with pytest.raises(ea.EpihipError):
        ea.preprocessBam(src, genome=FASTA)
    with pytest.raises(ea.EpihipError):
        ea.generateCytosineReport(src, genome=g)
