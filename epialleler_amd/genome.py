"""preprocessGenome and callMethylation: methylation calls (XG / XM tags) from the reference genome for BAM files that
carry only a strand tag -- bwa-meth (YD), BSMAP (ZS), or DRAGEN / Bismark written without calls (XG).
Mirrors R/preprocessGenome.R, R/callMethylation.R, .readGenome (R/internal.R:135-150) and .callMethylation
(R/internal.R:405-432), with the Rcpp exports rcpp_read_genome (src/rcpp_read_genome.cpp) and
rcpp_call_methylation_genome (src/rcpp_call_methylation.cpp).  The FASTA file is read by the library (epi_read_genome,
host), the calls are made on the GPU (epi_call_methylation: k_call_refspace / k_call_xm) and the output BAM is written by
the library's BGZF writer.
"""
import ctypes as C
import os
import sys
import time

import numpy as np

from . import _lib


class Genome:
    """What preprocessGenome returns: rid (0-based), rname and rlen of every sequence, in file order, and the sequences
    themselves inside the library (the reference keeps them behind the list's `rseq_xptr`).  The sequences are uploaded
    to a device by the first callMethylation there and stay resident while the object lives."""

    def __init__(self, handle):
        self._h = C.c_void_p(handle)
        lib = _lib.load()
        n = lib.epi_genome_count(self._h)
        self.rid = np.arange(n, dtype=np.int64)
        self.rname = [lib.epi_genome_name(self._h, i).decode("latin1") for i in range(n)]
        self.rlen = np.array([lib.epi_genome_length(self._h, i) for i in range(n)], dtype=np.int64)

    def __len__(self):
        return len(self.rname)

    def sequence(self, i):
        """Sequence i as bytes (upper-case A, C, G, T and N only)."""
        n = int(self.rlen[i])
        return C.string_at(_lib.load().epi_genome_sequence(self._h, int(i)), n) if n else b""

    def __repr__(self):
        return "Genome(%d sequences, %d bp)" % (len(self), int(self.rlen.sum()))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and _lib._lib is not None:
            _lib._lib.epi_genome_free(h)
            self._h = None


def _message(verbose, fmt, *args):
    if verbose:
        sys.stderr.write(fmt % args)
        sys.stderr.flush()


def rcpp_read_genome(fn, nthreads):
    """rcpp_read_genome(fn, nthreads): the FASTA file (plain, gzip or BGZF; no index needed) -> Genome."""
    lib = _lib.load()
    h = C.c_void_p()
    rc = lib.epi_read_genome(os.path.expanduser(str(fn)).encode(), int(max(nthreads, 1)), C.byref(h))
    if rc != _lib.EPI_OK:
        raise ValueError(lib.epi_last_error().decode("utf-8", "replace"))
    return Genome(h.value)


def preprocessGenome(genome_file, nthreads=1, verbose=True):
    """R/preprocessGenome.R: a path is read (.readGenome); anything else -- an already preprocessed Genome -- is
    returned unchanged."""
    if isinstance(genome_file, Genome):
        return genome_file
    _message(verbose, "Reading reference genome file ")
    t0 = time.time()
    g = rcpp_read_genome(genome_file, nthreads)
    _message(verbose, "[%.3fs]\n", time.time() - t0)
    return g


def rcpp_call_methylation_genome(in_fn, out_fn, genome, tag, nthreads, window_kib=0):
    """rcpp_call_methylation_genome(in_fn, out_fn, genome, tag, nthreads): calls with the given strand tag ("XG", "YD"
    or "ZS"; None chooses it as .callMethylation does).  Returns {"nrecs", "ncalled"}."""
    lib = _lib.load()
    eng = C.c_void_p()
    _lib.check(lib.epi_default_engine(C.byref(eng)))              # no device: EpihipError, there is no CPU path
    nrecs, ncalled = C.c_int64(0), C.c_int64(0)
    rc = lib.epi_call_methylation_windowed(eng, os.path.expanduser(str(in_fn)).encode(),
                                           os.path.expanduser(str(out_fn)).encode() if out_fn else b"", genome._h,
                                           tag.encode() if tag else None, int(max(nthreads, 1)), int(window_kib),
                                           C.byref(nrecs), C.byref(ncalled))
    if rc == _lib.EPI_ERR_ARG:
        raise ValueError(lib.epi_last_error().decode("utf-8", "replace"))    # stop(..., call.=FALSE) in the reference
    _lib.check(rc)
    return {"nrecs": int(nrecs.value), "ncalled": int(ncalled.value)}


def callMethylation(input_bam_file, output_bam_file, genome, nthreads=1, verbose=True, window_kib=0):
    """R/callMethylation.R: `genome` is a FASTA path or a Genome from preprocessGenome.  Records that are mapped, carry
    the strand tag (XG, else YD, else ZS, as found in the first 1024 records) and have no XM are written with XG (when
    absent) and XM appended; every other record is written unchanged.  Returns {"nrecs", "ncalled"}.
    window_kib: inflated bytes per processing window (0: the library's default); results do not depend on it."""
    genome = preprocessGenome(genome, nthreads=nthreads, verbose=verbose)
    _message(verbose, "Making methylation calls ")
    t0 = time.time()
    res = rcpp_call_methylation_genome(input_bam_file, output_bam_file, genome, None, nthreads, window_kib)
    _message(verbose, "[%.3fs]\n", time.time() - t0)
    return res
