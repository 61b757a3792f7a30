"""Host-side mirror of the reference's R interface for the hot path.

Same names, argument meaning, defaults and error behaviour as
  R/generateCytosineReport.R:164-208, R/generateMhlReport.R:170-197,
  R/preprocessBam.R:197-237, R/internal.R:54-65 / 439-456 / 486-522
and of the Rcpp exports they call (R/RcppExports.R: rcpp_threshold_reads,
rcpp_get_xm_beta, rcpp_cx_report, rcpp_mhl_report).  All compute goes through
the C ABI of libepihip.so (include/epihip.h); torch is used only for device
memory and streams.  There is no CPU path here.
"""
import ctypes as C
import gzip as _gzip

import numpy as np

from . import _lib

# R/internal.R:54-65 (.context.to.bases), verbatim
CONTEXT_TO_BASES = {
    "CG": dict(ctx_meth="Z", ctx_unmeth="z", ooctx_meth="XH", ooctx_unmeth="xh"),
    "CHG": dict(ctx_meth="X", ctx_unmeth="x", ooctx_meth="ZH", ooctx_unmeth="zh"),
    "CHH": dict(ctx_meth="H", ctx_unmeth="h", ooctx_meth="ZX", ooctx_unmeth="zx"),
    "CxG": dict(ctx_meth="ZX", ctx_unmeth="zx", ooctx_meth="H", ooctx_unmeth="h"),
    "CX": dict(ctx_meth="ZXH", ctx_unmeth="zxh", ooctx_meth="", ooctx_unmeth=""),
}
STRAND_LEVELS = ("+", "-")                                            # src/rcpp_read_bam.cpp:175
CONTEXT_LEVELS = ("NA1", "CHH", "NA3", "NA4", "NA5", "CHG", "CG")     # src/rcpp_cx_report.cpp:150-152
CX_COLUMNS = ("rname", "strand", "pos", "context", "meth", "unmeth")

_engines = {}


def _torch():
    import torch
    return torch


def _engine(device=None):
    """One epi_engine per GPU, created on first use.  Fails loudly without a GPU."""
    lib = _lib.load()
    torch = _torch()
    if device is None:
        device = torch.cuda.current_device() if torch.cuda.is_available() else 0
    if device not in _engines:
        h = C.c_void_p()
        _lib.check(lib.epi_engine_create(int(device), C.byref(h)))
        _engines[device] = h
    return _engines[device]


def _stream(device):
    torch = _torch()
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _engine_of(values):
    """(engine, device index, device string) of a call over `values` (array-likes or tensors): the device of the first CUDA
    tensor among them, else the default engine's."""
    torch = _torch()
    on_dev = [v.device for v in values if isinstance(v, torch.Tensor) and v.is_cuda]
    eng = _engine(on_dev[0].index if on_dev else None)
    index = _lib.load().epi_engine_device(eng)
    return eng, index, "cuda:%d" % index


def _table_cols(nint, ndbl, n, dev):
    """The columns of a table of n rows on `dev`, nint int32 ones and ndbl float64 ones: one allocation per type."""
    torch = _torch()
    return (list(torch.empty((nint, n), dtype=torch.int32, device=dev).unbind(0)),
            list(torch.empty((ndbl, n), dtype=torch.float64, device=dev).unbind(0)))


class Report(dict):
    """A report table: dict of equal-length numpy (or torch) columns plus factor levels,
    the analogue of the data.table the reference returns."""

    def __init__(self, cols, rname_levels=None):
        super().__init__(cols)
        self.levels = {"rname": tuple(rname_levels) if rname_levels is not None else None,
                       "strand": STRAND_LEVELS, "context": CONTEXT_LEVELS}

    @property
    def nrow(self):
        return int(next(iter(self.values())).shape[0]) if self else 0


class ProcessedBam:
    """What preprocessBam() returns in the reference: templates sorted by (rname,start)
    (R/internal.R:193-195) -- here as SoA columns (packed SEQXM bytes + offsets instead of a
    vector of strings behind seqxm_xptr), lazily made resident in HBM."""

    def __init__(self, n, nbytes, levels=None):
        self.n = int(n)
        self.nbytes = int(nbytes)
        self.levels = tuple(levels) if levels is not None else None
        self.host = None        # dict of numpy arrays or None
        self.dev = None         # dict of torch tensors (kept alive for an adopted batch) or None
        self.device = None
        self._batch = None
        self.realign = True     # adopted device columns: let the engine lay the rows out its own way (from_device)
        self._keep = None       # owner of the host buffers the numpy columns are views of (producer output, pinned tensors)
        self.ncalled = 0        # records called on the way in (preprocessBam(genome=))

    @classmethod
    def from_arrays(cls, xm, off, rname, strand, start, levels=None, keepalive=None, device=None):
        off = np.ascontiguousarray(off, dtype=np.int64)
        n = off.size - 1
        if n < 0:
            raise ValueError("off must have n+1 entries")
        xm = np.ascontiguousarray(xm, dtype=np.uint8)
        cols = [np.ascontiguousarray(a, dtype=np.int32) for a in (rname, strand, start)]
        for a in cols:
            if a.size != n:
                raise ValueError("column length does not match off")
        if n and int(off[-1]) != xm.size:
            raise ValueError("off[n] does not match len(xm)")
        self = cls(n, int(off[-1]) if off.size else 0, levels)
        self.host = dict(xm=xm, off=off, rname=cols[0], strand=cols[1], start=cols[2])
        self._keep = keepalive
        self.device = device
        return self

    @classmethod
    def from_pinned(cls, xm, nbytes, off, rname, strand, start, levels=None, device=None):
        """Pinned host tensors (torch, CPU): the columns are used in place -- epi_batch_upload recognises page-locked
        sources and DMAs straight from them (no staging copy)."""
        return cls.from_arrays(xm.numpy()[:int(nbytes)], off.numpy(), rname.numpy(), strand.numpy(), start.numpy(), levels,
                               keepalive=(xm, off, rname, strand, start), device=device)

    @classmethod
    def from_device(cls, xm, nbytes, off, rname, strand, start, levels=None, realign=True):
        """Adopt torch tensors already in HBM (xm: uint8 with capacity >= nbytes rounded up to 16).  realign: the engine
        makes its own position-congruent copy of xm when the batch is created (epi_batch_realign, include/epihip.h) and
        reads neither xm nor off afterwards; drop_source() then gives their memory back.  False: strictly zero-copy."""
        n = int(off.numel()) - 1
        self = cls(n, nbytes, levels)
        self.dev = dict(xm=xm, off=off, rname=rname, strand=strand, start=start)
        self.device = xm.device.index
        self.realign = bool(realign)
        return self

    def drop_source(self):
        """After the batch exists in the engine's own layout: release the adopted xm / off tensors."""
        if self.dev is not None and self._batch is not None and _lib.load().epi_batch_layout(self._batch) > 0:
            self.dev = {k: v for k, v in self.dev.items() if k not in ("xm", "off")}

    def batch(self, device=None):
        """The epi_batch handle (uploads on first use through the library's pinned double-buffered path)."""
        if self._batch is not None:
            return self._batch
        lib = _lib.load()
        h = C.c_void_p()
        if self.dev is not None:
            eng = _engine(self.device)
            d = self.dev
            _lib.check(lib.epi_batch_adopt(eng, C.c_void_p(d["xm"].data_ptr()), d["xm"].numel(), self.nbytes,
                                           C.c_void_p(d["off"].data_ptr()), C.c_void_p(d["rname"].data_ptr()),
                                           C.c_void_p(d["strand"].data_ptr()), C.c_void_p(d["start"].data_ptr()),
                                           self.n, C.byref(h)))
            if getattr(self, "realign", True):
                rc = lib.epi_batch_realign(h, None)
                if rc:
                    lib.epi_batch_free(h)
                    _lib.check(rc)
        else:
            eng = _engine(device if device is not None else self.device)
            self.device = lib.epi_engine_device(eng)
            hst = self.host
            p = lambda a: C.c_void_p(a.ctypes.data) if a.size else None
            _lib.check(lib.epi_batch_upload(eng, p(hst["xm"]), C.c_void_p(hst["off"].ctypes.data), p(hst["rname"]),
                                            p(hst["strand"]), p(hst["start"]), self.n, C.byref(h)))
        self._batch = h
        return h

    def close(self):
        if self._batch is not None:
            _lib.load().epi_batch_free(self._batch)
            self._batch = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _TemplatesOwner:
    """Keeps an epi_templates (epi_preprocess_bam output) alive while numpy views of its buffers are in use."""

    def __init__(self, t):
        self.t = t

    def __del__(self):
        try:
            _lib.load().epi_templates_free(C.byref(self.t))
        except Exception:
            pass


def _as_bam(bam):
    if isinstance(bam, ProcessedBam):
        return bam
    if isinstance(bam, dict):
        return ProcessedBam.from_arrays(bam["xm"], bam["off"], bam["rname"], bam["strand"], bam["start"],
                                        bam.get("levels"))
    raise TypeError("expected a ProcessedBam (preprocessBam() result) or a dict of SoA columns")


def preprocessBam(bam_file, paired=None, min_mapq=0, min_baseq=0, min_prob=-1, highest_prob=True,
                  skip_duplicates=False, skip_secondary=True, skip_qcfail=True, skip_supplementary=True,
                  trim=0, nthreads=1, verbose=False, window_kib=0, genome=None, mates=None):
    """R/preprocessBam.R:197-237.  An already preprocessed object is returned untouched (:226-235);
    a path is decoded by the library's host-side producer (epi_preprocess_bam: zlib BGZF reader + the
    reference's template packer), which yields the sorted SoA batch directly.

    genome: a FASTA path or a Genome (preprocessGenome).  The records callMethylation would call (mapped, carrying the
    strand tag, no XM) are called on the GPU inside the reader (epi_preprocess_bam_genome): the result equals
    preprocessBam(callMethylation(bam_file, tmp, genome); tmp) with the same options, errors included, and no BAM is
    written.  `ncalled` on the result counts the called records (0 without a genome).  There is no CPU path: without
    a device this raises EpihipError.

    mates: "adjacent" (None, the default) reads paired-end input whose mates are neighbours, as the reference does (a
    file that is not name-sorted is refused).  "anywhere" pairs the mates through their QNAMEs wherever they lie
    (coordinate-sorted input, DRAGEN's default) and merges the templates on the GPU (epi_preprocess_bam_anyorder): the
    result equals preprocessBam of the file regrouped by QNAME, READ1 before READ2 (include/epihip.h).  Single-end and
    long-read files read as with "adjacent".  Not together with genome=; no CPU path (EpihipError without a device)."""
    mates = _match_arg(mates, ("adjacent", "anywhere"), "mates")
    if mates == "anywhere" and genome is not None:
        raise ValueError("mates='anywhere' cannot be combined with genome= (yet)")
    if isinstance(bam_file, (ProcessedBam, dict)):
        return _as_bam(bam_file)
    import os
    lib = _lib.load()
    eng = None
    if genome is not None:
        from .genome import preprocessGenome
        genome = preprocessGenome(genome, nthreads=nthreads, verbose=verbose)
        eng = C.c_void_p()
        _lib.check(lib.epi_default_engine(C.byref(eng)))          # no device: EpihipError (as rcpp_call_methylation_genome)
    if mates == "anywhere":
        eng = C.c_void_p()
        _lib.check(lib.epi_default_engine(C.byref(eng)))          # no device: EpihipError, before the file is read
    trim2 = (list(np.atleast_1d(trim)) * 2)[:2]                       # head(rep.int(trim, 2), 2)
    opt = _lib.BamOptions(int(min_mapq), int(min_baseq), int(bool(skip_duplicates)), int(bool(skip_secondary)),
                          int(bool(skip_qcfail)), int(bool(skip_supplementary)), int(trim2[0]), int(trim2[1]),
                          -1 if paired is None else int(bool(paired)), max(int(nthreads), 1), int(min_prob),
                          int(bool(highest_prob)), int(window_kib))
    t = _lib.Templates()
    ncalled = C.c_int64(0)
    path = os.path.expanduser(str(bam_file)).encode()
    if genome is not None:
        rc = lib.epi_preprocess_bam_genome(eng, path, C.byref(opt), genome._h, C.byref(t), C.byref(ncalled))
    elif mates == "anywhere":
        rc = lib.epi_preprocess_bam_anyorder(eng, path, C.byref(opt), C.byref(t))
    else:
        rc = lib.epi_preprocess_bam(path, C.byref(opt), C.byref(t))
    if eng is not None and rc not in (_lib.EPI_OK, _lib.EPI_ERR_ARG):
        _lib.check(rc)                                                # device / HIP failures: EpihipError
    if rc != _lib.EPI_OK:
        msg = lib.epi_last_error().decode("utf-8", "replace")
        raise ValueError(msg)                                         # stop(..., call.=FALSE) in the reference
    # the producer's buffers are used in place (xm is pinned when a device is usable: the upload DMAs straight from it);
    # they are released when the ProcessedBam goes away
    keep = _TemplatesOwner(t)
    n = t.n

    def view(ptr, k):
        # every array owns its buffer: .base is a ctypes array that carries the _TemplatesOwner, so
        # `preprocessBam(p).host["xm"]` stays valid after the ProcessedBam itself is gone
        if k <= 0 or not ptr:
            return np.empty(0, dtype=np.dtype(ptr._type_))
        carr = (ptr._type_ * int(k)).from_address(C.addressof(ptr.contents))
        carr._owner = keep
        return np.frombuffer(carr, dtype=np.dtype(ptr._type_))
    levels = tuple(t.target_names[i].decode("latin1") for i in range(t.n_targets))
    bam = ProcessedBam.from_arrays(view(t.xm, t.nbytes), view(t.off, n + 1), view(t.rname, n), view(t.strand, n),
                                   view(t.start, n), levels, keepalive=keep)
    bam.nrecs, bam.npushed, bam.paired, bam.pinned = int(t.nrecs), int(n), bool(t.paired), bool(t.pinned)
    bam.ncalled = int(ncalled.value)
    return bam


# ---- Rcpp-level functions ----------------------------------------------------------------------

def rcpp_threshold_reads(df, ctx_meth, ctx_unmeth, ooctx_meth, ooctx_unmeth, min_n_ctx, min_ctx_meth_frac,
                         max_ooctx_meth_frac, as_device=False):
    """src/rcpp_threshold_reads.cpp:15-74 -> logical vector (numpy bool, or int32 torch tensor in HBM)."""
    torch = _torch()
    bam = _as_bam(df)
    b = bam.batch()
    out = torch.empty(max(bam.n, 1), dtype=torch.int32, device="cuda:%d" % bam.device)
    _lib.check(_lib.load().epi_batch_threshold_reads_dev(
        b, _lib.enc(ctx_meth), _lib.enc(ctx_unmeth), _lib.enc(ooctx_meth), _lib.enc(ooctx_unmeth),
        int(min_n_ctx), float(min_ctx_meth_frac), float(max_ooctx_meth_frac),
        C.c_void_p(out.data_ptr()), _stream(bam.device)))
    out = out[:bam.n]
    return out if as_device else out.cpu().numpy().astype(bool)


def rcpp_get_xm_beta(df, ctx_meth, ctx_unmeth, as_device=False):
    """src/rcpp_get_xm_beta.cpp:10-43 -> per-read beta (float64)."""
    torch = _torch()
    bam = _as_bam(df)
    b = bam.batch()
    out = torch.empty(max(bam.n, 1), dtype=torch.float64, device="cuda:%d" % bam.device)
    _lib.check(_lib.load().epi_batch_get_xm_beta_dev(b, _lib.enc(ctx_meth), _lib.enc(ctx_unmeth),
                                                     C.c_void_p(out.data_ptr()), _stream(bam.device)))
    out = out[:bam.n]
    return out if as_device else out.cpu().numpy()


def _pass_tensor(bam, pass_):
    """R logical -> int32 device tensor (NA stays non-zero = TRUE, src/rcpp_cx_report.cpp:118)."""
    torch = _torch()
    if pass_ is None:
        return None
    if isinstance(pass_, torch.Tensor):
        t = pass_.to(device="cuda:%d" % bam.device, dtype=torch.int32)
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(pass_).astype(np.int32))).to("cuda:%d" % bam.device)
    if t.numel() != bam.n:
        raise ValueError("pass must have one entry per template")
    return t.contiguous()


def _ptr_array(tensors):
    arr = (C.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr()
    return arr


def _cx_columns(bam, ctx, report):
    """The six int32 columns of a CX report.  They are allocated before the report runs, as many rows as the last report
    on this batch with these contexts had (the row count depends on the rows and the contexts alone), so that the tile
    kernel can write them itself; `report(cols, cap, nrow, written)` runs it.  When it could not (first report, pile-ups,
    ...) the rows come from the library's row pool as before."""
    torch = _torch()
    lib = _lib.load()
    b = bam.batch()
    dev = "cuda:%d" % bam.device
    cap = C.c_int64(-1)
    _lib.check(lib.epi_batch_cx_report_capacity(b, _lib.enc(ctx), C.byref(cap)))
    cap = max(cap.value, 0)
    buf = torch.empty((6, cap), dtype=torch.int32, device=dev)    # one allocation, before the kernels are queued
    nrow, written = C.c_int64(0), C.c_int(0)
    report(_ptr_array(buf.unbind(0)) if cap else None, cap, nrow, written)
    n = nrow.value
    if not written.value:
        if n > cap:
            buf = torch.empty((6, n), dtype=torch.int32, device=dev)
        if n:
            _lib.check(lib.epi_batch_cx_fetch_dev(b, _ptr_array(buf.unbind(0)), _stream(bam.device)))
    return [c[:n] for c in buf.unbind(0)]


def rcpp_cx_report(df, pass_, ctx, as_device=False):
    """src/rcpp_cx_report.cpp:34-159 -> columns rname,strand,pos,context,meth,unmeth (int32)."""
    lib = _lib.load()
    bam = _as_bam(df)
    b = bam.batch()
    p = _pass_tensor(bam, pass_)
    cols = _cx_columns(bam, ctx, lambda cols, cap, nrow, written: _lib.check(lib.epi_batch_cx_report_into_dev(
        b, C.c_void_p(p.data_ptr()) if p is not None and bam.n else None, _lib.enc(ctx), cols, cap, _stream(bam.device),
        C.byref(nrow), C.byref(written))))
    if not as_device:
        cols = [c.cpu().numpy() for c in cols]
    return Report(dict(zip(CX_COLUMNS, cols)), bam.levels)


def cytosine_report_fused(df, ctx_meth, ctx_unmeth, ooctx_meth, ooctx_unmeth, min_n_ctx, min_ctx_meth_frac,
                          max_ooctx_meth_frac, ctx, as_device=False, return_pass=False):
    """rcpp_threshold_reads followed by rcpp_cx_report with its result (what generateCytosineReport does with
    threshold.reads=TRUE, R/generateCytosineReport.R:181-199) as ONE call: epi_batch_cytosine_report_dev decides every
    read inside the tile kernel, from the bytes it has loaded anyway.  Same table as the two calls."""
    torch = _torch()
    lib = _lib.load()
    bam = _as_bam(df)
    b = bam.batch()
    dev = "cuda:%d" % bam.device
    pass_out = torch.empty(max(bam.n, 1), dtype=torch.int32, device=dev) if return_pass else None
    cols = _cx_columns(bam, ctx, lambda cols, cap, nrow, written: _lib.check(lib.epi_batch_cytosine_report_into_dev(
        b, _lib.enc(ctx_meth), _lib.enc(ctx_unmeth), _lib.enc(ooctx_meth), _lib.enc(ooctx_unmeth), int(min_n_ctx),
        float(min_ctx_meth_frac), float(max_ooctx_meth_frac), _lib.enc(ctx),
        C.c_void_p(pass_out.data_ptr()) if pass_out is not None else None, cols, cap, _stream(bam.device),
        C.byref(nrow), C.byref(written))))
    if not as_device:
        cols = [c.cpu().numpy() for c in cols]
    rep = Report(dict(zip(CX_COLUMNS, cols)), bam.levels)
    if return_pass:
        p = pass_out[:bam.n]
        return rep, (p if as_device else p.cpu().numpy().astype(bool))
    return rep


def _fetch_table(bam, fetch, n, nint, names, as_device, extra=()):
    """The columns of a finished report of n rows, nint int32 ones then float64 ones, through the library's `fetch`;
    `extra`: further device tensors (or None) that it takes between the columns and the stream."""
    icols, dcols = _table_cols(nint, len(names) - nint, n, "cuda:%d" % bam.device)
    if n:
        _lib.check(fetch(bam.batch(), _ptr_array(icols), _ptr_array(dcols),
                         *[C.c_void_p(t.data_ptr()) if t is not None else None for t in extra], _stream(bam.device)))
    cols = icols + dcols
    if not as_device:
        cols = [c.cpu().numpy() for c in cols]
    return Report(dict(zip(names, cols)), bam.levels)


def _pattern_counts(bam, n, k, with_counts, sides=1):
    """The [n, 2^k] int32 histograms a heterogeneity fetch fills, one per side (None without with_counts)."""
    torch = _torch()
    return [torch.empty((n, 1 << int(k)), dtype=torch.int32, device="cuda:%d" % bam.device) if with_counts else None
            for _ in range(sides)]


MHL_COLUMNS = ("rname", "strand", "pos", "context", "coverage", "length", "lmhl")
HETEROGENEITY_COLUMNS = ("rname", "strand", "pos", "end", "context", "nreads", "npatterns", "beta", "epipolymorphism", "entropy", "pdr")


def rcpp_mhl_report(df, ctx, hmax, hmin, max_ooctx_meth_frac, as_device=False):
    """src/rcpp_mhl_report.cpp:46-228 -> rname,strand,pos,context,coverage (int32), length,lmhl (float64)."""
    lib = _lib.load()
    bam = _as_bam(df)
    nrow = C.c_int64(0)
    _lib.check(lib.epi_batch_mhl_report_dev(bam.batch(), _lib.enc(ctx), int(hmax), int(hmin), float(max_ooctx_meth_frac),
                                            _stream(bam.device), C.byref(nrow)))
    return _fetch_table(bam, lib.epi_batch_mhl_fetch_dev, nrow.value, 5, MHL_COLUMNS, as_device)


def rcpp_heterogeneity_report(df, ctx, k, max_ooctx_meth_frac, min_reads=1, max_window_span=0, as_device=False,
                              with_counts=False):
    """Per window of k neighbouring sites of the un-thresholded cytosine report (include/epihip.h,
    epi_batch_heterogeneity_report_dev): rname, strand, pos, end, context, nreads, npatterns (int32), beta, epipolymorphism,
    entropy, pdr (float64).  ctx: context letters in both cases, as for rcpp_mhl_report.  with_counts: the Report's
    `counts` attribute holds the [nrow, 2^k] int32 pattern histogram of the reported windows."""
    lib = _lib.load()
    bam = _as_bam(df)
    nrow = C.c_int64(0)
    _lib.check(lib.epi_batch_heterogeneity_report_dev(bam.batch(), _lib.enc(ctx), int(k), float(max_ooctx_meth_frac), int(min_reads),
                                                      int(max_window_span), _stream(bam.device), C.byref(nrow)))
    counts = _pattern_counts(bam, nrow.value, k, with_counts)
    rep = _fetch_table(bam, lib.epi_batch_heterogeneity_fetch_dev, nrow.value, 7, HETEROGENEITY_COLUMNS, as_device, counts)
    if with_counts:
        rep.counts, = counts if as_device else [c.cpu().numpy() for c in counts]
    return rep


HETEROGENEITY_COMPARE_COLUMNS = ("rname", "strand", "pos", "end", "context", "nreads_a", "nreads_b", "npatterns_a", "npatterns_b", "df",
                                 "beta_a", "beta_b", "entropy_a", "entropy_b", "epipolymorphism_a", "epipolymorphism_b", "pdr_a", "pdr_b",
                                 "delta_beta", "delta_entropy", "jsd", "tvd", "g")


def _batch_pair(bam_a, bam_b):
    """The batches of two inputs that are compared: one sequence dictionary (checked before anything is uploaded), then
    both on the device of the first."""
    if bam_a.levels != bam_b.levels:
        raise ValueError("the two inputs have different sequence names (levels): their rname codes cannot be compared")
    a = bam_a.batch()
    b = bam_b.batch(bam_a.device)
    if bam_b.device != bam_a.device:
        raise ValueError("the two inputs are on different devices (%s and %s)" % (bam_a.device, bam_b.device))
    return a, b


def rcpp_heterogeneity_compare(df_a, df_b, ctx, k, max_ooctx_meth_frac, min_reads=1, max_window_span=0, as_device=False,
                               with_counts=False):
    """Per window of k neighbouring sites that the un-thresholded cytosine reports of both inputs have (include/epihip.h,
    epi_batch_heterogeneity_compare_dev): rname, strand, pos, end, context, nreads_a, nreads_b, npatterns_a, npatterns_b, df
    (int32), beta, entropy, epipolymorphism and pdr of either input, delta_beta, delta_entropy, jsd, tvd, g (float64).
    Both inputs under one sequence dictionary (differing `levels`: ValueError), on one device.  The Report carries df_a's
    levels and `ncommon`, the number of common sites; with_counts: `counts_a` and `counts_b` hold the [nrow, 2^k] int32
    pattern histograms of the reported windows."""
    bam_a, bam_b = _as_bam(df_a), _as_bam(df_b)
    a, b = _batch_pair(bam_a, bam_b)
    ncommon, nrow = C.c_int64(0), C.c_int64(0)
    lib = _lib.load()
    _lib.check(lib.epi_batch_heterogeneity_compare_dev(a, b, _lib.enc(ctx), int(k), float(max_ooctx_meth_frac), int(min_reads),
                                                       int(max_window_span), _stream(bam_a.device), C.byref(ncommon), C.byref(nrow)))
    counts = _pattern_counts(bam_a, nrow.value, k, with_counts, sides=2)
    rep = _fetch_table(bam_a, lib.epi_batch_heterogeneity_compare_fetch_dev, nrow.value, 10, HETEROGENEITY_COMPARE_COLUMNS, as_device, counts)
    rep.ncommon = ncommon.value
    if with_counts:
        rep.counts_a, rep.counts_b = counts if as_device else [c.cpu().numpy() for c in counts]
    return rep


LINKAGE_COLUMNS = ("rname", "strand", "pos", "pos2", "context", "neighbour", "nreads", "n_uu", "n_mu", "n_um", "n_mm",
                   "cov", "r2", "dprime")
BLOCK_COLUMNS = ("rname", "strand", "start", "end", "nsites", "mean_r2")


def _linkage_run(bam, ctx, max_neighbours, max_distance, max_ooctx_meth_frac, min_reads):
    """epi_batch_linkage_report_dev on the batch of `bam`: the number of reported pairs."""
    nrow = C.c_int64(0)
    _lib.check(_lib.load().epi_batch_linkage_report_dev(bam.batch(), _lib.enc(ctx), int(max_neighbours), int(max_distance),
                                                        float(max_ooctx_meth_frac), int(min_reads), _stream(bam.device),
                                                        C.byref(nrow)))
    return nrow.value


def rcpp_linkage_report(df, ctx, max_neighbours, max_distance, max_ooctx_meth_frac, min_reads=1, as_device=False):
    """Per pair (s_j, s_{j+d}), d = 1 .. max_neighbours, of sites of the un-thresholded cytosine report (include/epihip.h,
    epi_batch_linkage_report_dev): rname, strand, pos, pos2, context, neighbour, nreads, n_uu, n_mu, n_um, n_mm (int32),
    cov, r2, dprime (float64).  ctx: context letters in both cases, as for rcpp_mhl_report."""
    bam = _as_bam(df)
    n = _linkage_run(bam, ctx, max_neighbours, max_distance, max_ooctx_meth_frac, min_reads)
    return _fetch_table(bam, _lib.load().epi_batch_linkage_fetch_dev, n, 11, LINKAGE_COLUMNS, as_device)


def rcpp_linkage_blocks(df, ctx, max_neighbours, max_distance, max_ooctx_meth_frac, min_reads, min_r2, min_sites, as_device=False):
    """The haplotype blocks of the pair table rcpp_linkage_report computes with the same arguments
    (epi_batch_linkage_blocks_dev): rname, strand, start, end, nsites (int32), mean_r2 (float64)."""
    lib = _lib.load()
    bam = _as_bam(df)
    _linkage_run(bam, ctx, max_neighbours, max_distance, max_ooctx_meth_frac, min_reads)
    nblock = C.c_int64(0)
    _lib.check(lib.epi_batch_linkage_blocks_dev(bam.batch(), float(min_r2), int(min_sites), _stream(bam.device), C.byref(nblock)))
    return _fetch_table(bam, lib.epi_batch_linkage_blocks_fetch_dev, nblock.value, 5, BLOCK_COLUMNS, as_device)


FDRP_COLUMNS = ("rname", "strand", "pos", "context", "coverage", "nreads", "npairs", "ndiscordant", "fdrp", "qfdrp")


def rcpp_fdrp_report(df, ctx, flank_sites, max_reads, min_overlap, max_distance, max_ooctx_meth_frac, min_reads=2, as_device=False):
    """Per site of the un-thresholded cytosine report, over the pairs of reads that have a call there (include/epihip.h,
    epi_batch_fdrp_report_dev): rname, strand, pos, context, coverage, nreads, npairs, ndiscordant (int32), fdrp, qfdrp
    (float64).  ctx: context letters in both cases, as for rcpp_mhl_report."""
    lib = _lib.load()
    bam = _as_bam(df)
    nrow = C.c_int64(0)
    _lib.check(lib.epi_batch_fdrp_report_dev(bam.batch(), _lib.enc(ctx), int(flank_sites), int(max_reads), int(min_overlap),
                                             int(max_distance), float(max_ooctx_meth_frac), int(min_reads), _stream(bam.device),
                                             C.byref(nrow)))
    return _fetch_table(bam, lib.epi_batch_fdrp_fetch_dev, nrow.value, 8, FDRP_COLUMNS, as_device)


REGION_COLUMNS = ("rname", "start", "end", "nreads", "nlong", "kreads", "tbase", "mbase", "cbase", "ndiscordant",
                  "nmethylated", "n_u", "n_x", "n_m", "maxsites", "beta", "pdr", "chalm", "mcr", "mbs", "mhl")


def rcpp_region_report(df, regions, ctx, min_sites, max_sites, reverse_offset, u_max, m_min, max_ooctx_meth_frac, as_device=False):
    """One row per region, in the order given, from the calls that the kept rows have inside it (include/epihip.h,
    epi_batch_region_report_dev): rname, start, end, nreads, nlong, kreads, tbase, mbase, cbase, ndiscordant, nmethylated,
    n_u, n_x, n_m, maxsites (int32), beta, pdr, chalm, mcr, mbs, mhl (float64).  regions: (rname codes, start, end), three
    integer sequences, numpy arrays or device tensors of one length (1-based closed ranges; a code that no row has, NA
    included, gives a row of zero counts).  ctx: context letters in both cases, as for rcpp_mhl_report."""
    torch = _torch()
    lib = _lib.load()
    bam = _as_bam(df)
    b = bam.batch()
    dev = "cuda:%d" % bam.device
    cols3 = [r.to(device=dev, dtype=torch.int32).contiguous() if isinstance(r, torch.Tensor)
             else torch.from_numpy(np.ascontiguousarray(np.asarray(r, np.int64).astype(np.int32))).to(dev) for r in regions]
    if len(cols3) != 3 or any(c.dim() != 1 or c.numel() != cols3[0].numel() for c in cols3):
        raise ValueError("regions: expected (rname codes, start, end), three sequences of one length")
    n = int(cols3[0].numel())
    icols, dcols = _table_cols(15, 6, n, dev)
    _lib.check(lib.epi_batch_region_report_dev(b, *[C.c_void_p(c.data_ptr()) if n else None for c in cols3], n, _lib.enc(ctx), int(min_sites),
                                               int(max_sites), int(reverse_offset), float(u_max), float(m_min), float(max_ooctx_meth_frac),
                                               _ptr_array(icols), _ptr_array(dcols), _stream(bam.device)))
    cols = icols + dcols
    if not as_device:
        cols = [c.cpu().numpy() for c in cols]
    return Report(dict(zip(REGION_COLUMNS, cols)), bam.levels)


MBIAS_COLUMNS = ("end", "strand", "context", "offset", "meth", "unmeth", "beta")
MBIAS_END_LEVELS = ("start", "end")
_MBIAS_CODES = (2, 6, 7)                                  # context codes in table order: CHH, CHG, CG
_MBIAS_MAX_OFFSET = 1024


def _beta(meth, unmeth):
    """meth / (meth + unmeth) in float64, NaN at 0 / 0 (numpy arrays or tensors)"""
    if isinstance(meth, np.ndarray):
        with np.errstate(invalid="ignore", divide="ignore"):
            return meth.astype(np.float64) / (meth + unmeth).astype(np.float64)
    return meth.double() / (meth + unmeth).double()


def _mbias_select(rep, codes):
    """The rows of an M-bias report (and of its totals) whose context code is one of `codes`, in their order"""
    def rows(r):
        ctx = r["context"]
        keep = np.isin(ctx, codes) if isinstance(ctx, np.ndarray) else sum(ctx == c for c in codes).bool()
        out = Report({k: v[keep] for k, v in r.items()}, r.levels["rname"])
        out.levels = dict(r.levels)
        return out
    out = rows(rep)
    out.totals = rows(rep.totals)
    return out


def rcpp_mbias_report(df, max_offset, as_device=False):
    """Methylation by offset from either end of the template (include/epihip.h, epi_batch_mbias_report_dev): 12 * max_offset
    dense rows in the order end (1 = start, 2 = end), strand, context (2 = CHH, 6 = CHG, 7 = CG), offset (0-based), all-zero
    rows included; meth and unmeth (int32) count the bytes of that class at that offset of that end over every row of the
    batch, beta = meth / (meth + unmeth) in float64 (NaN at 0 / 0).  The Report's `totals` (always on the host) has one row
    per strand and context over every byte of the batch: strand, context, meth, unmeth (int64) and beta."""
    torch = _torch()
    max_offset = _whole_number(max_offset, "max.offset", 1, _MBIAS_MAX_OFFSET)
    bam = _as_bam(df)
    b = bam.batch()
    dev = "cuda:%d" % bam.device
    counts = torch.empty(24 * max_offset, dtype=torch.int64, device=dev)
    totals = torch.empty(12, dtype=torch.int64, device=dev)
    _lib.check(_lib.load().epi_batch_mbias_report_dev(b, max_offset, C.c_void_p(counts.data_ptr()), C.c_void_p(totals.data_ptr()),
                                                      _stream(bam.device)))
    if int(counts.max()) > 2 ** 31 - 1:                   # (a cell gets at most one count per row)
        raise ValueError("rcpp_mbias_report: a cell counts more than 2^31 - 1 rows, which an int32 column cannot hold")
    cells = counts.view(-1, 2).to(torch.int32)
    meth, unmeth = cells[:, 0].contiguous(), cells[:, 1].contiguous()
    grid = np.indices((2, 2, 3, max_offset), dtype=np.int32).reshape(4, -1)
    keys = [grid[0] + 1, grid[1] + 1, np.asarray(_MBIAS_CODES, np.int32)[grid[2]], grid[3]]
    if as_device:
        cols = [torch.from_numpy(np.ascontiguousarray(k)).to(dev) for k in keys] + [meth, unmeth]
    else:
        cols = keys + [meth.cpu().numpy(), unmeth.cpu().numpy()]
    cols.append(_beta(cols[4], cols[5]))
    rep = Report(dict(zip(MBIAS_COLUMNS, cols)), bam.levels)
    rep.levels["end"] = MBIAS_END_LEVELS
    t = totals.cpu().numpy().reshape(6, 2)
    tg = np.indices((2, 3), dtype=np.int32).reshape(2, -1)
    tm, tu = np.ascontiguousarray(t[:, 0]), np.ascontiguousarray(t[:, 1])
    rep.totals = Report(dict(strand=tg[0] + 1, context=np.asarray(_MBIAS_CODES, np.int32)[tg[1]], meth=tm, unmeth=tu, beta=_beta(tm, tu)),
                        bam.levels)
    return rep


CX_COMPARE_COLUMNS = ("rname", "strand", "pos", "context", "meth_a", "unmeth_a", "meth_b", "unmeth_b", "beta_a", "beta_b", "delta_beta", "p")
DMR_COLUMNS = ("rname", "start", "end", "nsites", "direction", "beta_a", "beta_b", "delta_beta", "mean_delta_beta", "p")


def _device_columns(rep, names, what):
    """The named columns of a device Report (int32 ones first, then float64 ones): contiguous tensors, all on one GPU."""
    torch = _torch()
    cols = []
    for i, k in enumerate(names):
        if k not in rep or not isinstance(rep[k], torch.Tensor) or not rep[k].is_cuda:
            raise TypeError("%s: expected a device Report (as_device=True) with the column '%s'" % (what, k))
        cols.append(rep[k].contiguous())
        if cols[i].dtype not in (torch.int32, torch.float64) or cols[i].shape != cols[0].shape or cols[i].device != cols[0].device:
            raise TypeError("%s: column '%s' does not fit the table (int32 / float64 columns of one length on one device)" % (what, k))
    return cols


def _table_to_host(rep, as_device):
    if as_device:
        return rep
    out = Report({k: v.cpu().numpy() for k, v in rep.items()}, rep.levels["rname"])
    out.__dict__.update({k: v for k, v in rep.__dict__.items() if k != "levels"})
    return out


def rcpp_cx_compare(rep_a, rep_b, min_coverage=1, as_device=False):
    """Two device cytosine reports (rcpp_cx_report / generateCytosineReport with as_device=True) against each other per
    cytosine both have (include/epihip.h, epi_cx_compare_dev): rname, strand, pos, context, meth_a, unmeth_a, meth_b,
    unmeth_b (int32), beta_a, beta_b, delta_beta = beta_b - beta_a and the two-sided Fisher exact p of (meth_a unmeth_a /
    meth_b unmeth_b) (float64), for the common sites covered min_coverage times in either.  Both reports under one
    sequence dictionary (differing `levels`: ValueError), on one device, rows ascending in (rname, pos, strand).  The
    Report carries rep_a's levels and `ncommon`, the number of common sites."""
    min_coverage = _whole_number(min_coverage, "min.coverage", 0, 2 ** 31 - 1)
    if rep_a.levels["rname"] != rep_b.levels["rname"]:
        raise ValueError("the two reports have different sequence names (levels): their rname codes cannot be compared")
    torch = _torch()
    lib = _lib.load()
    a, b = _device_columns(rep_a, CX_COLUMNS, "rcpp_cx_compare"), _device_columns(rep_b, CX_COLUMNS, "rcpp_cx_compare")
    if a[0].device != b[0].device:
        raise ValueError("the two reports are on different devices (%s and %s)" % (a[0].device, b[0].device))
    dev = a[0].device
    na, nb = int(a[0].numel()), int(b[0].numel())
    cap = min(na, nb)
    icols, dcols = _table_cols(8, 4, cap, dev)
    ncommon, nrow = C.c_int64(0), C.c_int64(0)
    _lib.check(lib.epi_cx_compare_dev(_engine(dev.index), _ptr_array(a), na, _ptr_array(b), nb, min_coverage, _ptr_array(icols),
                                      _ptr_array(dcols), cap, _stream(dev.index), C.byref(ncommon), C.byref(nrow)))
    rep = Report(dict(zip(CX_COMPARE_COLUMNS, [c[:nrow.value] for c in icols + dcols])), rep_a.levels["rname"])
    rep.ncommon = ncommon.value
    return _table_to_host(rep, as_device)


SMOOTH_COLUMNS = CX_COLUMNS + ("nsites", "halfwidth", "degree", "beta", "smoothed", "weight")
_SMOOTH_MAX_BANDWIDTH, _SMOOTH_MAX_WINDOW, _SMOOTH_MAX_DEGREE = 2 ** 30, 65536, 2        # EPI_SMOOTH_MAX_*


def _smooth_args(bandwidth, min_sites, max_gap, degree):
    return (_whole_number(bandwidth, "bandwidth", 1, _SMOOTH_MAX_BANDWIDTH), _whole_number(min_sites, "min.sites", 1, _SMOOTH_MAX_WINDOW),
            _whole_number(max_gap, "max.gap", 0, 2 ** 31 - 1), _whole_number(degree, "degree", 0, _SMOOTH_MAX_DEGREE))


def rcpp_cx_merge_strands(rep, as_device=False):
    """CpG strand merging of a device cytosine report (include/epihip.h, epi_cx_merge_strands_dev): the '-' row of a CpG at
    pos + 1 is added to the '+' row at pos; a '-' CpG row without a '+' partner moves to (pos - 1, '+') where nothing stands
    in its way and stays otherwise; every other row is copied.  Rows ascending in (rname, pos, strand).  The Report carries
    rep's levels and `nmerged`, `nmoved`, `nkept`: the pairs, and the lone '-' CpG rows that moved and that stayed."""
    torch = _torch()
    lib = _lib.load()
    cols = _device_columns(rep, CX_COLUMNS, "rcpp_cx_merge_strands")
    dev = cols[0].device
    n = int(cols[0].numel())
    out, _ = _table_cols(6, 0, n, dev)
    counts = [C.c_int64(0) for _ in range(4)]
    _lib.check(lib.epi_cx_merge_strands_dev(_engine(dev.index), _ptr_array(cols), n, _ptr_array(out), n, _stream(dev.index),
                                            *[C.byref(c) for c in counts]))
    res = Report(dict(zip(CX_COLUMNS, [c[:counts[0].value] for c in out])), rep.levels["rname"])
    res.nmerged, res.nmoved, res.nkept = counts[1].value, counts[2].value, counts[3].value
    return _table_to_host(res, as_device)


def rcpp_cx_smooth(rep, bandwidth=1000, min_sites=70, max_gap=10 ** 8, degree=2, as_device=False):
    """Local-regression smoothing of a device cytosine report (include/epihip.h, epi_cx_smooth_dev, has the definitions):
    per row a tricube-weighted, coverage-weighted polynomial fit of `degree` over the neighbouring cytosines of the same
    rname, strand and context -- those closer than max(bandwidth, the distance that takes in min_sites sites), within a
    cluster of sites whose neighbours are at most max_gap apart.  SMOOTH_COLUMNS: the six columns of rep, nsites,
    halfwidth, degree (the degree the fit could use; -1: no coverage in the window), beta, smoothed and weight, in rep's
    row order.  The Report carries rep's levels, `ncluster` and `max_window`."""
    bandwidth, min_sites, max_gap, degree = _smooth_args(bandwidth, min_sites, max_gap, degree)
    torch = _torch()
    lib = _lib.load()
    cols = _device_columns(rep, CX_COLUMNS, "rcpp_cx_smooth")
    dev = cols[0].device
    n = int(cols[0].numel())
    icols, dcols = _table_cols(9, 3, n, dev)
    ncluster, max_window = C.c_int64(0), C.c_int64(0)
    _lib.check(lib.epi_cx_smooth_dev(_engine(dev.index), _ptr_array(cols), n, bandwidth, min_sites, max_gap, degree, _ptr_array(icols),
                                     _ptr_array(dcols), _stream(dev.index), C.byref(ncluster), C.byref(max_window)))
    res = Report(dict(zip(SMOOTH_COLUMNS, icols + dcols)), rep.levels["rname"])
    res.ncluster, res.max_window = ncluster.value, max_window.value
    return _table_to_host(res, as_device)


def _cx_report_on_device(report, what):
    """(device Report, was it one already) of a cytosine report on the host or on a device: a host one is uploaded."""
    torch = _torch()
    missing = [k for k in CX_COLUMNS if k not in report]
    if missing:
        raise TypeError("%s: expected a cytosine report with the column '%s'" % (what, missing[0]))
    if all(isinstance(report[k], torch.Tensor) and report[k].is_cuda for k in CX_COLUMNS):
        return report, True
    cols = []
    for k in CX_COLUMNS:
        a = report[k].cpu().numpy() if isinstance(report[k], torch.Tensor) else np.asarray(report[k])
        if a.dtype.kind not in "iu" or a.ndim != 1 or a.shape != np.shape(report[CX_COLUMNS[0]]):
            raise TypeError("%s: column '%s' does not fit the table (integer columns of one length)" % (what, k))
        if a.size and (a.min() < -2 ** 31 or a.max() > 2 ** 31 - 1):
            raise ValueError("%s: column '%s' should hold 32-bit integers" % (what, k))
        cols.append(np.ascontiguousarray(a, np.int32))
    _, _, dev = _engine_of(())
    out = Report({k: torch.from_numpy(a).to(dev) for k, a in zip(CX_COLUMNS, cols)}, report.levels["rname"])
    out.levels = dict(report.levels)
    return out, False


def mergeCpgStrands(report):
    """A cytosine report (generateCytosineReport, on the host or with as_device=True) with the two strands of every CpG
    merged into one row at the '+' strand's position, meth and unmeth summed: Bismark's --merge_CpG, methylKit's
    destrand=TRUE (rcpp_cx_merge_strands has the rules for a CpG seen on one strand only).  A host report is uploaded and
    the result comes back to the host; a device report gives a device report.  The Report keeps `levels` and carries
    `nmerged`, `nmoved` and `nkept`.  The reference has no such function."""
    rep, on_device = _cx_report_on_device(report, "mergeCpgStrands")
    out = rcpp_cx_merge_strands(rep, as_device=on_device)
    out.levels = dict(report.levels)
    return out


def smoothCytosineReport(report, bandwidth=1000, min_sites=70, max_gap=10 ** 8, degree=2):
    """A cytosine report (on the host or a device, thresholded or not, strands merged or not) with three columns that make
    low-coverage data comparable -- the raw beta, `smoothed`, a local polynomial regression of methylation over the
    neighbouring cytosines of the same sequence, strand and context, and its `weight` (the kernel-weighted coverage of the
    window) -- and the window's `nsites`, `halfwidth` and the `degree` the fit used (the idea of bsseq's BSmooth and of
    DSS's smoothing, as a weighted least-squares fit on the beta scale): the window of a cytosine holds the sites closer
    than max(bandwidth, the distance that takes in min_sites sites), and never reaches across a gap of more than max_gap
    bases; degree 0 is a weighted mean, 1 a local line, 2 a local parabola (lowered where the window cannot support it).
    A cytosine without coverage gets a smoothed value from its neighbours; a window without any coverage gives NaN.  A
    host report is uploaded and the result comes back to the host; a device report gives a device report.  The Report keeps
    `levels` and carries `ncluster` and `max_window`.  The reference has no such function."""
    args = _smooth_args(bandwidth, min_sites, max_gap, degree)
    rep, on_device = _cx_report_on_device(report, "smoothCytosineReport")
    out = rcpp_cx_smooth(rep, *args, as_device=on_device)
    out.levels = dict(report.levels)
    return out


SEGMENT_SITE_COLUMNS = CX_COLUMNS + ("state",)
SEGMENT_COLUMNS = ("rname", "strand", "context", "start", "end", "state", "nsites", "meth", "unmeth", "beta")
EPI_SEGMENT_MIN_STATES, EPI_SEGMENT_MAX_STATES, EPI_SEGMENT_MAX_COVERAGE, EPI_SEGMENT_MAX_SITES = 2, 4, 32767, 2 ** 26
_SEGMENT_FLOOR = 2.0 ** -16                                # the smallest probability of a model (include/epihip.h, Model)


def _segment_args(max_gap, max_coverage, max_iter):
    return (_whole_number(max_gap, "max.gap", 0, 2 ** 31 - 1), _whole_number(max_coverage, "max.coverage", 1, EPI_SEGMENT_MAX_COVERAGE),
            _whole_number(max_iter, "max.iter", 1, 2 ** 31 - 1))


def _segment_numbers(values, name, shape):
    try:
        a = np.array(values, dtype=np.float64)
    except (TypeError, ValueError):
        a = None
    if a is None or a.shape != shape or np.asarray(values).dtype.kind not in "fiu":
        raise ValueError("'%s' should hold %s numbers" % (name, " x ".join(str(x) for x in shape)))
    return np.ascontiguousarray(a)


def _segment_model(p, trans, init):
    """(p, trans, init) as contiguous float64 arrays of K, K x K and K entries, checked as epi_cx_segment_dev checks them."""
    k = len(p) if hasattr(p, "__len__") else 0
    if not EPI_SEGMENT_MIN_STATES <= k <= EPI_SEGMENT_MAX_STATES:
        raise ValueError("'p' should hold %d to %d methylation levels, one per state" % (EPI_SEGMENT_MIN_STATES, EPI_SEGMENT_MAX_STATES))
    p, trans, init = _segment_numbers(p, "p", (k,)), _segment_numbers(trans, "trans", (k, k)), _segment_numbers(init, "init", (k,))
    for a, name, top in ((p, "p", 1.0 - _SEGMENT_FLOOR), (trans, "trans", 1.0), (init, "init", 1.0)):
        if not ((a >= _SEGMENT_FLOOR) & (a <= top)).all():
            raise ValueError("every entry of '%s' should lie between 2^-16 and %s" % (name, "1 - 2^-16" if name == "p" else "1"))
    for row, name in [(trans[j], "every row of 'trans'") for j in range(k)] + [(init, "'init'")]:
        if not abs(float(np.add.accumulate(row)[-1]) - 1.0) <= 1e-9:
            raise ValueError("%s should sum to 1" % name)
    return p, trans, init


def _segment_start(state_beta, stay):
    """The model segmentCytosineReport starts from: the states' levels, trans[j][j] = stay with the rest of a row shared
    evenly, a uniform init."""
    k = len(state_beta) if hasattr(state_beta, "__len__") else 0
    if not EPI_SEGMENT_MIN_STATES <= k <= EPI_SEGMENT_MAX_STATES:
        raise ValueError("'state.beta' should hold %d to %d methylation levels, one per state" % (EPI_SEGMENT_MIN_STATES, EPI_SEGMENT_MAX_STATES))
    p = _segment_numbers(state_beta, "state.beta", (k,))
    if not ((p >= _SEGMENT_FLOOR) & (p <= 1.0 - _SEGMENT_FLOOR)).all():
        raise ValueError("every entry of 'state.beta' should lie between 2^-16 and 1 - 2^-16")
    if isinstance(stay, (bool, np.bool_)) or not isinstance(stay, (int, float, np.integer, np.floating)) or \
            not (stay >= _SEGMENT_FLOOR and (1.0 - stay) / (k - 1) >= _SEGMENT_FLOOR):
        raise ValueError("'stay' should be a number from 2^-16 to 1 - %d * 2^-16" % (k - 1))
    trans = np.full((k, k), (1.0 - float(stay)) / (k - 1), np.float64)
    trans[np.arange(k), np.arange(k)] = float(stay)
    return _segment_model(p, trans, np.full(k, 1.0 / k, np.float64))


def rcpp_cx_segment(rep, p, trans, init, max_gap=5000, max_coverage=1000, max_iter=10, as_device=False):
    """Methylation segments of a device cytosine report by a hidden Markov model (include/epihip.h, epi_cx_segment_dev, has
    the model): K = len(p) states with methylation levels p, transitions trans (K x K) and initial distribution init,
    decoded by exact Viterbi per chain -- the cytosines of one rname, strand and context whose neighbours are at most
    max_gap apart -- on counts clipped to max_coverage, and refitted by hard EM for at most max_iter decodes (1: a pure
    decode).  SEGMENT_SITE_COLUMNS: the six columns of rep and `state`, in rep's row order.  The Report carries rep's
    levels, `segments` (a Report of SEGMENT_COLUMNS: the maximal runs of one state inside a chain), `fit` (p, trans, init,
    score, iterations, converged), `nchain` and `nsegment`."""
    p, trans, init = _segment_model(p, trans, init)
    max_gap, max_coverage, max_iter = _segment_args(max_gap, max_coverage, max_iter)
    torch = _torch()
    lib = _lib.load()
    cols = _device_columns(rep, CX_COLUMNS, "rcpp_cx_segment")
    dev = cols[0].device
    n = int(cols[0].numel())
    k = int(p.size)
    state = torch.empty(n, dtype=torch.int32, device=dev)
    icols, dcols = _table_cols(7, 3, n, dev)
    fit, nchain, nsegment = _lib.SegmentFit(), C.c_int64(0), C.c_int64(0)
    _lib.check(lib.epi_cx_segment_dev(_engine(dev.index), _ptr_array(cols), n, k, p.ctypes.data, trans.ctypes.data, init.ctypes.data, max_gap,
                                      max_coverage, max_iter, C.c_void_p(state.data_ptr()), _ptr_array(icols), _ptr_array(dcols), n,
                                      _stream(dev.index), C.byref(fit), C.byref(nchain), C.byref(nsegment)))
    levels = rep.levels["rname"]
    res = Report(dict(zip(SEGMENT_SITE_COLUMNS, cols + [state])), levels)
    segs = Report(dict(zip(SEGMENT_COLUMNS, [c[:nsegment.value] for c in icols + dcols])), levels)
    res.segments = _table_to_host(segs, as_device)
    res.fit = dict(p=np.array(fit.p[:k]), trans=np.array(fit.trans[:k * k]).reshape(k, k), init=np.array(fit.init[:k]), score=int(fit.score),
                   iterations=int(fit.iterations), converged=int(fit.converged))
    res.nchain, res.nsegment = nchain.value, nsegment.value
    return _table_to_host(res, as_device)


def segmentCytosineReport(report, state_beta=(0.1, 0.5, 0.9), stay=0.99, max_gap=5000, max_coverage=1000, max_iter=10):
    """A cytosine report (on the host or a device, strands merged or not) cut into regions of its own: every cytosine gets
    the `state` of a hidden Markov model whose states emit methylated calls at the levels `state_beta` (two to four of
    them: say unmethylated, partially and fully methylated), and the maximal runs of one state become `segments` (rname,
    strand, context, start, end, state, nsites and the run's meth, unmeth and beta) -- the idea of MethylSeekR's UMR / LMR /
    PMD and methpipe's hmr / pmd.  The model starts with the probability `stay` of keeping a state from one cytosine to the
    next (the rest shared evenly) and a uniform start, is decoded exactly (Viterbi) per chain of cytosines of one
    sequence, strand and context whose neighbours are at most max_gap bases apart, with coverage above max_coverage scaled
    down to it, and is refitted to its own decode (hard EM) until nothing changes or max_iter decodes have run (1: a pure
    decode of the starting model).  A host report is uploaded and the result comes back to the host; a device report gives
    a device report.  The Report keeps `levels` and carries `segments`, `fit`, `nchain` and `nsegment`.  The reference has
    no such function."""
    p, trans, init = _segment_start(state_beta, stay)
    args = _segment_args(max_gap, max_coverage, max_iter)
    rep, on_device = _cx_report_on_device(report, "segmentCytosineReport")
    out = rcpp_cx_segment(rep, p, trans, init, *args, as_device=on_device)
    out.levels = dict(report.levels)
    out.segments.levels = dict(report.levels)
    return out


def _region_args(max_p, min_delta_beta, max_gap, min_sites, p_name="max.p"):
    for value, name in ((max_p, p_name), (min_delta_beta, "min.delta.beta")):
        if isinstance(value, bool) or not 0 <= value <= 1:
            raise ValueError("'%s' should be a number from 0 to 1" % name)
    return float(max_p), float(min_delta_beta), _whole_number(max_gap, "max.gap", 0, 2 ** 31 - 1), _whole_number(min_sites, "min.sites", 1, 2 ** 31 - 1)


def rcpp_cx_compare_regions(rep, max_p=0.05, min_delta_beta=0.1, max_gap=500, min_sites=3, as_device=False, significance="p"):
    """The differentially methylated regions of a device comparison table (rcpp_cx_compare with as_device=True;
    include/epihip.h, epi_cx_compare_regions_dev): maximal runs of at least min_sites consecutive rows with p <= max_p and
    |delta_beta| >= min_delta_beta, of one direction and sequence, neighbours at most max_gap apart.  rname, start, end,
    nsites, direction (int32), the pooled beta_a, beta_b and delta_beta, mean_delta_beta and the Fisher p of the pooled
    table (float64).  significance="q": the table's `q` column (adjustReport) is what max_p is tested against."""
    max_p, min_delta_beta, max_gap, min_sites = _region_args(max_p, min_delta_beta, max_gap, min_sites)
    significance = _match_arg(significance, ("p", "q"), "significance")
    torch = _torch()
    lib = _lib.load()
    cols = _device_columns(rep, CX_COMPARE_COLUMNS[:-1] + (significance,), "rcpp_cx_compare_regions")
    dev = cols[0].device
    n = int(cols[0].numel())
    cap = n // min_sites                                   # (runs do not overlap)
    icols, dcols = _table_cols(5, 5, cap, dev)
    nregion = C.c_int64(0)
    _lib.check(lib.epi_cx_compare_regions_dev(_engine(dev.index), _ptr_array(cols[:8]), _ptr_array(cols[8:]), n, max_p, min_delta_beta,
                                              max_gap, min_sites, _ptr_array(icols), _ptr_array(dcols), cap, _stream(dev.index),
                                              C.byref(nregion)))
    out = Report(dict(zip(DMR_COLUMNS, [c[:nregion.value] for c in icols + dcols])), rep.levels["rname"])
    return _table_to_host(out, as_device)


def _fisher_cells(x, name):
    """One cell of the tables as int32: a device tensor stays on its device; NaN in a float array-like is NA."""
    torch = _torch()
    if isinstance(x, torch.Tensor):
        if x.dtype.is_floating_point or x.dtype.is_complex:
            raise ValueError("'%s' should hold integers" % name)
        return x.reshape(-1)
    v = np.asarray(x).reshape(-1)
    if v.dtype.kind == "f":
        nan = np.isnan(v)
        w = np.where(nan, 0.0, v)
        if np.any(w != np.floor(w)):
            raise ValueError("'%s' should hold integers" % name)
        v = np.where(nan, float(NA_INTEGER), w)
    elif v.dtype.kind not in "iub":
        raise ValueError("'%s' should hold integers" % name)
    if v.size and (v.min() < NA_INTEGER or v.max() > 2 ** 31 - 1):
        raise ValueError("'%s' should hold 32-bit integers" % name)
    return np.ascontiguousarray(v.astype(np.int32))


def fisherExact(a, b, c, d, as_device=False):
    """Two-sided Fisher exact p-values of the 2x2 tables (a[i] b[i] / c[i] d[i]) on the GPU (epi_fisher_exact_dev): the
    definition of rcpp_fep, one thread per table.  a, b, c, d: array-likes or device tensors of integers, one length; a
    negative cell (NA) gives NaN.  Returns float64, a device tensor with as_device."""
    cells = [_fisher_cells(x, k) for x, k in zip((a, b, c, d), "abcd")]
    n = int(cells[0].shape[0])
    if any(int(x.shape[0]) != n for x in cells):
        raise ValueError("'a', 'b', 'c' and 'd' should have one length")
    torch = _torch()
    lib = _lib.load()
    eng, index, dev = _engine_of(cells)
    cells = [(x if isinstance(x, torch.Tensor) else torch.from_numpy(x)).to(device=dev, dtype=torch.int32).contiguous() for x in cells]
    p = torch.empty(n, dtype=torch.float64, device=dev)
    _lib.check(lib.epi_fisher_exact_dev(eng, *[C.c_void_p(x.data_ptr()) for x in cells], n, C.c_void_p(p.data_ptr()), _stream(index)))
    return p if as_device else p.cpu().numpy()


def _tail_values(x, name):
    """A column of statistics or degrees of freedom as flat float64: a device tensor stays on its device."""
    torch = _torch()
    if isinstance(x, torch.Tensor):
        if x.dtype.is_complex or x.dtype == torch.bool:
            raise ValueError("'%s' should hold numbers" % name)
        return x.reshape(-1)
    try:
        v = np.asarray(x)
        if v.dtype.kind not in "fiu":
            raise TypeError
        return np.ascontiguousarray(v.reshape(-1), np.float64)
    except (TypeError, ValueError):
        raise ValueError("'%s' should hold numbers" % name)


def _dist_tail(kind, x, df, names, as_device):
    """epi_dist_tail_dev over x and df (df of x's length or one value)."""
    x, df = _tail_values(x, names[0]), _tail_values(df, names[1])
    n = int(x.shape[0])
    if int(df.shape[0]) not in (1, n):
        raise ValueError("'%s' should be one number or have the length of '%s'" % (names[1], names[0]))
    torch = _torch()
    lib = _lib.load()
    eng, index, dev = _engine_of((x, df))
    x, df = [(v if isinstance(v, torch.Tensor) else torch.from_numpy(v)).to(device=dev, dtype=torch.float64) for v in (x, df)]
    if int(df.shape[0]) != n:
        df = df.expand(n)
    x, df = x.contiguous(), df.contiguous()
    p = torch.empty(n, dtype=torch.float64, device=dev)
    _lib.check(lib.epi_dist_tail_dev(eng, kind, C.c_void_p(x.data_ptr()), C.c_void_p(df.data_ptr()), n, C.c_void_p(p.data_ptr()), _stream(index)))
    return p if as_device else p.cpu().numpy()


def chisqPValues(stat, df, as_device=False):
    """Upper tail probabilities of the chi-square distribution on the GPU (include/epihip.h, epi_dist_tail_dev with
    EPI_DIST_CHISQ): P(X >= stat) with df degrees of freedom, R's pchisq(stat, df, lower.tail = FALSE) -- the p-value of a
    likelihood-ratio statistic such as compareHeterogeneity's g with its df.  stat, df: array-likes or device tensors of
    numbers; df one value or of stat's length, from above 0 to 1e4.  A negative or NaN stat, or a df outside the range, gives
    NaN.  Returns float64, a device tensor with as_device."""
    return _dist_tail(0, stat, df, ("stat", "df"), as_device)


def tTestPValues(t, df, as_device=False):
    """Two-sided tail probabilities of Student's t distribution on the GPU (epi_dist_tail_dev with EPI_DIST_T2):
    P(|T| >= |t|) with df degrees of freedom, R's 2 * pt(-abs(t), df).  t of either sign; otherwise as chisqPValues."""
    return _dist_tail(1, t, df, ("t", "df"), as_device)


GROUP_COMPARE_COLUMNS = ("rname", "strand", "pos", "context", "meth_a", "unmeth_a", "meth_b", "unmeth_b", "nsamples_a", "nsamples_b",
                         "beta_a", "beta_b", "delta_beta", "mean_beta_a", "mean_beta_b", "var_a", "var_b", "stat", "df", "phi", "p")
GROUP_TESTS = ("lrt", "lrt_mn", "welch", "fisher")
_GROUP_TEST_CODES = {"fisher": 0, "lrt": 1, "lrt_mn": 2, "welch": 3}                      # EPI_CXG_*
_GROUP_MAX = 32


def _group_min_samples(value, size, name):
    return size if value is None else _whole_number(value, name, 1, size)


def rcpp_cx_compare_groups(reps_a, reps_b, min_coverage=1, min_samples_a=None, min_samples_b=None, test="lrt", as_device=False):
    """Two groups of device cytosine reports (lists of rcpp_cx_report / generateCytosineReport tables with as_device=True)
    against each other per cytosine (include/epihip.h, epi_cx_groups_dev, has the definitions): a sample counts at a
    cytosine when it covers it min_coverage times, and the cytosines at which min_samples_a samples of a and min_samples_b
    of b count (None: every sample of the group) are reported with GROUP_COMPARE_COLUMNS -- the counts pooled over the
    counting samples, nsamples_a, nsamples_b, the pooled betas and their difference, mean and variance of the samples' betas
    and stat, df, phi, p of `test`: "fisher" (the pooled table), "lrt" (binomial logistic regression, chi-square), "lrt_mn"
    (the same with McCullagh-Nelder overdispersion, F test) or "welch" (t-test on the samples' betas).  1 to 32 reports a
    side, under one sequence dictionary and on one device (else ValueError, before the device is touched).  The Report
    carries the first report's levels and `nsites`, the cytosines at which any sample counts."""
    min_coverage = _whole_number(min_coverage, "min.coverage", 0, 2 ** 31 - 1)
    test = _match_arg(test, GROUP_TESTS, "test")
    reps_a, reps_b = list(reps_a), list(reps_b)
    for reps, name in ((reps_a, "reps_a"), (reps_b, "reps_b")):
        if not 1 <= len(reps) <= _GROUP_MAX:
            raise ValueError("'%s' should hold 1 to %d reports" % (name, _GROUP_MAX))
    min_samples_a = _group_min_samples(min_samples_a, len(reps_a), "min.samples.a")
    min_samples_b = _group_min_samples(min_samples_b, len(reps_b), "min.samples.b")
    reps = reps_a + reps_b
    if any(r.levels["rname"] != reps[0].levels["rname"] for r in reps):
        raise ValueError("the reports have different sequence names (levels): their rname codes cannot be compared")
    tabs = [_device_columns(r, CX_COLUMNS, "rcpp_cx_compare_groups") for r in reps]
    dev = tabs[0][0].device
    if any(t[0].device != dev for t in tabs):
        raise ValueError("the reports are on different devices")
    torch = _torch()
    lib = _lib.load()
    nrows = [int(t[0].numel()) for t in tabs]
    cap = sum(nrows) // (min_samples_a + min_samples_b)
    icols, dcols = _table_cols(10, 11, cap, dev)
    nsite, nrow = C.c_int64(0), C.c_int64(0)
    _lib.check(lib.epi_cx_groups_dev(_engine(dev.index), _ptr_array([c for t in tabs for c in t]), (C.c_int64 * len(nrows))(*nrows), len(reps_a),
                                     len(reps_b), min_coverage, min_samples_a, min_samples_b, _GROUP_TEST_CODES[test], _ptr_array(icols),
                                     _ptr_array(dcols), cap, _stream(dev.index), C.byref(nsite), C.byref(nrow)))
    rep = Report(dict(zip(GROUP_COMPARE_COLUMNS, [c[:nrow.value] for c in icols + dcols])), reps[0].levels["rname"])
    rep.nsites = nsite.value
    return _table_to_host(rep, as_device)


P_ADJUST_METHODS = ("holm", "hochberg", "bonferroni", "BH", "BY", "fdr", "none")          # R's p.adjust.methods without hommel
_P_ADJUST_CODES = {"none": 0, "bonferroni": 1, "holm": 2, "hochberg": 3, "BH": 4, "fdr": 4, "BY": 5}   # EPI_PADJ_*


def _p_adjust_args(method, n_tests, name="method"):
    """(EPI_PADJ_* code, n_tests or 0) of a p.adjust method and R's p.adjust(n =)."""
    method = _match_arg(method, P_ADJUST_METHODS, name)
    if n_tests is not None:
        try:
            n_tests = _whole_number(n_tests, "n.tests", 1, 2 ** 31 - 1)
        except (TypeError, OverflowError, ValueError):
            raise ValueError("'n.tests' should be an integer from 1 to %d" % (2 ** 31 - 1))
    return _P_ADJUST_CODES[method], n_tests or 0


def _p_values(p, name):
    """A column of p-values as flat float64: a device tensor stays on its device."""
    torch = _torch()
    if isinstance(p, torch.Tensor):
        if not p.dtype.is_floating_point:
            raise ValueError("'%s' should hold floating-point numbers" % name)
        return p.reshape(-1)
    try:
        v = np.asarray(p)
        if v.dtype.kind not in "fiu":
            raise TypeError
        return np.ascontiguousarray(v.reshape(-1), np.float64)
    except (TypeError, ValueError):
        raise ValueError("'%s' should hold numbers" % name)


def _p_adjust(p, code, n_tests):
    """epi_p_adjust_dev on a flat column (_p_values): q, a device tensor."""
    torch = _torch()
    lib = _lib.load()
    eng, index, dev = _engine_of((p,))
    p = (p if isinstance(p, torch.Tensor) else torch.from_numpy(p)).to(device=dev, dtype=torch.float64).contiguous()
    n = int(p.shape[0])
    q = torch.empty(n, dtype=torch.float64, device=dev)
    m = C.c_int64(0)
    _lib.check(lib.epi_p_adjust_dev(eng, C.c_void_p(p.data_ptr()), n, code, n_tests, C.c_void_p(q.data_ptr()), None, _stream(index),
                                    C.byref(m)))
    return q


def adjustPValues(p, method="BH", n_tests=None, as_device=False):
    """R's p.adjust on the GPU (include/epihip.h, epi_p_adjust_dev): the p-values adjusted for the number of tests by
    `method`, one of "holm", "hochberg", "bonferroni", "BH", "BY", "fdr" (= "BH") and "none"; `hommel` is not built.  p: an
    array-like or a device tensor of floats; NaN is NA, stays NaN and is not counted as a test; any other value outside
    [0, 1] is an error.  n_tests: R's `n`, the number of tests when it is larger than the number of p-values given.
    Returns float64 of p's length, a device tensor with as_device."""
    code, n_tests = _p_adjust_args(method, n_tests)
    q = _p_adjust(_p_values(p, "p"), code, n_tests)
    return q if as_device else q.cpu().numpy()


def adjustReport(report, method="BH", column="p", name="q", n_tests=None):
    """The Report with one more float64 column `name`: its `column` adjusted by adjustPValues over the table's rows -- a
    device tensor when `column` is one, else numpy.  For the tables of compareCytosineReports and generateDmrReport (p)
    and of generateVcfReport ("FEp+", "FEp-").  Levels and attributes such as `ncommon` are kept."""
    code, n_tests = _p_adjust_args(method, n_tests)
    if not isinstance(report, Report) or not isinstance(column, str) or column not in report:
        raise ValueError("'report' should be a Report with the column %r" % (column,))
    if not isinstance(name, str) or not name or name in report:
        raise ValueError("'name' should be the name of a column the report does not have yet")
    p = _p_values(report[column], column)
    on_device = hasattr(report[column], "is_cuda")
    q = _p_adjust(p, code, n_tests)
    out = Report(dict(report), report.levels["rname"])
    out.__dict__.update({k: v for k, v in report.__dict__.items() if k != "levels"})
    out.levels = dict(report.levels)
    out[name] = q if on_device else q.cpu().numpy()
    return out


PATTERN_LEVELS = ("NA1", "H", "A", "C", "NA5", "X", "Z", "NA8", "NA9", "h", "G", "T", "N", "x", "z", "NA16")   # :192-195
NA_INTEGER = -2 ** 31


def rcpp_extract_patterns(df, target_rname, target_start, target_end, min_overlap, ctx, min_ctx_freq, clip,
                          reverse_offset, hlght=()):
    """src/rcpp_extract_patterns.cpp:26-211 -> Report with seqnames, strand, start, end, nbase, beta, pattern (16 hex
    digits) and one int32 column per position (context / base factor codes, levels PATTERN_LEVELS, NA = -2^31), or an
    empty Report when no pattern was found."""
    lib = _lib.load()
    bam = _as_bam(df)
    b = bam.batch()
    hl = np.ascontiguousarray(hlght, dtype=np.int32)
    t = _lib.PatternTable()
    _lib.check(lib.epi_batch_extract_patterns(b, int(target_rname), int(target_start), int(target_end), int(min_overlap),
                                              _lib.enc(ctx), float(min_ctx_freq), int(bool(clip)), int(reverse_offset),
                                              C.c_void_p(hl.ctypes.data) if hl.size else None, int(hl.size),
                                              _stream(bam.device), C.byref(t)))
    try:
        return _pattern_report(t, target_rname, bam)
    finally:
        lib.epi_pattern_table_free(C.byref(t))


def _pattern_report(t, target_rname, bam):
    """An epi_pattern_table (still owned by the library) -> Report."""
    k, m = int(t.npat), int(t.ncol)
    if k == 0:
        return Report({}, bam.levels)
    take = lambda ptr, n, dt: np.ctypeslib.as_array(ptr, shape=(n,)).astype(dt, copy=True)
    cols = {"seqnames": np.full(k, int(target_rname), np.int32)}
    for nm in ("strand", "start", "end", "nbase"):
        cols[nm] = take(getattr(t, nm), k, np.int32)
    cols["beta"] = take(t.beta, k, np.float64)
    cols["pattern"] = np.asarray(["%016X" % int(v) for v in take(t.fnv, k, np.uint64)], object)      # :174-176
    pos = take(t.positions, m, np.int32)
    cells = take(t.cells, m * k, np.int32).reshape(m, k)
    for i in range(m):
        cols[str(int(pos[i]))] = cells[i]
    rep = Report(cols, bam.levels)
    rep.pattern_levels = PATTERN_LEVELS
    return rep


def _patterns_multi(df, targets, hlght, fn_name, table_type, free_name, report, scalars):
    """The call both multi-target entry points share: targets as [3][nt] int32, highlight positions as CSR, one
    library-owned table per target turned into a Report by report(table, k) and released."""
    lib = _lib.load()
    bam = _as_bam(df)
    tg = np.ascontiguousarray(np.asarray(list(targets), dtype=np.int64).reshape(-1, 3).T, dtype=np.int32)    # [3][nt]
    nt = tg.shape[1]
    if hlght is not None and len(hlght) != nt:
        raise ValueError("hlght must hold one sequence of positions per target")
    b = bam.batch()
    hl_off = np.zeros(nt + 1, np.int64)
    if hlght is not None:
        np.cumsum([len(h) for h in hlght], out=hl_off[1:])
    hl = np.ascontiguousarray([p for h in hlght for p in h] if hlght is not None else [], dtype=np.int32)
    tabs = (table_type * max(nt, 1))()
    ptr = lambda a: C.c_void_p(a.ctypes.data) if a.size else None
    min_overlap, ctx, min_ctx_freq, clip, reverse_offset = scalars
    _lib.check(getattr(lib, fn_name)(b, nt, ptr(tg[0]), ptr(tg[1]), ptr(tg[2]), int(min_overlap), _lib.enc(ctx), float(min_ctx_freq),
                                     int(bool(clip)), int(reverse_offset), ptr(hl),
                                     C.c_void_p(hl_off.ctypes.data) if hlght is not None else None, _stream(bam.device), tabs))
    try:
        return [report(tabs[k], tg[0, k], bam) for k in range(nt)]
    finally:
        for k in range(nt):
            getattr(lib, free_name)(C.byref(tabs[k]))


def rcpp_extract_patterns_multi(df, targets, min_overlap, ctx, min_ctx_freq, clip, reverse_offset, hlght=None):
    """rcpp_extract_patterns for every target of a list in one pass over the candidate rows
    (epi_batch_extract_patterns_multi).  targets: a sequence of (rname_code, start, end); hlght: None, or one sequence
    of highlight positions per target (sorted, unique, inside the target).  Returns one Report per target, each what
    rcpp_extract_patterns(df, *targets[k], ..., hlght[k]) returns."""
    return _patterns_multi(df, targets, hlght, "epi_batch_extract_patterns_multi", _lib.PatternTable, "epi_pattern_table_free",
                           _pattern_report, (min_overlap, ctx, min_ctx_freq, clip, reverse_offset))


def _summary_report(t, bam, beta_letters=None):
    """An epi_pattern_summary (still owned by the library) -> Report: pattern, one column per position, count, and with
    beta_letters = (ctx_meth, ctx_unmeth) beta: per row meth / (meth + unmeth) over its cells, 0 without either, where the
    cells that count are the factor codes of those letters and an NA cell counts in neither (R/plotPatterns.R:174-184)."""
    k, m = int(t.nuniq), int(t.ncol)
    if k == 0:
        return Report({}, bam.levels)
    take = lambda ptr, n, dt: np.ctypeslib.as_array(ptr, shape=(n,)).astype(dt, copy=True)
    cols = {"pattern": np.asarray(["%016X" % int(v) for v in take(t.fnv, k, np.uint64)], object)}
    pos = take(t.positions, m, np.int32)
    cells = take(t.cells, m * k, np.int32).reshape(m, k)
    for i in range(m):
        cols[str(int(pos[i]))] = cells[i]
    cols["count"] = take(t.count, k, np.int32)
    if beta_letters is not None:
        lut = np.zeros((2, len(PATTERN_LEVELS) + 1), np.int64)                 # [meth, unmeth][factor code]; NA -> code 0
        for row, letters in zip(lut, beta_letters):
            row[[PATTERN_LEVELS.index(ch) + 1 for ch in letters]] = 1
        code = np.clip(cells, 0, len(PATTERN_LEVELS))
        meth = lut[0][code].sum(axis=0).astype(np.float64)
        total = meth + lut[1][code].sum(axis=0).astype(np.float64)
        cols["beta"] = np.divide(meth, total, out=np.zeros(k, np.float64), where=total > 0)
    rep = Report(cols, bam.levels)
    rep.pattern_levels = PATTERN_LEVELS
    return rep


def rcpp_summarise_patterns_multi(df, targets, min_overlap, ctx, min_ctx_freq, clip, reverse_offset, hlght=None, beta_letters=None):
    """The unique rows, by (pattern, every position column), of what rcpp_extract_patterns returns for every target of a
    list, with their counts and in the order of their first appearance -- grouped on the GPU, so that nothing per read
    comes to the host (epi_batch_summarise_patterns_multi).  Arguments as rcpp_extract_patterns_multi.  Returns one
    Report per target: pattern (16 hex digits), one int32 column per position, count (int32), and with beta_letters =
    (ctx_meth, ctx_unmeth) beta (float64, computed here from the cells)."""
    return _patterns_multi(df, targets, hlght, "epi_batch_summarise_patterns_multi", _lib.PatternSummary, "epi_pattern_summary_free",
                           lambda t, _, bam: _summary_report(t, bam, beta_letters), (min_overlap, ctx, min_ctx_freq, clip, reverse_offset))


# ---- exported R API ------------------------------------------------------------------------------

def _deliver(rep, report_file, gzip, as_device=True):
    """The end of every report function: the report itself (a device table comes to the host unless as_device), or with a
    report_file the report written there and None."""
    if report_file is None:
        return _table_to_host(rep, as_device)
    writeReport(rep, report_file, gzip)
    return None


def _match_arg(value, choices, name):
    if value is None:
        return choices[0]                       # match.arg: first choice is the default
    if value not in choices:
        raise ValueError("'%s' should be one of %s" % (name, ", ".join(repr(c) for c in choices)))
    return value


_CTX_CHOICES = ("CG", "CHG", "CHH", "CxG", "CX")


def generateCytosineReport(bam, report_file=None, threshold_reads=True, threshold_context=None,
                           min_context_sites=2, min_context_beta=0.5, max_outofcontext_beta=0.1,
                           report_context=None, gzip=False, verbose=False, as_device=False, **preprocess_args):
    """R/generateCytosineReport.R:164-208."""
    threshold_context = _match_arg(threshold_context, _CTX_CHOICES, "threshold.context")
    report_context = threshold_context if report_context is None else _match_arg(report_context, _CTX_CHOICES, "report.context")
    bam = preprocessBam(bam, **preprocess_args)
    if threshold_reads:
        c = CONTEXT_TO_BASES[threshold_context]   # .thresholdReads + .getCytosineReport (:181-199) in one pass over the bytes
        rep = cytosine_report_fused(bam, c["ctx_meth"], c["ctx_unmeth"], c["ooctx_meth"], c["ooctx_unmeth"],
                                    min_context_sites, min_context_beta, max_outofcontext_beta,
                                    CONTEXT_TO_BASES[report_context]["ctx_meth"], as_device=as_device)
    else:                                       # pass <- rep(TRUE, nrow(bam)), :193-195
        rep = rcpp_cx_report(bam, None, CONTEXT_TO_BASES[report_context]["ctx_meth"], as_device=as_device)
    return _deliver(rep, report_file, gzip)


def generateMhlReport(bam, report_file=None, haplotype_context=None, max_haplotype_window=0,
                      min_haplotype_length=0, max_outofcontext_beta=0.1, gzip=False, verbose=False,
                      as_device=False, **preprocess_args):
    """R/generateMhlReport.R:170-197."""
    haplotype_context = _match_arg(haplotype_context, _CTX_CHOICES, "haplotype.context")
    bam = preprocessBam(bam, **preprocess_args)
    c = CONTEXT_TO_BASES[haplotype_context]
    rep = rcpp_mhl_report(bam, c["ctx_meth"] + c["ctx_unmeth"], max_haplotype_window, min_haplotype_length,
                          max_outofcontext_beta, as_device=as_device)
    return _deliver(rep, report_file, gzip)


def generateHeterogeneityReport(bam, report_file=None, window_context=None, window_sites=4, min_reads=1, max_window_span=0,
                                max_outofcontext_beta=0.1, gzip=False, verbose=False, as_device=False, **preprocess_args):
    """Within-sample heterogeneity per window of `window_sites` (2 to 6) neighbouring cytosines of `window_context`:
    epipolymorphism, methylation entropy and the fraction of discordant reads, with the window's read count, pattern
    count and beta.  The sites are those of generateCytosineReport(threshold_reads=False, report_context=window_context),
    the reads those generateMhlReport keeps under max_outofcontext_beta; windows with fewer than min_reads reads, or
    (max_window_span > 0) spanning more than max_window_span bases, are left out.  The reference has no such report."""
    window_context = _match_arg(window_context, _CTX_CHOICES, "window.context")
    window_sites = _whole_number(window_sites, "window.sites", 2, 6)
    bam = preprocessBam(bam, **preprocess_args)
    c = CONTEXT_TO_BASES[window_context]
    rep = rcpp_heterogeneity_report(bam, c["ctx_meth"] + c["ctx_unmeth"], window_sites, max_outofcontext_beta,
                                    min_reads, max_window_span, as_device=as_device)
    return _deliver(rep, report_file, gzip)


def compareHeterogeneity(bam_a, bam_b, report_file=None, window_context=None, window_sites=4, min_reads=1, max_window_span=0,
                         max_outofcontext_beta=0.1, gzip=False, verbose=False, as_device=False, **preprocess_args):
    """Two samples against each other per window of `window_sites` (2 to 6) neighbouring cytosines of `window_context`
    that the cytosine reports of BOTH have (generateCytosineReport(threshold_reads=False, report_context=window_context);
    same position, strand and context): what generateHeterogeneityReport gives for either sample on these windows
    (columns *_a, *_b), delta_beta and delta_entropy (b minus a), the Jensen-Shannon divergence of the two epiallele
    histograms in bits (jsd), their total variation distance (tvd) and the likelihood-ratio statistic g of the 2 x 2^k
    table with its degrees of freedom df (chisqPValues(g, df) gives its p-value).  Windows with fewer than min_reads reads in either
    sample, or (max_window_span > 0) spanning more than max_window_span bases, are left out.  Both inputs go through
    preprocessBam with the same preprocess_args and must have the same sequence names.  The Report's `ncommon` is the
    number of common sites.  The reference has no such report."""
    window_context = _match_arg(window_context, _CTX_CHOICES, "window.context")
    window_sites = _whole_number(window_sites, "window.sites", 2, 6)
    bam_a = preprocessBam(bam_a, **preprocess_args)
    bam_b = preprocessBam(bam_b, **preprocess_args)
    c = CONTEXT_TO_BASES[window_context]
    rep = rcpp_heterogeneity_compare(bam_a, bam_b, c["ctx_meth"] + c["ctx_unmeth"], window_sites, max_outofcontext_beta,
                                     min_reads, max_window_span, as_device=as_device)
    return _deliver(rep, report_file, gzip)


def _whole_number(value, name, lo, hi=None):
    if isinstance(value, bool) or int(value) != value or int(value) < lo or (hi is not None and int(value) > hi):
        raise ValueError("'%s' should be an integer %s" % (name, "from %d to %d" % (lo, hi) if hi is not None else "of at least %d" % lo))
    return int(value)


def _linkage_args(linkage_context, max_neighbours, max_distance):
    return (_match_arg(linkage_context, _CTX_CHOICES, "linkage.context"), _whole_number(max_neighbours, "max.neighbours", 1, 16),
            _whole_number(max_distance, "max.distance", 0))


def generateLinkageReport(bam, report_file=None, linkage_context=None, max_neighbours=4, max_distance=0, min_reads=1,
                          max_outofcontext_beta=0.1, gzip=False, verbose=False, as_device=False, **preprocess_args):
    """Co-methylation of every cytosine of `linkage_context` with each of its next `max_neighbours` (1 to 16) neighbours on
    the same sequence and strand, over the reads that have a call at both: the 2 x 2 table (n_uu, n_mu, n_um, n_mm; the
    first letter is the first site's state), its covariance, r2 and D'.  The sites are those of
    generateCytosineReport(threshold_reads=False, report_context=linkage_context), the reads those generateMhlReport keeps
    under max_outofcontext_beta; pairs with fewer than min_reads reads, or (max_distance > 0) more than max_distance bases
    apart, are left out.  The other half of Guo et al. 2017, where lMHL comes from; the reference has no such report."""
    linkage_context, max_neighbours, max_distance = _linkage_args(linkage_context, max_neighbours, max_distance)
    bam = preprocessBam(bam, **preprocess_args)
    c = CONTEXT_TO_BASES[linkage_context]
    rep = rcpp_linkage_report(bam, c["ctx_meth"] + c["ctx_unmeth"], max_neighbours, max_distance, max_outofcontext_beta,
                              min_reads, as_device=as_device)
    return _deliver(rep, report_file, gzip)


def generateHaplotypeBlocks(bam, report_file=None, linkage_context=None, max_neighbours=4, max_distance=0, min_reads=10,
                            max_outofcontext_beta=0.1, min_r2=0.5, min_sites=3, gzip=False, verbose=False, as_device=False,
                            **preprocess_args):
    """Methylation haplotype blocks: runs of at least `min_sites` neighbouring cytosines in which every site is linked
    (r2 >= min_r2 over at least min_reads reads) to each of the up to `max_neighbours` sites of the block in front of it;
    built greedily from each strand's first site on the pair table of generateLinkageReport with the same arguments
    (include/epihip.h has the rule).  Columns: rname, strand, start, end, nsites, mean_r2 (of the adjacent pairs)."""
    linkage_context, max_neighbours, max_distance = _linkage_args(linkage_context, max_neighbours, max_distance)
    min_sites = _whole_number(min_sites, "min.sites", 2)
    if isinstance(min_r2, bool) or not 0 <= min_r2 <= 1:
        raise ValueError("'min.r2' should be a number from 0 to 1")
    bam = preprocessBam(bam, **preprocess_args)
    c = CONTEXT_TO_BASES[linkage_context]
    rep = rcpp_linkage_blocks(bam, c["ctx_meth"] + c["ctx_unmeth"], max_neighbours, max_distance, max_outofcontext_beta,
                              min_reads, min_r2, min_sites, as_device=as_device)
    return _deliver(rep, report_file, gzip)


def generateFdrpReport(bam, report_file=None, fdrp_context=None, flank_sites=8, max_reads=40, min_overlap=1, max_distance=0,
                       min_reads=2, max_outofcontext_beta=0.1, gzip=False, verbose=False, as_device=False, **preprocess_args):
    """FDRP and qFDRP (Scherer et al. 2020, the WSH package) per cytosine of `fdrp_context`: over the pairs of reads that
    have a call at the cytosine, the fraction of pairs whose calls differ anywhere in the window of `flank_sites` (0 to 31)
    cytosines on either side (fdrp), and the mean over the pairs of the share of differing calls among the window's
    cytosines both reads call (qfdrp).  A pair counts when both reads call at least `min_overlap` cytosines of the window;
    with max_distance > 0 the window holds only cytosines within that many bases.  At most `max_reads` (2 to 64; WSH's
    sample size of 40 by default) reads per cytosine are compared: those at evenly spaced ranks of the covering reads,
    not a random draw as in WSH -- and over a window of cytosines, not over the reads' whole overlap.  The sites are those of
    generateCytosineReport(threshold_reads=False, report_context=fdrp_context), the reads those generateMhlReport keeps
    under max_outofcontext_beta; cytosines with fewer than max(min_reads, 2) compared reads or without a counted pair are
    left out.  Columns: rname, strand, pos, context, coverage, nreads, npairs, ndiscordant, fdrp, qfdrp
    (include/epihip.h has the definitions).  The reference has no such report."""
    fdrp_context = _match_arg(fdrp_context, _CTX_CHOICES, "fdrp.context")
    flank_sites = _whole_number(flank_sites, "flank.sites", 0, 31)
    max_reads = _whole_number(max_reads, "max.reads", 2, 64)
    min_overlap = _whole_number(min_overlap, "min.overlap", 1, 2 * flank_sites + 1)
    max_distance = _whole_number(max_distance, "max.distance", 0)
    bam = preprocessBam(bam, **preprocess_args)
    c = CONTEXT_TO_BASES[fdrp_context]
    rep = rcpp_fdrp_report(bam, c["ctx_meth"] + c["ctx_unmeth"], flank_sites, max_reads, min_overlap, max_distance,
                           max_outofcontext_beta, min_reads, as_device=as_device)
    return _deliver(rep, report_file, gzip)


def _context_codes(context):
    """The context codes (2 = CHH, 6 = CHG, 7 = CG) of one of _CTX_CHOICES"""
    return [((ord(ch) + 2) >> 2) & 7 for ch in CONTEXT_TO_BASES[context]["ctx_meth"]]


def generateMbiasReport(bam, report_file=None, report_context="CX", max_offset=150, gzip=False, verbose=False, as_device=False,
                        **preprocess_args):
    """M-bias table: methylation as a function of the offset from either end of the template, per strand and context -- the
    quality-control table that tells how many end bases to pass as preprocessBam(trim=) (suggestTrim reads it off).  Every
    template counts as it is packed: no thresholding, no read rule.  One row per end ("start": offset 0 is the template's
    first base; "end": offset 0 is its last), strand, context of `report_context` and offset 0 .. max_offset - 1 (1 to 1024
    offsets), rows without calls included: meth, unmeth and beta = meth / (meth + unmeth).  Offsets are template
    coordinates, the filler between mates included, so trim = (t5, t3) removes exactly the offsets < t5 of "start" and < t3
    of "end".  The Report's `totals` gives meth, unmeth and beta per strand and context over ALL bases, whatever max_offset
    is: its CHG and CHH rows are the usual estimate of incomplete bisulfite conversion.  The kernel counts every context;
    report_context only selects the rows.  The reference has no such report."""
    report_context = _match_arg(report_context, _CTX_CHOICES, "report.context")
    max_offset = _whole_number(max_offset, "max.offset", 1, _MBIAS_MAX_OFFSET)
    bam = preprocessBam(bam, **preprocess_args)
    rep = rcpp_mbias_report(bam, max_offset, as_device=as_device)
    if report_context != "CX":
        rep = _mbias_select(rep, _context_codes(report_context))
    return _deliver(rep, report_file, gzip)


def suggestTrim(report, context="CG", max_delta=0.05, min_calls=100, run=3):
    """(trim5, trim3) for preprocessBam(trim=) from an M-bias report (generateMbiasReport): per end, the number of leading
    offsets to cut so that the next `run` offsets all conform to the plateau.  Per end the two strands of `context` are
    pooled; with D0 = max_offset // 2 the plateau is sum_{d >= D0} meth / sum_{d >= D0} (meth + unmeth) (ValueError when no
    call lies there); offset d conforms when it has fewer than min_calls calls or |beta_d - plateau| <= max_delta; the trim
    is the smallest t in [0, D0] such that every d in [t, min(t + run, D0)) conforms.  trim5 comes from the "start" table,
    trim3 from the "end" table.  Which physical ends these are: a paired-end template starts with one mate's 5' end and
    ends with the other mate's 5' end, so both trims cut 5' ends of reads; for single-end rows "start" is the read's 5' end
    on strand '+' and its 3' end on strand '-' (the template is stored in reference direction)."""
    context = _match_arg(context, _CTX_CHOICES, "context")
    run = _whole_number(run, "run", 1)
    cols = {k: (report[k].cpu().numpy() if hasattr(report[k], "cpu") else np.asarray(report[k])) for k in ("end", "context", "offset", "meth", "unmeth")}
    max_offset = int(cols["offset"].max()) + 1 if cols["offset"].size else 0
    d0 = max_offset // 2
    in_ctx = np.isin(cols["context"], _context_codes(context))
    trims = []
    for end in (1, 2):
        keep = in_ctx & (cols["end"] == end)
        meth = np.bincount(cols["offset"][keep], weights=cols["meth"][keep], minlength=max_offset).astype(np.int64)
        calls = meth + np.bincount(cols["offset"][keep], weights=cols["unmeth"][keep], minlength=max_offset).astype(np.int64)
        if calls[d0:].sum() == 0:
            raise ValueError("suggestTrim: the %s table has no %s call at offsets >= %d to take the plateau from"
                             % (MBIAS_END_LEVELS[end - 1], context, d0))
        plateau = np.float64(meth[d0:].sum()) / np.float64(calls[d0:].sum())
        with np.errstate(invalid="ignore", divide="ignore"):
            conforms = (calls < min_calls) | (np.abs(meth.astype(np.float64) / calls.astype(np.float64) - plateau) <= max_delta)
        trims.append(next(t for t in range(d0 + 1) if conforms[t:min(t + run, d0)].all()))
    return tuple(trims)


def _cytosine_comparison(bam_a, bam_b, threshold_reads, threshold_context, min_context_sites, min_context_beta, max_outofcontext_beta,
                         report_context, min_coverage, preprocess_args):
    """The device comparison table of compareCytosineReports; every argument is checked before a file is opened."""
    threshold_context = _match_arg(threshold_context, _CTX_CHOICES, "threshold.context")
    report_context = threshold_context if report_context is None else _match_arg(report_context, _CTX_CHOICES, "report.context")
    min_coverage = _whole_number(min_coverage, "min.coverage", 0, 2 ** 31 - 1)
    bam_a = preprocessBam(bam_a, **preprocess_args)
    bam_b = preprocessBam(bam_b, **preprocess_args)
    _batch_pair(bam_a, bam_b)
    reps = [generateCytosineReport(bam, None, threshold_reads, threshold_context, min_context_sites, min_context_beta,
                                   max_outofcontext_beta, report_context, as_device=True) for bam in (bam_a, bam_b)]
    return rcpp_cx_compare(reps[0], reps[1], min_coverage, as_device=True)


def compareCytosineReports(bam_a, bam_b, report_file=None, threshold_reads=True, threshold_context=None, min_context_sites=2,
                           min_context_beta=0.5, max_outofcontext_beta=0.1, report_context=None, min_coverage=1, gzip=False,
                           verbose=False, as_device=False, **preprocess_args):
    """Two samples against each other per cytosine: the tables generateCytosineReport gives for either input with these
    arguments, joined on the device over the cytosines both have (same position, strand and context) and that are covered
    at least min_coverage times in either.  Columns: rname, strand, pos, context, meth_a, unmeth_a, meth_b, unmeth_b,
    beta_a, beta_b, delta_beta (b minus a) and p, the two-sided Fisher exact p-value of (meth_a unmeth_a / meth_b unmeth_b);
    no p-value is adjusted for the number of tests (adjustReport does that).  Both inputs go through preprocessBam with the same preprocess_args
    and must have the same sequence names.  The Report's `ncommon` is the number of common cytosines.  The reference has
    no such report."""
    rep = _cytosine_comparison(bam_a, bam_b, threshold_reads, threshold_context, min_context_sites, min_context_beta,
                               max_outofcontext_beta, report_context, min_coverage, preprocess_args)
    return _deliver(rep, report_file, gzip, as_device)


def generateSmoothedReport(bam, report_file=None, threshold_reads=True, threshold_context=None, min_context_sites=2,
                           min_context_beta=0.5, max_outofcontext_beta=0.1, report_context=None, merge_strands=True, bandwidth=1000,
                           min_sites=70, max_gap=10 ** 8, degree=2, gzip=False, verbose=False, as_device=False, **preprocess_args):
    """The smoothed cytosine report of one sample: the table generateCytosineReport gives with these arguments, on the
    device, its CpG strands merged (mergeCpgStrands) when merge_strands is set, then smoothed (smoothCytosineReport has the
    columns and the meaning of bandwidth, min_sites, max_gap and degree).  Every argument is checked before a file is
    opened.  The Report carries `ncluster`, `max_window` and, when merged, `nmerged`, `nmoved`, `nkept`.  The reference has
    no such report."""
    threshold_context = _match_arg(threshold_context, _CTX_CHOICES, "threshold.context")
    report_context = threshold_context if report_context is None else _match_arg(report_context, _CTX_CHOICES, "report.context")
    if not isinstance(merge_strands, (bool, np.bool_)):
        raise ValueError("'merge.strands' should be TRUE or FALSE")
    args = _smooth_args(bandwidth, min_sites, max_gap, degree)
    bam = preprocessBam(bam, **preprocess_args)
    rep = generateCytosineReport(bam, None, threshold_reads, threshold_context, min_context_sites, min_context_beta,
                                 max_outofcontext_beta, report_context, as_device=True)
    counts = {}
    if merge_strands:
        rep = rcpp_cx_merge_strands(rep, as_device=True)
        counts = dict(nmerged=rep.nmerged, nmoved=rep.nmoved, nkept=rep.nkept)
    rep = rcpp_cx_smooth(rep, *args, as_device=True)
    rep.__dict__.update(counts)
    return _deliver(rep, report_file, gzip, as_device)


def generateSegmentReport(bam, report_file=None, threshold_reads=True, threshold_context=None, min_context_sites=2,
                          min_context_beta=0.5, max_outofcontext_beta=0.1, report_context=None, merge_strands=True,
                          state_beta=(0.1, 0.5, 0.9), stay=0.99, max_gap=5000, max_coverage=1000, max_iter=10, gzip=False, verbose=False,
                          as_device=False, **preprocess_args):
    """The methylation segments of one sample: the table generateCytosineReport gives with these arguments, on the device,
    its CpG strands merged (mergeCpgStrands) when merge_strands is set, then segmented (segmentCytosineReport has the model
    and the meaning of state_beta, stay, max_gap, max_coverage and max_iter).  The report is the SEGMENT table (rname,
    strand, context, start, end, state, nsites, meth, unmeth, beta), which generateRegionReport and extractPatternsBed take
    as regions.  Every argument is checked before a file is opened.  The Report carries `sites` (the per-cytosine table
    with `state`), `fit`, `nchain`, `nsegment` and, when merged, `nmerged`, `nmoved`, `nkept`.  The reference has no such
    report."""
    threshold_context = _match_arg(threshold_context, _CTX_CHOICES, "threshold.context")
    report_context = threshold_context if report_context is None else _match_arg(report_context, _CTX_CHOICES, "report.context")
    if not isinstance(merge_strands, (bool, np.bool_)):
        raise ValueError("'merge.strands' should be TRUE or FALSE")
    p, trans, init = _segment_start(state_beta, stay)
    args = _segment_args(max_gap, max_coverage, max_iter)
    bam = preprocessBam(bam, **preprocess_args)
    rep = generateCytosineReport(bam, None, threshold_reads, threshold_context, min_context_sites, min_context_beta,
                                 max_outofcontext_beta, report_context, as_device=True)
    counts = {}
    if merge_strands:
        rep = rcpp_cx_merge_strands(rep, as_device=True)
        counts = dict(nmerged=rep.nmerged, nmoved=rep.nmoved, nkept=rep.nkept)
    sites = rcpp_cx_segment(rep, p, trans, init, *args, as_device=True)
    seg = sites.segments
    del sites.segments
    seg.sites = _table_to_host(sites, as_device)
    seg.fit, seg.nchain, seg.nsegment = sites.fit, sites.nchain, sites.nsegment
    seg.__dict__.update(counts)
    return _deliver(seg, report_file, gzip, as_device)


def generateDmrReport(bam_a, bam_b, report_file=None, threshold_reads=True, threshold_context=None, min_context_sites=2,
                      min_context_beta=0.5, max_outofcontext_beta=0.1, report_context=None, min_coverage=1, gzip=False,
                      verbose=False, as_device=False, max_p=0.05, min_delta_beta=0.1, max_gap=500, min_sites=3, **preprocess_args):
    """Differentially methylated regions between two samples: the comparison of compareCytosineReports with the same
    arguments, and of its rows the maximal runs of at least `min_sites` consecutive cytosines (both strands, in table
    order) with p <= max_p and |delta_beta| >= min_delta_beta that change in one direction, lie on one sequence and whose
    neighbours are at most `max_gap` bases apart.  Columns: rname, start, end, nsites, direction (+1: b above a, -1),
    beta_a, beta_b and delta_beta of the region's pooled counts, mean_delta_beta of its cytosines and p, the Fisher exact
    p-value of the pooled table.  The Report's `ncommon` is the number of common cytosines."""
    args = _region_args(max_p, min_delta_beta, max_gap, min_sites)
    cmp_ = _cytosine_comparison(bam_a, bam_b, threshold_reads, threshold_context, min_context_sites, min_context_beta,
                                max_outofcontext_beta, report_context, min_coverage, preprocess_args)
    rep = rcpp_cx_compare_regions(cmp_, *args, as_device=True)
    rep.ncommon = cmp_.ncommon
    return _deliver(rep, report_file, gzip, as_device)


def generateAdjustedDmrReport(bam_a, bam_b, report_file=None, threshold_reads=True, threshold_context=None, min_context_sites=2,
                              min_context_beta=0.5, max_outofcontext_beta=0.1, report_context=None, min_coverage=1, gzip=False,
                              verbose=False, as_device=False, max_q=0.05, min_delta_beta=0.1, max_gap=500, min_sites=3,
                              p_adjust="BH", **preprocess_args):
    """generateDmrReport on adjusted p-values: the comparison of compareCytosineReports with the same arguments, its p
    adjusted over its rows by `p_adjust` (adjustPValues' methods) into q, and the regions of generateDmrReport formed on
    q <= max_q.  Columns: generateDmrReport's, and q: the regions' pooled p adjusted over the reported regions by the same
    method.  The Report's `ncommon` is the number of common cytosines."""
    args = _region_args(max_q, min_delta_beta, max_gap, min_sites, "max.q")
    _p_adjust_args(p_adjust, None, "p.adjust")
    cmp_ = _cytosine_comparison(bam_a, bam_b, threshold_reads, threshold_context, min_context_sites, min_context_beta,
                                max_outofcontext_beta, report_context, min_coverage, preprocess_args)
    rep = rcpp_cx_compare_regions(adjustReport(cmp_, p_adjust), *args, as_device=True, significance="q")
    rep = adjustReport(rep, p_adjust)
    rep.ncommon = cmp_.ncommon
    return _deliver(rep, report_file, gzip, as_device)


def _group_comparison(bams_a, bams_b, threshold_reads, threshold_context, min_context_sites, min_context_beta, max_outofcontext_beta,
                      report_context, min_coverage, min_samples, test, preprocess_args):
    """The device table of compareCytosineGroups; every argument is checked before a file is opened."""
    threshold_context = _match_arg(threshold_context, _CTX_CHOICES, "threshold.context")
    report_context = threshold_context if report_context is None else _match_arg(report_context, _CTX_CHOICES, "report.context")
    min_coverage = _whole_number(min_coverage, "min.coverage", 0, 2 ** 31 - 1)
    test = _match_arg(test, GROUP_TESTS, "test")
    if isinstance(bams_a, (str, bytes, ProcessedBam, dict)) or isinstance(bams_b, (str, bytes, ProcessedBam, dict)):
        raise ValueError("'bams.a' and 'bams.b' should be lists of 1 to %d inputs" % _GROUP_MAX)
    bams_a, bams_b = list(bams_a), list(bams_b)
    for bams, name in ((bams_a, "bams.a"), (bams_b, "bams.b")):
        if not 1 <= len(bams) <= _GROUP_MAX:
            raise ValueError("'%s' should be a list of 1 to %d inputs" % (name, _GROUP_MAX))
    if min_samples is None or isinstance(min_samples, (int, float, np.integer, np.floating)):
        min_samples = (min_samples, min_samples)
    if len(min_samples) != 2:
        raise ValueError("'min.samples' should be an integer or a pair of integers")
    min_a = _group_min_samples(min_samples[0], len(bams_a), "min.samples")
    min_b = _group_min_samples(min_samples[1], len(bams_b), "min.samples")
    given = [b for b in bams_a + bams_b if isinstance(b, ProcessedBam)]
    if any(b.levels != given[0].levels for b in given):
        raise ValueError("the inputs have different sequence names (levels): their rname codes cannot be compared")
    reps = []
    for bam in bams_a + bams_b:                       # one batch at a time: only the samples' device tables stay
        pb = preprocessBam(bam, **preprocess_args)
        if reps and pb.levels != reps[0].levels["rname"]:
            raise ValueError("the inputs have different sequence names (levels): their rname codes cannot be compared")
        reps.append(generateCytosineReport(pb, None, threshold_reads, threshold_context, min_context_sites, min_context_beta,
                                           max_outofcontext_beta, report_context, as_device=True))
        if pb is not bam:
            pb.close()
    return rcpp_cx_compare_groups(reps[:len(bams_a)], reps[len(bams_a):], min_coverage, min_a, min_b, test, as_device=True)


def compareCytosineGroups(bams_a, bams_b, report_file=None, threshold_reads=True, threshold_context=None, min_context_sites=2,
                          min_context_beta=0.5, max_outofcontext_beta=0.1, report_context=None, min_coverage=1, min_samples=None,
                          test="lrt", gzip=False, verbose=False, as_device=False, **preprocess_args):
    """Two groups of samples (replicates) against each other per cytosine: the tables generateCytosineReport gives for every
    input with these arguments, joined on the device.  A sample counts at a cytosine (same position, strand and context)
    when it covers it at least min_coverage times; cytosines at which at least min_samples samples of either group count (an
    integer or a pair for a and b; None: every sample) are reported.  Columns: GROUP_COMPARE_COLUMNS -- rname, strand, pos,
    context, the counts pooled over the counting samples (meth_a, unmeth_a, meth_b, unmeth_b), nsamples_a, nsamples_b,
    beta_a, beta_b and delta_beta (b minus a) of the pooled counts, mean_beta_* and var_* of the samples' betas, and stat,
    df, phi, p of `test`: "lrt", the likelihood-ratio test of the two-group binomial logistic regression (chi-square, 1 df);
    "lrt_mn", the same deviance divided by the McCullagh-Nelder overdispersion phi, F test with nsamples - 2 df (the idea
    of methylKit's overdispersion = "MN", test = "F"; parity with it is not claimed); "welch", Welch's t-test on the
    samples' betas; "fisher", the Fisher exact test of the pooled table, which takes replicate spread for signal (with one
    sample a side it is compareCytosineReports).  No p-value is adjusted for the number of tests (adjustReport does that).
    Inputs: 1 to 32 a side, paths or preprocessBam results under one sequence dictionary; an input given as a path is read,
    reported and its batch dropped before the next is read.  The Report's `nsites` is the number of cytosines at which any
    sample counts.  The reference has no such report."""
    rep = _group_comparison(bams_a, bams_b, threshold_reads, threshold_context, min_context_sites, min_context_beta,
                            max_outofcontext_beta, report_context, min_coverage, min_samples, test, preprocess_args)
    return _deliver(rep, report_file, gzip, as_device)


def generateGroupDmrReport(bams_a, bams_b, report_file=None, threshold_reads=True, threshold_context=None, min_context_sites=2,
                           min_context_beta=0.5, max_outofcontext_beta=0.1, report_context=None, min_coverage=1, min_samples=None,
                           test="lrt", gzip=False, verbose=False, as_device=False, max_q=0.05, min_delta_beta=0.1, max_gap=500,
                           min_sites=3, p_adjust="BH", **preprocess_args):
    """Differentially methylated regions between two groups of samples, by generateAdjustedDmrReport's sequence: the
    table of compareCytosineGroups with the same arguments, its p adjusted over its rows by `p_adjust` into q, the regions
    of generateDmrReport formed on q <= max_q and |delta_beta| >= min_delta_beta of the pooled betas, and the regions' p
    adjusted over the reported regions into q.  The regions' own p stays the Fisher exact test of the region's pooled
    counts, whatever `test` is: a replicate-aware regional test is not built.  Columns: generateAdjustedDmrReport's.  The
    Report's `nsites` is compareCytosineGroups'."""
    args = _region_args(max_q, min_delta_beta, max_gap, min_sites, "max.q")
    _p_adjust_args(p_adjust, None, "p.adjust")
    cmp_ = _group_comparison(bams_a, bams_b, threshold_reads, threshold_context, min_context_sites, min_context_beta,
                             max_outofcontext_beta, report_context, min_coverage, min_samples, test, preprocess_args)
    rep = rcpp_cx_compare_regions(adjustReport(cmp_, p_adjust), *args, as_device=True, significance="q")
    rep = adjustReport(rep, p_adjust)
    rep.nsites = cmp_.nsites
    return _deliver(rep, report_file, gzip, as_device)


def writeReport(report, report_file, gzip=False, nthreads=None):
    """R/internal.R:274-287 (.writeReport): TSV with header, factors written as their labels, NA / NaN as empty
    fields -- data.table::fwrite's conventions.  Numeric and factor columns go through the library's threaded writer
    (epi_write_report); a table with a text column (extractPatterns' hash) is written row by row here."""
    import os
    cols, keep = [], []
    n = report.nrow
    text_cols = False
    for k, v in report.items():
        a = v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)
        lev = report.levels.get(k)
        if a.dtype.kind == "f":
            a = np.ascontiguousarray(a, np.float64)
            cols.append((k, 1, a, None))
        elif a.dtype.kind in "iub":
            a = np.ascontiguousarray(a, np.int32)
            cols.append((k, 2 if lev is not None else 0, a, lev))
        else:
            text_cols = True
            cols.append((k, -1, a, lev))
    if text_cols or not cols:
        _write_report_py(cols, n, report_file, gzip)
        return
    lib = _lib.load()
    arr = (_lib.ReportColumn * len(cols))()
    for i, (k, kind, a, lev) in enumerate(cols):
        arr[i].name = k.encode()
        arr[i].kind = kind
        arr[i].data = a.ctypes.data if a.size else None
        if lev is not None:
            lv = (C.c_char_p * len(lev))(*[str(x).encode("latin1") for x in lev])
            keep.append(lv)
            arr[i].levels = lv
            arr[i].nlevels = len(lev)
        keep.append(a)
    if nthreads is None:
        nthreads = min(os.cpu_count() or 1, 16)
    rc = lib.epi_write_report(os.path.expanduser(str(report_file)).encode(), arr, len(cols), n, int(bool(gzip)), int(nthreads))
    if rc != _lib.EPI_OK:
        raise OSError(lib.epi_last_error().decode("utf-8", "replace"))


def _write_report_py(cols, n, report_file, gzip):
    opener = (lambda p: _gzip.open(p, "wt")) if gzip else (lambda p: open(p, "w"))

    def cell(kind, a, lev, i):
        v = a[i]
        if kind == 1:
            return "" if np.isnan(v) else ("%.15g" % v)
        if kind == -1:
            return "" if v is None else str(v)
        if int(v) == -2 ** 31:
            return ""
        if lev is not None:
            return str(lev[int(v) - 1]) if 1 <= int(v) <= len(lev) else ""
        return str(int(v))

    with opener(report_file) as f:
        f.write("\t".join(k for k, _, _, _ in cols) + "\n")
        for i in range(n):
            f.write("\t".join(cell(kind, a, lev, i) for _, kind, a, lev in cols) + "\n")
