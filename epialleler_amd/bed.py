"""BED-assisted reports: the R-level callers that reuse thresholding and per-read beta
(SURVEY 8f row 3).  Mirrors R/generateBedReport.R:219-273 (+ generateAmpliconReport /
generateCaptureReport aliases), R/generateBedEcdf.R:122-153 and the helpers
.readBed / .matchTarget / .getBedReport / .getBedEcdf (R/internal.R:205-222, 463-478, 529-604).
Matching runs on the GPU (epi_batch_match_target_dev); the per-region tallies are what data.table's
dcast/merge do in the reference and are done with torch.bincount on the device vectors.
"""
import ctypes as C

import numpy as np

from . import _lib
from .api import (CONTEXT_TO_BASES, Report, _CTX_CHOICES, _as_bam, _deliver, _match_arg, _stream, _whole_number, preprocessBam,
                  rcpp_extract_patterns, rcpp_extract_patterns_multi, rcpp_get_xm_beta, rcpp_region_report,
                  rcpp_summarise_patterns_multi, rcpp_threshold_reads, writeReport)

NA_INTEGER = -2 ** 31


class Bed:
    """A BED table as GRanges would hold it: 1-based closed ranges + the extra columns."""

    def __init__(self, chrom, start, end, extra=None):
        self.chrom = list(chrom)
        self.start = np.asarray(start, np.int64)
        self.end = np.asarray(end, np.int64)
        self.extra = dict(extra or {})

    def __len__(self):
        return len(self.chrom)

    def names(self):
        """as.character(GRanges): "chr:start-end"."""
        return ["%s:%d-%d" % (c, s, e) for c, s, e in zip(self.chrom, self.start, self.end)]


def readBed(bed_file, zero_based_bed=False):
    """R/internal.R:205-222: tab-separated, blank lines skipped, first three columns chr/start/end,
    header detected as data.table::fread does (a first line whose start/end are not numeric)."""
    rows = []
    with open(bed_file) as f:
        for ln in f:
            ln = ln.rstrip("\n\r")
            if ln.strip():
                rows.append(ln.split("\t"))
    header = None
    if rows and not (rows[0][1].lstrip("-").isdigit() and rows[0][2].lstrip("-").isdigit()):
        header, rows = rows[0], rows[1:]
    ncol = max(len(r) for r in rows) if rows else 3
    names = list(header) if header else ["V%d" % (i + 1) for i in range(ncol)]
    names[:3] = ["chr", "start", "end"]
    start = np.asarray([int(r[1]) for r in rows], np.int64) + (1 if zero_based_bed else 0)
    end = np.asarray([int(r[2]) for r in rows], np.int64)
    extra = {names[i]: [r[i] if i < len(r) else "" for r in rows] for i in range(3, ncol)}
    return Bed([r[0] for r in rows], start, end, extra)


def _match_target(bam, bed, bed_type, match_tolerance, match_min_overlap):
    """.matchTarget (R/internal.R:463-478): BED seqnames become factor codes of the BAM's rname levels."""
    import torch
    lib = _lib.load()
    b = bam.batch()
    dev = "cuda:%d" % bam.device
    levels = list(bam.levels) if bam.levels is not None else []
    idx = {c: i + 1 for i, c in enumerate(levels)}
    chrom = np.asarray([idx.get(c, NA_INTEGER) for c in bed.chrom], np.int32)   # NA never equals an rname
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    d_chr, d_s, d_e = t(chrom), t(bed.start), t(bed.end)
    out = torch.empty(max(bam.n, 1), dtype=torch.int32, device=dev)
    _lib.check(lib.epi_batch_match_target_dev(
        b, C.c_void_p(d_chr.data_ptr()), C.c_void_p(d_s.data_ptr()), C.c_void_p(d_e.data_ptr()), len(bed),
        1 if bed_type == "capture" else 0, int(match_min_overlap if bed_type == "capture" else match_tolerance),
        C.c_void_p(out.data_ptr()), _stream(bam.device)))
    return out[:bam.n]


def generateBedReport(bam, bed, report_file=None, zero_based_bed=False, bed_type=None, match_tolerance=1,
                      match_min_overlap=1, threshold_reads=True, threshold_context=None, min_context_sites=2,
                      min_context_beta=0.5, max_outofcontext_beta=0.1, gzip=False, verbose=False, **preprocess_args):
    """R/generateBedReport.R:219-273.  Returns the BED rows (plus a last NA row for unmatched reads, when there
    are any) with columns seqnames,start,end,width,strand,<extra>,nreads+,nreads-,VEF; NaN where R has NA."""
    import torch
    bed_type = _match_arg(bed_type, ("amplicon", "capture"), "bed.type")
    threshold_context = _match_arg(threshold_context, _CTX_CHOICES, "threshold.context")
    if not isinstance(bed, Bed):
        bed = readBed(bed, zero_based_bed)
    bam = _as_bam(preprocessBam(bam, **preprocess_args))
    bam.batch()
    dev = "cuda:%d" % bam.device
    if threshold_reads:
        c = CONTEXT_TO_BASES[threshold_context]
        pass_ = rcpp_threshold_reads(bam, c["ctx_meth"], c["ctx_unmeth"], c["ooctx_meth"], c["ooctx_unmeth"],
                                     min_context_sites, min_context_beta, max_outofcontext_beta, as_device=True)
    else:
        pass_ = torch.ones(bam.n, dtype=torch.int32, device=dev)
    match = _match_target(bam, bed, bed_type, match_tolerance, match_min_overlap)
    strand = bam.dev["strand"] if bam.dev is not None else torch.from_numpy(bam.host["strand"]).to(dev)
    # .getBedReport (R/internal.R:529-561): reads per (bedmatch, strand, pass); NA matches get slot nbed
    nbed = len(bed)
    slot = torch.where(match < 0, torch.full_like(match, nbed), match - 1).to(torch.int64)
    key = slot * 4 + (strand.to(torch.int64) - 1) * 2 + (pass_ != 0).to(torch.int64)
    key = key[(strand >= 1) & (strand <= 2)]                # (strand 0: the reference's placeholder template of an empty paired-end
                                                            # file, src/rcpp_read_bam.cpp:155 -- an NA strand, counted on neither)
    cnt = torch.bincount(key, minlength=(nbed + 1) * 4).reshape(nbed + 1, 2, 2).cpu().numpy().astype(np.float64)
    present = cnt.sum(axis=(1, 2)) > 0                      # regions with no read at all are NA after the merge
    rows = list(range(nbed)) + ([nbed] if present[nbed] else [])
    npl, nmi = cnt[:, 0, :].sum(1), cnt[:, 1, :].sum(1)
    vef = np.divide(cnt[:, :, 1].sum(1), npl + nmi, out=np.full(nbed + 1, np.nan), where=(npl + nmi) > 0)
    na = lambda a: np.where(present, a, np.nan)[rows]
    cols = {"seqnames": np.asarray(bed.chrom + [None], object)[rows],
            "start": np.append(bed.start.astype(np.float64), np.nan)[rows],
            "end": np.append(bed.end.astype(np.float64), np.nan)[rows],
            "width": np.append((bed.end - bed.start + 1).astype(np.float64), np.nan)[rows],
            "strand": np.asarray(["*"] * nbed + [None], object)[rows]}
    for k, v in bed.extra.items():
        cols[k] = np.asarray(list(v) + [None], object)[rows]
    cols["nreads+"] = na(npl)
    cols["nreads-"] = na(nmi)
    cols["VEF"] = na(vef) if threshold_reads else np.full(len(rows), np.nan)          # :267
    rep = Report(cols)
    rep.levels = {}
    if report_file is None:
        return rep
    writeReport(rep, report_file, gzip)
    return None


def generateAmpliconReport(bam, bed, **kw):
    """R/generateBedReport.R:187-199."""
    kw.pop("bed_type", None)
    return generateBedReport(bam, bed, bed_type="amplicon", **kw)


def generateCaptureReport(bam, bed, **kw):
    """R/generateBedReport.R:203-215."""
    kw.pop("bed_type", None)
    return generateBedReport(bam, bed, bed_type="capture", **kw)


class Ecdf:
    """stats::ecdf of a numeric vector: right-continuous step function, callable on scalars or arrays."""

    def __init__(self, x):
        self.x = np.sort(np.asarray(x, np.float64))

    def __call__(self, q):
        n = self.x.size
        r = np.searchsorted(self.x, np.asarray(q, np.float64), side="right") / n if n else np.full(np.shape(q), np.nan)
        return float(r) if np.ndim(q) == 0 else r


def generateBedEcdf(bam, bed, bed_type=None, bed_rows=(1,), zero_based_bed=False, match_tolerance=1,
                    match_min_overlap=1, ecdf_context=None, verbose=False, **preprocess_args):
    """R/generateBedEcdf.R:122-153 + .getBedEcdf (R/internal.R:568-604).  bed_rows: 1-based BED rows, None = all
    (including the NA group of unmatched reads, keyed None).  Returns {region name: {"context": Ecdf,
    "out.of.context": Ecdf}} in the reference's order."""
    bed_type = _match_arg(bed_type, ("amplicon", "capture"), "bed.type")
    ecdf_context = _match_arg(ecdf_context, _CTX_CHOICES, "ecdf.context")
    if not isinstance(bed, Bed):
        bed = readBed(bed, zero_based_bed)
    bam = _as_bam(preprocessBam(bam, **preprocess_args))
    c = CONTEXT_TO_BASES[ecdf_context]
    match = _match_target(bam, bed, bed_type, match_tolerance, match_min_overlap).cpu().numpy()
    ctx_beta = rcpp_get_xm_beta(bam, c["ctx_meth"], c["ctx_unmeth"])
    oo_beta = rcpp_get_xm_beta(bam, c["ooctx_meth"], c["ooctx_unmeth"])
    all_rows = sorted(set(int(m) for m in np.unique(match[match > 0]))) + ([None] if (match < 0).any() else [])
    rows = all_rows if bed_rows is None else [r for r in bed_rows if r in all_rows]      # intersect(bed.rows, all.bed.rows)
    names = bed.names()
    out = {}
    for r in rows:
        sel = (match < 0) if r is None else (match == r)
        out[None if r is None else names[r - 1]] = {"context": Ecdf(ctx_beta[sel]), "out.of.context": Ecdf(oo_beta[sel])}
    return out


def _pattern_bed(bed, zero_based_bed):
    """The `bed` argument of extractPatterns: a Bed, a string "chr:start-end", or a path."""
    if isinstance(bed, str) and ":" in bed and "-" in bed.rsplit(":", 1)[1] and not __import__("os").path.exists(bed):
        chrom, rng = bed.rsplit(":", 1)                                        # as("chr:start-end", "GRanges")
        a, b_ = rng.split("-")
        return Bed([chrom], [int(a)], [int(b_)])
    return bed if isinstance(bed, Bed) else readBed(bed, zero_based_bed)


def extractPatterns(bam, bed, bed_row=1, zero_based_bed=False, match_min_overlap=1, extract_context=None,
                    min_context_freq=0.01, clip_patterns=False, strand_offset=None, highlight_positions=(), verbose=False,
                    **preprocess_args):
    """R/extractPatterns.R:107-143 + .getPatterns (R/internal.R:683-714).  bed: a path, a Bed, or a string
    "chr:start-end"; bed_row is 1-based.  The result carries the BED row it belongs to in `.bed`."""
    extract_context = _match_arg(extract_context, _CTX_CHOICES, "extract.context")
    if strand_offset is None:
        strand_offset = {"CG": 1, "CHG": 2, "CHH": 0, "CxG": 0, "CX": 0}[extract_context]
    bed = _pattern_bed(bed, zero_based_bed)
    bam = _as_bam(preprocessBam(bam, **preprocess_args))
    row = int(np.atleast_1d(bed_row)[0]) - 1
    if row < 0 or row >= len(bed):
        return Report({}, bam.levels)                                          # data.table()[bed.row] of a missing row: no target
    levels = list(bam.levels) if bam.levels is not None else []
    chrom = bed.chrom[row]
    seq = levels.index(chrom) + 1 if chrom in levels else NA_INTEGER           # factor(seqnames, levels=levels(rname))
    start, end = int(bed.start[row]), int(bed.end[row])
    hl = sorted({int(p) for p in np.atleast_1d(np.asarray(highlight_positions, np.int64)) if start <= int(p) <= end})
    c = CONTEXT_TO_BASES[extract_context]
    rep = rcpp_extract_patterns(bam, seq, start, end, match_min_overlap, c["ctx_meth"] + c["ctx_unmeth"], min_context_freq,
                                clip_patterns, int(strand_offset), hl)
    rep.bed = bed.names()[row]
    return rep


def _pattern_calls(bam, bed, bed_rows, zero_based_bed, extract_context, strand_offset, highlight_positions, preprocess_args):
    """What extractPatternsBed and summarisePatterns do before their GPU call: the arguments checked before any I/O, the
    BAM preprocessed once, the requested BED rows as (rname code, start, end) with the highlight positions inside each.
    -> (bam, bed, the requested rows 0-based, the indices of those inside the BED, their targets, their highlight
    positions, the context letters, the strand offset)"""
    extract_context = _match_arg(extract_context, _CTX_CHOICES, "extract.context")
    if bed_rows is not None:
        bed_rows = list(np.atleast_1d(np.asarray(bed_rows, object)))
        for r in bed_rows:
            if isinstance(r, (bool, np.bool_)) or not isinstance(r, (int, np.integer)):
                raise ValueError("'bed.rows' should be None or 1-based integer row numbers, not %r" % (r,))
    if strand_offset is None:
        strand_offset = {"CG": 1, "CHG": 2, "CHH": 0, "CxG": 0, "CX": 0}[extract_context]
    bed = _pattern_bed(bed, zero_based_bed)
    bam = _as_bam(preprocessBam(bam, **preprocess_args))
    rows = list(range(len(bed))) if bed_rows is None else [int(r) - 1 for r in bed_rows]
    levels = list(bam.levels) if bam.levels is not None else []
    code = {c: i + 1 for i, c in enumerate(levels)}
    hl_all = np.unique(np.atleast_1d(np.asarray(highlight_positions, np.int64)))
    keep = [k for k, r in enumerate(rows) if 0 <= r < len(bed)]
    targets, hl = [], []
    for k in keep:
        r = rows[k]
        start, end = int(bed.start[r]), int(bed.end[r])
        targets.append((code.get(bed.chrom[r], NA_INTEGER), start, end))       # factor(seqnames, levels=levels(rname))
        hl.append([int(p) for p in hl_all[(hl_all >= start) & (hl_all <= end)]])
    c = CONTEXT_TO_BASES[extract_context]
    return bam, bed, rows, keep, targets, hl, c["ctx_meth"] + c["ctx_unmeth"], int(strand_offset)


def _pattern_reports(bam, bed, rows, keep, reps):
    """One Report per requested row: reps for those inside the BED, each with its BED row's name, and the empty Report
    of data.table()[bed.row] for a missing row."""
    names = bed.names()
    out = [Report({}, bam.levels) for _ in rows]
    for k, rep in zip(keep, reps):
        rep.bed = names[rows[k]]
        out[k] = rep
    return out


def extractPatternsBed(bam, bed, bed_rows=None, zero_based_bed=False, match_min_overlap=1, extract_context=None,
                       min_context_freq=0.01, clip_patterns=False, strand_offset=None, highlight_positions=(), verbose=False,
                       **preprocess_args):
    """extractPatterns for many BED rows in one pass on the GPU (epi_batch_extract_patterns_multi): the list
    [extractPatterns(bam, bed, bed_row=r, ...) for r in bed_rows], at the cost of the reads on the targets instead of
    one scan of the batch per target.  bed_rows: 1-based rows in the order wanted, duplicates allowed, None = every
    row in BED order; a row outside the BED gives the empty Report the single call gives.  highlight_positions: one
    list for the call, every target uses the positions inside it.  The BAM is preprocessed once."""
    bam, bed, rows, keep, targets, hl, ctx, offset = _pattern_calls(bam, bed, bed_rows, zero_based_bed, extract_context, strand_offset,
                                                                    highlight_positions, preprocess_args)
    reps = rcpp_extract_patterns_multi(bam, targets, match_min_overlap, ctx, min_context_freq, clip_patterns, offset, hl)
    return _pattern_reports(bam, bed, rows, keep, reps)


def summarisePatterns(bam, bed, bed_rows=None, zero_based_bed=False, match_min_overlap=1, extract_context=None,
                      min_context_freq=0.01, clip_patterns=False, strand_offset=None, highlight_positions=(),
                      bin_context=None, verbose=False, **preprocess_args):
    """The epiallele frequency table of every requested BED row: what plotPatterns makes of extractPatterns' table
    before it draws (R/plotPatterns.R:170-184).  For a row r, with P = extractPatterns(bam, bed, bed_row=r, ...), the
    Report holds the unique rows of P by (pattern, every position column) in the order of their first appearance in P:
    `pattern` (16 hex digits), one column per position, `count`, and `beta` (float64) for bin_context (default: the
    first choice, "CG", as plotPatterns' bin.context).  Strand, start, end and nbase are not part of the key and are not
    returned.  The rows are grouped on the GPU (epi_batch_summarise_patterns_multi): nothing per read comes to the
    host.  bed_rows as extractPatternsBed: 1-based, duplicates allowed, None = every row; a row outside the BED, or one
    without patterns, gives an empty Report.  `.bed` and `.pattern_levels` as on extractPatterns' Report."""
    bin_context = _match_arg(bin_context, _CTX_CHOICES, "bin.context")
    bam, bed, rows, keep, targets, hl, ctx, offset = _pattern_calls(bam, bed, bed_rows, zero_based_bed, extract_context, strand_offset,
                                                                    highlight_positions, preprocess_args)
    cb = CONTEXT_TO_BASES[bin_context]
    reps = rcpp_summarise_patterns_multi(bam, targets, match_min_overlap, ctx, min_context_freq, clip_patterns, offset, hl,
                                         (cb["ctx_meth"], cb["ctx_unmeth"]))
    return _pattern_reports(bam, bed, rows, keep, reps)


def generateRegionReport(bam, bed, report_file=None, zero_based_bed=False, region_context=None, min_sites=4, max_sites=64,
                         strand_offset=None, uxm_thresholds=(0.25, 0.75), max_outofcontext_beta=0.1, gzip=False, verbose=False,
                         as_device=False, **preprocess_args):
    """Read-level methylation statistics per region: one row per region of `bed`, in its order.  A read's calls in a region
    are its cytosines of `region_context` whose position (less `strand_offset` on the reverse strand: 1 for CG, 2 for CHG,
    else 0, as in extractPatterns) lies inside; the reads are those generateMhlReport keeps under max_outofcontext_beta.
    Reads with 1 to `max_sites` (1 to 256) calls are counted, those with at least `min_sites` (1 to max_sites) are the
    k-reads; a read with more than max_sites calls is counted in nlong only.  Columns: rname, start, end, nreads, nlong,
    kreads, tbase, mbase, cbase, ndiscordant, nmethylated, n_u, n_x, n_m, maxsites (int32); beta (mean methylation), pdr
    (share of k-reads with both states), chalm (share of k-reads with a methylated call), mcr (unmethylated calls on reads
    with a methylated one, over all calls), mbs (methylation block score), mhl (methylated haplotype load, Guo et al.
    2017) (float64).  n_u / n_x / n_m split the k-reads by their methylated share m / n at uxm_thresholds = (u_max, m_min):
    m <= u_max n, m >= m_min n, and the rest.  A region nothing falls on has zero counts and NaN ratios; regions may
    overlap, repeat and come in any order.  bed: a path, a Bed, "chr:start-end", or a Report with rname, start and end
    columns (generateHaplotypeBlocks, generateDmrReport; on the host or on the device) whose rname codes are used as they
    are and whose strand is ignored.  include/epihip.h has the definitions.  The reference has no such report."""
    region_context = _match_arg(region_context, _CTX_CHOICES, "region.context")
    max_sites = _whole_number(max_sites, "max.sites", 1, 256)
    min_sites = _whole_number(min_sites, "min.sites", 1, max_sites)
    if strand_offset is None:
        strand_offset = {"CG": 1, "CHG": 2, "CHH": 0, "CxG": 0, "CX": 0}[region_context]
    strand_offset = _whole_number(strand_offset, "strand.offset", 0, 2 ** 31 - 1)
    try:
        u_max, m_min = (float(v) for v in uxm_thresholds)
        ok = 0 <= u_max < m_min <= 1
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("'uxm.thresholds' should be two numbers (u_max, m_min) with 0 <= u_max < m_min <= 1")
    from_report = isinstance(bed, Report)
    if from_report:
        for k in ("rname", "start", "end"):
            if k not in bed:
                raise ValueError("'bed' should be a BED file, a Bed, \"chr:start-end\" or a Report with rname, start and end columns")
    else:
        bed = _pattern_bed(bed, zero_based_bed)
    bam = _as_bam(preprocessBam(bam, **preprocess_args))
    if from_report:
        regions = (bed["rname"], bed["start"], bed["end"])
    else:
        code = {c: i + 1 for i, c in enumerate(bam.levels or ())}
        regions = ([code.get(c, NA_INTEGER) for c in bed.chrom], bed.start, bed.end)   # factor(seqnames, levels=levels(rname))
    c = CONTEXT_TO_BASES[region_context]
    rep = rcpp_region_report(bam, regions, c["ctx_meth"] + c["ctx_unmeth"], min_sites, max_sites, strand_offset, u_max, m_min,
                             max_outofcontext_beta, as_device=True)
    return _deliver(rep, report_file, gzip, as_device)


def selectPatterns(summary, order_by="beta", beta_range=(0, 1), nbins=10, npatterns_per_bin=2):
    """The table plotPatterns returns invisibly (R/plotPatterns.R:168, :186-188), from a summarisePatterns Report: the
    most frequent unique patterns of every beta bin.
      bins  nbins + 1 equally spaced edges over beta_range (seq(from, to, length.out=nbins + 1))
      bin   findInterval(beta, bins, all.inside=TRUE), 1-based, for a beta inside the closed range; other rows are dropped
      rows  a stable sort by count, descending; per bin, in the order the bins first appear in that sorted table, the first
            npatterns_per_bin[bin - 1] rows (the value is recycled to nbins entries; float("inf") keeps all)
      I     number of selected rows - rank; rank 1 is the first row in decreasing (order_by, beta, count) order, ties in
            table order
    Returns a Report with the summary's columns plus `bin` (int32) and `I` (int32); `.bins` holds the edges.
    These semantics are read from the reference's source; nothing here can run R, so they are not pinned against it,
    and the last bits of the bin edges (R's seq against numpy's linspace) are not pinned either."""
    if order_by not in ("beta", "count"):
        raise ValueError("'order.by' should be one of 'beta', 'count'")
    nbins = int(nbins)
    if nbins < 1:
        raise ValueError("'nbins' should be at least 1")
    lo, hi = (float(v) for v in beta_range)
    if not lo <= hi:
        raise ValueError("'beta.range' should be (from, to) with from <= to")
    per = np.resize(np.atleast_1d(np.asarray(npatterns_per_bin, np.float64)), nbins)
    bins = np.linspace(lo, hi, nbins + 1)
    out = Report({}, getattr(summary, "levels", {}).get("rname"))
    for a in ("bed", "pattern_levels"):
        if hasattr(summary, a):
            setattr(out, a, getattr(summary, a))
    out.bins = bins
    if not summary:
        return out
    beta, count = np.asarray(summary["beta"], np.float64), np.asarray(summary["count"])
    inside = np.flatnonzero((beta >= lo) & (beta <= hi))
    bin_ = np.clip(np.searchsorted(bins, beta[inside], side="right"), 1, nbins)          # all.inside=TRUE
    order = np.argsort(-count[inside].astype(np.int64), kind="stable")
    taken = {}
    for j in order:                                                            # (groups in order of first appearance)
        taken.setdefault(int(bin_[j]), [])
        if len(taken[int(bin_[j])]) < per[int(bin_[j]) - 1]:
            taken[int(bin_[j])].append(j)
    sel = np.asarray([j for js in taken.values() for j in js], np.int64)
    idx = inside[sel]
    for k in summary:
        out[k] = np.asarray(summary[k])[idx]
    out["bin"] = bin_[sel].astype(np.int32)
    n = idx.size
    cnt = count[idx].astype(np.float64)
    # decreasing (order_by, beta, count), ties in table order: a stable sort on the negated keys, the last key first
    rank = np.lexsort((-cnt, -beta[idx], -(cnt if order_by == "count" else beta[idx])))
    I = np.empty(n, np.int32)
    I[rank] = n - np.arange(1, n + 1)
    out["I"] = I
    return out
