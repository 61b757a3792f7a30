"""generateVcfReport: base frequencies and Fisher exact tests at the SNVs of a VCF file.
Mirrors R/generateVcfReport.R, .readVcf (R/internal.R:230-267) and .getBaseFreqReport (R/internal.R:611-676), with the
Rcpp exports rcpp_get_base_freqs (src/rcpp_get_base_freqs.cpp) and rcpp_fep (src/rcpp_fep.cpp).  The VCF is parsed by
the library (epi_read_vcf), the per-site tallies run on the GPU (epi_batch_base_freqs_dev) and the Fisher tests on the
host (epi_fisher_exact).

Seqlevels styles: GenomeInfoDb's tables are not reproduced.  Only what the reference's fixtures need is: "UCSC" names
carry a "chr" prefix, "NCBI" / "Ensembl" names do not, and "chrM" <-> "MT".
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from .api import CONTEXT_TO_BASES, Report, _CTX_CHOICES, _as_bam, _pass_tensor, _stream, preprocessBam, \
    rcpp_threshold_reads, writeReport
from .bed import Bed, readBed

NA_INTEGER = -2 ** 31

# .getBaseFreqReport's column names of the rcpp_get_base_freqs matrix (R/internal.R:629-633)
FREQ_COLUMNS = tuple("%s%s%s" % (m, s, b) for m in "UM" for s in "+-" for b in "ACGTN")
REPORT_COLUMNS = ("name", "seqnames", "range", "REF", "ALT", "M+Ref", "U+Ref", "M-Ref", "U-Ref", "M+Alt", "U+Alt",
                  "M-Alt", "U-Alt", "SumRef", "SumAlt", "FEp+", "FEp-")

# R/internal.R:642-666: per (REF, ALT) the bases summed into M+Ref, U+Ref, M-Ref, U-Ref, M+Alt, U+Alt, M-Alt, U-Alt
# (the strand is the column's own; None = NA: the strand cannot tell the alleles apart after bisulfite conversion)
_ALLELE_TABLE = {
    ("A", "C"): ("A", "A", "A", "A", "CT", "CT", "C", "C"),
    ("A", "T"): ("A", "A", "A", "A", "T", "T", "T", "T"),
    ("A", "G"): ("A", "A", None, None, "G", "G", None, None),
    ("C", "A"): ("CT", "CT", "C", "C", "A", "A", "A", "A"),
    ("C", "T"): (None, None, "C", "C", None, None, "T", "T"),
    ("C", "G"): ("CT", "CT", "C", "C", "G", "G", "AG", "AG"),
    ("T", "A"): ("T", "T", "T", "T", "A", "A", "A", "A"),
    ("T", "C"): (None, None, "T", "T", None, None, "C", "C"),
    ("T", "G"): ("T", "T", "T", "T", "G", "G", "AG", "AG"),
    ("G", "A"): ("G", "G", None, None, "A", "A", None, None),
    ("G", "C"): ("G", "G", "AG", "AG", "CT", "CT", "C", "C"),
    ("G", "T"): ("G", "G", "AG", "AG", "T", "T", "T", "T"),
}
_ALLELE_COLUMNS = ("M+Ref", "U+Ref", "M-Ref", "U-Ref", "M+Alt", "U+Alt", "M-Alt", "U-Alt")


class Vcf:
    """The SNV rows of a VCF as the reference keeps them after readVcf + expand: one row per ALT allele, single-base
    REF and single-character ALT, in file order.  chrom: 0-based codes into `levels` (the seqlevels)."""

    def __init__(self, levels, chrom, pos, ref, alt, names):
        self.levels = list(levels)
        self.chrom = np.asarray(chrom, np.int32)
        self.pos = np.asarray(pos, np.int32)
        self.ref = np.asarray(ref, dtype="U1")
        self.alt = np.asarray(alt, dtype="U1")
        self.names = np.asarray(names, dtype=object)

    def __len__(self):
        return int(self.pos.size)

    @property
    def seqnames(self):
        return np.asarray(self.levels, dtype=object)[self.chrom] if len(self) else np.asarray([], dtype=object)

    def subset(self, sel):
        return Vcf(self.levels, self.chrom[sel], self.pos[sel], self.ref[sel], self.alt[sel], self.names[sel])

    def restyle(self, style):
        """seqlevelsStyle(x) <- style, for the chr / MT rules only."""
        return Vcf([_rename(s, style) for s in self.levels], self.chrom, self.pos, self.ref, self.alt, self.names)


def _style_of(names):
    """seqlevelsStyle() of a set of names, by the chr-prefix rule: UCSC if most carry the prefix."""
    names = list(names)
    chr_ = sum(1 for s in names if s.startswith("chr"))
    return "UCSC" if names and 2 * chr_ >= len(names) else "NCBI"


def _rename(name, style):
    if style == "UCSC":
        if name == "MT":
            return "chrM"
        return name if name.startswith("chr") else "chr" + name
    if style in ("NCBI", "Ensembl"):
        if name == "chrM":
            return "MT"
        return name[3:] if name.startswith("chr") else name
    raise ValueError("seqlevels style %r is not supported (UCSC, NCBI, Ensembl)" % (style,))


def _reduce(bed):
    """GenomicRanges::reduce: per chromosome, overlapping or adjacent ranges merged."""
    out = {}
    for c in dict.fromkeys(bed.chrom):
        sel = np.asarray([x == c for x in bed.chrom])
        s, e = bed.start[sel], bed.end[sel]
        o = np.argsort(s, kind="stable")
        ms, me = [], []
        for a, b in zip(s[o], e[o]):
            if ms and a <= me[-1] + 1:
                me[-1] = max(me[-1], b)
            else:
                ms.append(a)
                me.append(b)
        out[c] = (np.asarray(ms, np.int64), np.asarray(me, np.int64))
    return out


def _read_vcf_file(path):
    lib = _lib.load()
    t = _lib.VcfTable()
    _lib.check(lib.epi_read_vcf(os.path.expanduser(str(path)).encode(), C.byref(t)))
    try:
        n = int(t.nrec)
        levels = [t.chrom_names[i].decode("latin1") for i in range(t.n_chrom)]
        chrom = np.ctypeslib.as_array(t.chrom, (n,)).copy() if n else np.zeros(0, np.int32)
        pos = np.ctypeslib.as_array(t.pos, (n,)).copy() if n else np.zeros(0, np.int32)
        ref = np.frombuffer(C.string_at(t.ref, n), dtype="S1").astype("U1") if n else np.zeros(0, "U1")
        alt = np.frombuffer(C.string_at(t.alt, n), dtype="S1").astype("U1") if n else np.zeros(0, "U1")
        names = C.string_at(t.names, int(t.names_bytes)).decode("latin1").split("\0")[:n] if n else []
    finally:
        lib.epi_vcf_free(C.byref(t))
    return Vcf(levels, chrom, pos, ref, alt, names)


def readVcf(path, vcf_style=None, bed=None, zero_based_bed=False):
    """.readVcf (R/internal.R:230-267) + expand(): with a BED, only the records inside reduce(bed) -- the BED's names
    renamed to vcf_style for the query, the VCF's renamed to the BED's style afterwards."""
    vcf = _read_vcf_file(path)
    if bed is None:
        return vcf
    if not isinstance(bed, Bed):
        bed = readBed(bed, zero_based_bed)
    bed_style = _style_of(dict.fromkeys(bed.chrom))
    if vcf_style is not None:
        bed = Bed([_rename(c, vcf_style) for c in bed.chrom], bed.start, bed.end, bed.extra)
    keep = np.zeros(len(vcf), bool)
    names = vcf.seqnames
    for c, (s, e) in _reduce(bed).items():
        sel = np.flatnonzero(names == c)
        if sel.size and s.size:
            p = vcf.pos[sel].astype(np.int64)
            k = np.searchsorted(s, p, side="right") - 1           # the last range starting at or before p
            keep[sel] = (k >= 0) & (p <= e[np.maximum(k, 0)])
    return vcf.subset(keep).restyle(bed_style)


# ---- Rcpp-level functions ----------------------------------------------------------------------

def rcpp_get_base_freqs(df, pass_, vcf_chr, vcf_pos):
    """src/rcpp_get_base_freqs.cpp:15-57 -> (nsite, 20) float64 matrix, columns FREQ_COLUMNS.  vcf_chr: rname factor
    codes of the sites (NA_INTEGER: a zero row), in any order -- the counts do not depend on it (the reference's merge
    needs the sites sorted in the BAM's level order)."""
    import torch
    lib = _lib.load()
    bam = _as_bam(df)
    b = bam.batch()
    dev = "cuda:%d" % bam.device
    chr_ = np.ascontiguousarray(vcf_chr, np.int32)
    pos = np.ascontiguousarray(vcf_pos, np.int32)
    if chr_.shape != pos.shape:
        raise ValueError("vcf seqnames and start must have the same length")
    res = np.zeros((chr_.size, 20), np.float64)
    idx = np.flatnonzero(chr_ != NA_INTEGER)
    idx = idx[np.lexsort((pos[idx], chr_[idx]))]                 # (code, pos), stable
    m = int(idx.size)
    if m == 0:
        return res
    p = _pass_tensor(bam, pass_)
    d_chr = torch.from_numpy(chr_[idx]).to(dev)
    d_pos = torch.from_numpy(pos[idx]).to(dev)
    cnt = torch.empty(20 * m, dtype=torch.int32, device=dev)
    _lib.check(lib.epi_batch_base_freqs_dev(b, C.c_void_p(p.data_ptr()) if p is not None and bam.n else None,
                                            C.c_void_p(d_chr.data_ptr()), C.c_void_p(d_pos.data_ptr()), m,
                                            C.c_void_p(cnt.data_ptr()), _stream(bam.device)))
    res[idx, :] = cnt.cpu().numpy().view(np.uint32).reshape(20, m).T
    return res


def rcpp_fep(df, colnames, nthreads=None):
    """src/rcpp_fep.cpp:10-36: two-sided Fisher exact p-values of the tables (df[colnames[0]], df[colnames[1]] /
    df[colnames[2]], df[colnames[3]]); NA (NaN or NA_INTEGER) in any cell gives NaN."""
    lib = _lib.load()
    cells = []
    for k in colnames[:4]:
        a = np.asarray(df[k])
        if a.dtype.kind == "f":
            a = np.where(np.isnan(a), NA_INTEGER, a)
        cells.append(np.ascontiguousarray(a, np.int32))
    n = int(cells[0].size)
    out = np.empty(n, np.float64)
    if n:
        if nthreads is None:
            nthreads = min(os.cpu_count() or 1, 16)
        _lib.check(lib.epi_fisher_exact(*[c.ctypes.data for c in cells], n, out.ctypes.data, int(nthreads)))
    return out


def base_freq_columns(freqs, ref, alt):
    """The allele columns of .getBaseFreqReport (R/internal.R:642-669) from the (nsite, 20) matrix: M+Ref .. U-Alt
    (NaN = NA), SumRef, SumAlt."""
    freqs = np.asarray(freqs, np.float64)
    n = freqs.shape[0]
    out = {k: np.full(n, np.nan) for k in _ALLELE_COLUMNS}
    col = {k: i for i, k in enumerate(FREQ_COLUMNS)}
    ref = np.asarray(ref).astype("U1")
    alt = np.asarray(alt).astype("U1")
    for (r, a), bases in _ALLELE_TABLE.items():
        sel = np.flatnonzero((ref == r) & (alt == a))
        if not sel.size:
            continue
        for name, bs in zip(_ALLELE_COLUMNS, bases):
            if bs is not None:
                ms = name[:2]                                     # "M+", "U-", ...
                out[name][sel] = sum(freqs[sel, col[ms + x]] for x in bs)
    out["SumRef"] = np.nansum(np.stack([out[k] for k in _ALLELE_COLUMNS[:4]]), axis=0)
    out["SumAlt"] = np.nansum(np.stack([out[k] for k in _ALLELE_COLUMNS[4:]]), axis=0)
    return out


def generateVcfReport(bam, vcf, vcf_style=None, bed=None, report_file=None, zero_based_bed=False, threshold_reads=True,
                      threshold_context=None, min_context_sites=2, min_context_beta=0.5, max_outofcontext_beta=0.1,
                      gzip=False, verbose=False, **preprocess_args):
    """R/generateVcfReport.R.  vcf: a path, or a Vcf from readVcf (then bed and zero_based_bed have no effect).
    Returns a Report with the 17 columns of REPORT_COLUMNS (NaN where R has NA; seqnames a factor over the BAM's
    rname levels)."""
    import torch
    from .api import _match_arg
    threshold_context = _match_arg(threshold_context, _CTX_CHOICES, "threshold.context")
    if not isinstance(vcf, Vcf):
        vcf = readVcf(vcf, vcf_style=vcf_style, bed=bed, zero_based_bed=zero_based_bed)
    bam = _as_bam(preprocessBam(bam, **preprocess_args))
    bam.batch()
    if threshold_reads:
        c = CONTEXT_TO_BASES[threshold_context]
        pass_ = rcpp_threshold_reads(bam, c["ctx_meth"], c["ctx_unmeth"], c["ooctx_meth"], c["ooctx_unmeth"],
                                     min_context_sites, min_context_beta, max_outofcontext_beta, as_device=True)
    else:
        pass_ = torch.ones(bam.n, dtype=torch.int32, device="cuda:%d" % bam.device)
    # .getBaseFreqReport: sort(rowRanges) -- seqlevels order, then start (stable) -- and seqnames as BAM factor codes
    vcf = vcf.subset(np.lexsort((vcf.pos, vcf.chrom)))
    levels = list(bam.levels) if bam.levels is not None else []
    code_of = {s: i + 1 for i, s in enumerate(levels)}
    lev_code = np.asarray([code_of.get(s, NA_INTEGER) for s in vcf.levels] or [NA_INTEGER], np.int32)
    seq = lev_code[vcf.chrom] if len(vcf) else np.zeros(0, np.int32)
    if not (seq != NA_INTEGER).any():
        raise ValueError("Looks like seqlevels styles of BAM and VCF don't match. "
                         "Please provide VCF as an object with correct seqlevels.")
    freqs = rcpp_get_base_freqs(bam, pass_, seq, vcf.pos)
    cols = {"name": vcf.names, "seqnames": seq, "range": vcf.pos.copy(),
            "REF": vcf.ref.astype(object), "ALT": vcf.alt.astype(object)}
    cols.update(base_freq_columns(freqs, vcf.ref, vcf.alt))
    cols["FEp+"] = rcpp_fep(cols, ("M+Ref", "U+Ref", "M+Alt", "U+Alt"))
    cols["FEp-"] = rcpp_fep(cols, ("M-Ref", "U-Ref", "M-Alt", "U-Alt"))
    rep = Report({k: cols[k] for k in REPORT_COLUMNS})
    rep.levels = {"seqnames": tuple(levels)}
    if report_file is None:
        return rep
    writeReport(rep, report_file, gzip)
    return None
