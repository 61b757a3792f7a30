"""generateVcfReport: base frequencies and Fisher exact tests at the SNVs of a VCF file; generateAsmReport and
generateAsmSnvReport: allele-specific methylation at those SNVs (no reference counterpart; at the end of this file).
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
from .api import CONTEXT_TO_BASES, Report, _CTX_CHOICES, _as_bam, _deliver, _fetch_table, _match_arg, _pass_tensor, _ptr_array, \
    _stream, _table_cols, _table_to_host, _whole_number, preprocessBam, rcpp_threshold_reads, writeReport
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


# ---- allele-specific methylation -----------------------------------------------------------------

_ASM_PAIR_DEVICE = ("snv", "rname", "snv_pos", "strand", "pos", "context", "meth_ref", "unmeth_ref", "meth_alt", "unmeth_alt",
                    "beta_ref", "beta_alt", "delta_beta", "p")
_ASM_SNV_DEVICE = ("rname", "pos", "reads_ref", "reads_alt", "reads_other", "npairs", "meth_ref", "unmeth_ref", "meth_alt",
                   "unmeth_alt", "beta_ref", "beta_alt", "delta_beta", "p")
ASM_COLUMNS = ("name", "REF", "ALT") + _ASM_PAIR_DEVICE
ASM_SNV_COLUMNS = ("name", "REF", "ALT") + _ASM_SNV_DEVICE
_BASE_BIT = {"A": 1, "C": 2, "G": 4, "T": 8}                 # 1 << seq_nt16_int


def allele_masks(ref, alt):
    """The site_alleles of epi_batch_asm_report_dev (include/epihip.h) from _ALLELE_TABLE: per (REF, ALT) four 4-bit masks
    over A, C, G, T -- bits 0-3 the bases read as REF on '+' rows, 4-7 as ALT on '+', 8-11 REF on '-', 12-15 ALT on '-'
    (zero where the strand cannot tell the alleles apart after bisulfite conversion).  A pair that is not in the table
    gets 0 everywhere.  Returns int32."""
    ref = np.asarray(ref).astype("U1").reshape(-1)
    alt = np.asarray(alt).astype("U1").reshape(-1)
    if ref.shape != alt.shape:
        raise ValueError("REF and ALT must have the same length")
    out = np.zeros(ref.size, np.int32)
    for (r, a), bases in _ALLELE_TABLE.items():
        mask = 0
        for shift, bs in ((0, bases[0]), (8, bases[2]), (4, bases[4]), (12, bases[6])):     # M+Ref, M-Ref, M+Alt, M-Alt
            mask |= sum(_BASE_BIT[x] for x in (bs or "")) << shift
        out[(ref == r) & (alt == a)] = mask
    return out


def rcpp_asm_report(df, site_chr, site_pos, site_alleles, ctx, max_distance, min_coverage, max_ooctx_meth_frac, as_device=False):
    """Allele-specific methylation per (SNV, cytosine) and per SNV (include/epihip.h, epi_batch_asm_report_dev) ->
    (pairs, snvs), two Reports.  pairs: snv, rname, snv_pos, strand, pos, context, meth_ref, unmeth_ref, meth_alt,
    unmeth_alt (int32), beta_ref, beta_alt, delta_beta, p (float64), in (rname, snv_pos, snv, pos, strand, context) order.  snvs:
    one row per site, in the order given: rname, pos, reads_ref, reads_alt, reads_other, npairs and the four cells summed over
    the site's pair rows (int32), the pooled beta_ref, beta_alt, delta_beta, p (float64).  site_chr: rname factor codes
    (NA_INTEGER: a row of zero counts and NaN), site_alleles: allele_masks(); the sites in any order -- NA is dropped and the
    rest are sorted for the device, `snv` indexes the order given.  ctx: context letters in both cases, as for
    rcpp_mhl_report."""
    import torch
    lib = _lib.load()
    bam = _as_bam(df)
    b = bam.batch()
    dev = "cuda:%d" % bam.device
    chr_ = np.ascontiguousarray(np.asarray(site_chr, np.int64).astype(np.int32)).reshape(-1)
    pos = np.ascontiguousarray(np.asarray(site_pos, np.int64).astype(np.int32)).reshape(-1)
    masks = np.ascontiguousarray(np.asarray(site_alleles, np.int64).astype(np.int32)).reshape(-1)
    if not chr_.shape == pos.shape == masks.shape:
        raise ValueError("site seqnames, positions and alleles must have the same length")
    nsite = int(chr_.size)
    idx = np.flatnonzero(chr_ != NA_INTEGER)
    idx = idx[np.lexsort((pos[idx], chr_[idx]))]                 # (code, pos), stable
    m = int(idx.size)
    d_sites = [torch.from_numpy(a[idx]).to(dev) for a in (chr_, pos, masks)]
    icols, dcols = _table_cols(10, 4, m, dev)
    npair = C.c_int64(0)
    _lib.check(lib.epi_batch_asm_report_dev(b, *[C.c_void_p(t.data_ptr()) if m else None for t in d_sites], m, _lib.enc(ctx),
                                            int(max_distance), int(min_coverage), float(max_ooctx_meth_frac),
                                            _ptr_array(icols), _ptr_array(dcols), _stream(bam.device), C.byref(npair)))
    pairs = _fetch_table(bam, lib.epi_batch_asm_fetch_dev, npair.value, 10, _ASM_PAIR_DEVICE, True)
    d_idx = torch.from_numpy(idx).to(dev)
    pairs["snv"] = d_idx[pairs["snv"].long()].to(torch.int32)    # the caller's order
    # the SNV rows in the caller's order: an NA site keeps its code and position, counts nothing and has no ratio
    full_i = torch.zeros((10, nsite), dtype=torch.int32, device=dev)
    full_i[0] = torch.from_numpy(chr_).to(dev)
    full_i[1] = torch.from_numpy(pos).to(dev)
    full_d = torch.full((4, nsite), float("nan"), dtype=torch.float64, device=dev)
    if m:
        full_i[:, d_idx] = torch.stack(icols)
        full_d[:, d_idx] = torch.stack(dcols)
    snvs = Report(dict(zip(_ASM_SNV_DEVICE, list(full_i.unbind(0)) + list(full_d.unbind(0)))), bam.levels)
    return _table_to_host(pairs, as_device), _table_to_host(snvs, as_device)


def _asm_tables(bam, vcf, vcf_style, bed, zero_based_bed, asm_context, max_distance, min_coverage, max_outofcontext_beta,
                as_device, preprocess_args):
    """What generateAsmReport and generateAsmSnvReport share: the arguments, the VCF as generateVcfReport reads and styles
    it, and both tables with name, REF and ALT of the Vcf in front (host tables only)."""
    asm_context = _match_arg(asm_context, _CTX_CHOICES, "asm.context")
    max_distance = _whole_number(max_distance, "max.distance", 0, 2 ** 31 - 1)
    min_coverage = _whole_number(min_coverage, "min.coverage", 0, 2 ** 31 - 1)
    if not isinstance(vcf, Vcf):
        vcf = readVcf(vcf, vcf_style=vcf_style, bed=bed, zero_based_bed=zero_based_bed)
    bam = _as_bam(preprocessBam(bam, **preprocess_args))
    vcf = vcf.subset(np.lexsort((vcf.pos, vcf.chrom)))           # sort(rowRanges), as .getBaseFreqReport
    levels = list(bam.levels) if bam.levels is not None else []
    code_of = {s: i + 1 for i, s in enumerate(levels)}
    lev_code = np.asarray([code_of.get(s, NA_INTEGER) for s in vcf.levels] or [NA_INTEGER], np.int32)
    seq = lev_code[vcf.chrom] if len(vcf) else np.zeros(0, np.int32)
    if not (seq != NA_INTEGER).any():
        raise ValueError("Looks like seqlevels styles of BAM and VCF don't match. "
                         "Please provide VCF as an object with correct seqlevels.")
    c = CONTEXT_TO_BASES[asm_context]
    pairs, snvs = rcpp_asm_report(bam, seq, vcf.pos, allele_masks(vcf.ref, vcf.alt), c["ctx_meth"] + c["ctx_unmeth"],
                                  max_distance, min_coverage, max_outofcontext_beta, as_device=as_device)
    if as_device:
        return pairs, snvs
    s = pairs["snv"]
    front = lambda sel: {"name": vcf.names[sel], "REF": vcf.ref.astype(object)[sel], "ALT": vcf.alt.astype(object)[sel]}
    out = []
    for rep, sel in ((pairs, s), (snvs, slice(None))):
        cols = front(sel)
        cols.update(rep)
        out.append(Report(cols, rep.levels["rname"]))
    return out


def generateAsmReport(bam, vcf, vcf_style=None, bed=None, report_file=None, zero_based_bed=False, asm_context=None,
                      max_distance=0, min_coverage=1, max_outofcontext_beta=0.1, gzip=False, verbose=False, as_device=False,
                      **preprocess_args):
    """Allele-specific methylation per (SNV, cytosine): for every SNV of `vcf` and every cytosine of `asm_context` on the reads
    that cover the SNV, the methylated / unmethylated calls of the reads that carry the reference allele against those of the
    reads that carry the alternative one (meth_ref, unmeth_ref, meth_alt, unmeth_alt), their betas, delta_beta = beta_alt -
    beta_ref and the two-sided Fisher exact p (what CGmapTools asm, MethPipe allelicmeth and DAMEfinder's SNP mode report).
    A read's allele is its base at the SNV, read bisulfite-aware (R/internal.R:642-666: C>T is told apart on '-' reads only,
    G>A on '+' reads only); reads without an allele there, and reads that generateMhlReport drops under
    max_outofcontext_beta, count nowhere.  Cytosines more than max_distance bases from the SNV (0: no limit) and those with
    fewer than max(min_coverage, 1) calls on either allele are left out.  vcf, vcf_style, bed, zero_based_bed: as for
    generateVcfReport.  Columns: ASM_COLUMNS -- name, REF, ALT of the SNV, snv (its row in the sorted VCF), rname, snv_pos,
    strand, pos, context, the four cells, beta_ref, beta_alt, delta_beta, p; with as_device the numeric columns alone, as
    device tensors.  Composes with adjustReport(rep, column="p").  The reference has no such report."""
    pairs, _ = _asm_tables(bam, vcf, vcf_style, bed, zero_based_bed, asm_context, max_distance, min_coverage, max_outofcontext_beta,
                           as_device, preprocess_args)
    return _deliver(pairs, report_file, gzip)


def generateAsmSnvReport(bam, vcf, vcf_style=None, bed=None, report_file=None, zero_based_bed=False, asm_context=None,
                         max_distance=0, min_coverage=1, max_outofcontext_beta=0.1, gzip=False, verbose=False, as_device=False,
                         **preprocess_args):
    """generateAsmReport pooled per SNV: one row per SNV of the sorted VCF with the reads that carry either allele or
    neither (reads_ref, reads_alt, reads_other), the number of its cytosines in generateAsmReport's table (npairs), the four
    cells summed over them, the pooled betas, delta_beta and the Fisher exact p of the pooled table (NaN ratios where a
    denominator is zero).  Same arguments.  Columns: ASM_SNV_COLUMNS; with as_device the numeric columns alone."""
    _, snvs = _asm_tables(bam, vcf, vcf_style, bed, zero_based_bed, asm_context, max_distance, min_coverage, max_outofcontext_beta,
                          as_device, preprocess_args)
    return _deliver(snvs, report_file, gzip)
