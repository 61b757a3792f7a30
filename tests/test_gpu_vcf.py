"""generateVcfReport on the GPU: the known answers of inst/unitTests/test_generateVcfReport.R
(tests/golden/vcf_expected.json), and the base-frequency kernel (epi_batch_base_freqs_dev / epi_get_base_freqs)
against a restatement of the reference's loop (src/rcpp_get_base_freqs.cpp:27-52) on seeded batches, counts exactly
equal, under every row layout."""
import csv
import ctypes as C
import json
import os

import numpy as np
import pytest

import synth_np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BAM = os.path.join(GOLDEN, "bam")
VCF = os.path.join(GOLDEN, "vcf")
NA = -2 ** 31
NT16_INT = np.array([4, 0, 1, 4, 2, 4, 4, 4, 3, 4, 4, 4, 4, 4, 4, 4])     # HTSlib's seq_nt16_int


@pytest.fixture(scope="module")
def ea():
    import epialleler_amd
    return epialleler_amd


def _want(expr):
    with open(os.path.join(GOLDEN, "vcf_expected.json")) as f:
        v = json.load(f)["values"][expr]
    return v["value"] if isinstance(v, dict) else v


def _by_allele(rep, col):
    keys = sorted(set(zip(rep["REF"].tolist(), rep["ALT"].tolist())))
    if col is None:
        return [int(((rep["REF"] == r) & (rep["ALT"] == a)).sum()) for r, a in keys]
    v = np.nan_to_num(np.asarray(rep[col], np.float64))
    return [float(v[(rep["REF"] == r) & (rep["ALT"] == a)].sum()) for r, a in keys]


def _amplicon(ea, **kw):
    return ea.generateVcfReport(os.path.join(BAM, "amplicon010meth.bam"), os.path.join(VCF, "amplicon.vcf.gz"),
                                vcf_style="NCBI", bed=os.path.join(BAM, "amplicon.bed"), **kw)


AMP = "amplicon.report[, sum(`%s`, na.rm=TRUE), by=.(REF,ALT)][order(REF, ALT)]$V1"
CAP = "capture.report[, sum(`%s`, na.rm=TRUE), by=.(REF,ALT)][order(REF, ALT)]$V1"


def test_amplicon_report(ea):
    rep = _amplicon(ea)
    assert (rep.nrow, len(rep)) == tuple(_want("dim(amplicon.report)"))
    assert list(rep.keys()) == ["name", "seqnames", "range", "REF", "ALT", "M+Ref", "U+Ref", "M-Ref", "U-Ref", "M+Alt",
                                "U+Alt", "M-Alt", "U-Alt", "SumRef", "SumAlt", "FEp+", "FEp-"]
    assert np.nansum(rep["FEp+"]) == pytest.approx(_want("sum(amplicon.report$`FEp+`, na.rm=TRUE)"), abs=1e-8)
    assert np.nansum(rep["FEp-"]) == pytest.approx(_want("sum(amplicon.report$`FEp-`, na.rm=TRUE)"), abs=1e-8)
    assert np.nansum(rep["SumRef"]) == _want("sum(amplicon.report$SumRef, na.rm=TRUE)")
    assert np.nansum(rep["SumAlt"]) == _want("sum(amplicon.report$SumAlt, na.rm=TRUE)")
    assert _by_allele(rep, None) == _want("amplicon.report[, .N, by=.(REF,ALT)][order(REF, ALT)]$N")
    for col in ("M+Ref", "U+Ref", "M-Ref", "U-Ref", "M+Alt", "U+Alt", "M-Alt", "U-Alt", "SumRef", "SumAlt"):
        assert _by_allele(rep, col) == _want(AMP % col), col
    assert _by_allele(rep, "range") == _want("amplicon.report[, sum(as.numeric(range)), by=.(REF,ALT)][order(REF,ALT)]$V1")
    assert rep.levels["seqnames"][rep["seqnames"][0] - 1] == "chr17"
    assert np.all(np.diff(rep["range"]) >= 0)


def test_capture_report_and_preread_vcf(ea):
    vcf = ea.readVcf(os.path.join(VCF, "capture.vcf.gz"))
    rep = ea.generateVcfReport(os.path.join(BAM, "capture.bam"), vcf, bed=os.path.join(BAM, "capture.bed"))
    nobed = ea.generateVcfReport(os.path.join(BAM, "capture.bam"), vcf, bed=None)
    assert (rep.nrow, len(rep)) == tuple(_want("dim(capture.report)"))
    assert np.nansum(rep["FEp+"]) == pytest.approx(_want("sum(capture.report$`FEp+`, na.rm=TRUE)"), abs=1e-8)
    assert np.nansum(rep["FEp-"]) == pytest.approx(_want("sum(capture.report$`FEp-`, na.rm=TRUE)"), abs=1e-8)
    assert _by_allele(rep, None) == _want("capture.report[, .N, by=.(REF,ALT)][order(REF, ALT)]$N")
    for col in ("M+Ref", "U+Ref", "M-Ref", "U-Ref", "SumRef"):
        assert _by_allele(rep, col) == _want(CAP % col), col
    alt = sum(np.nan_to_num(rep[c]) for c in ("M+Alt", "U+Alt", "M-Alt", "U-Alt", "SumAlt"))
    keys = sorted(set(zip(rep["REF"].tolist(), rep["ALT"].tolist())))
    assert [float(alt[(rep["REF"] == r) & (rep["ALT"] == a)].sum()) for r, a in keys] == \
        _want("capture.report[, sum(`M+Alt`, `U+Alt`, `M-Alt`, `U-Alt`, `SumAlt`, na.rm=TRUE), by=.(REF,ALT)][order(REF, ALT)]$V1")
    assert _by_allele(rep, "range") == _want("capture.report[, sum(as.numeric(range)), by=.(REF,ALT)][order(REF,ALT)]$V1")
    assert list(rep.keys()) == list(nobed.keys())            # identical(capture.report, capture.report.nobed)
    for k in rep:
        a, b = np.asarray(rep[k]), np.asarray(nobed[k])
        assert np.array_equal(a, b, equal_nan=(a.dtype.kind == "f")), k


def test_nothreshold_and_quality(ea):
    rep = _amplicon(ea, threshold_reads=False)
    assert rep.nrow == _want("dim(nothreshold.report)")[0]
    assert np.nansum(rep["FEp+"]) == pytest.approx(_want("sum(nothreshold.report$`FEp+`, na.rm=TRUE)"), abs=1e-8)
    assert np.nansum(rep["FEp-"]) == pytest.approx(_want("sum(nothreshold.report$`FEp-`, na.rm=TRUE)"), abs=1e-8)
    q = _amplicon(ea, threshold_reads=False, min_mapq=30, min_baseq=20)
    assert np.nansum(q["FEp+"]) == pytest.approx(_want("sum(quality.report$`FEp+`, na.rm=TRUE)"), abs=1e-8)
    assert np.nansum(q["FEp-"]) == pytest.approx(_want("sum(quality.report$`FEp-`, na.rm=TRUE)"), abs=1e-8)
    assert np.nansum(q["SumRef"]) == _want("sum(quality.report$SumRef, na.rm=TRUE)")
    assert np.nansum(q["SumAlt"]) == _want("sum(quality.report$SumAlt, na.rm=TRUE)")


def test_amplicon_without_bed_raises(ea):
    with pytest.raises(ValueError, match="seqlevels styles"):
        ea.generateVcfReport(os.path.join(BAM, "amplicon010meth.bam"), os.path.join(VCF, "amplicon.vcf.gz"),
                             vcf_style="NCBI", bed=None, threshold_reads=False)


def test_report_file(ea, tmp_path):
    out = tmp_path / "vcf.tsv"
    assert _amplicon(ea, report_file=str(out)) is None
    with open(out) as f:
        rows = list(csv.reader(f, delimiter="\t"))
    assert len(rows) == 57 and all(len(r) == 17 for r in rows)
    assert rows[0][:5] == ["name", "seqnames", "range", "REF", "ALT"] and rows[0][-2:] == ["FEp+", "FEp-"]
    rep = _amplicon(ea)
    assert [r[1] for r in rows[1:]] == ["chr17"] * 56
    assert [int(r[2]) for r in rows[1:]] == rep["range"].tolist()
    assert sum(float(r[13]) for r in rows[1:]) == 5282


# ---- the kernel against the reference's loop -------------------------------------------------------------------------

def restated_base_freqs(t, pass_, chr_, pos):
    """src/rcpp_get_base_freqs.cpp:27-52 on sorted rows and sorted non-NA sites, written as the loop it is: for every
    read, the sites from the first one not before the read's start, while they are not past its end."""
    res = np.zeros((len(chr_), 20), np.int64)
    xm, off, rname, strand, start = t["xm"], t["off"], t["rname"], t["strand"], t["start"]
    cur = 0
    for x in range(len(start)):
        r, s, e = int(rname[x]), int(start[x]), int(start[x]) + int(off[x + 1] - off[x]) - 1
        for i in range(cur, len(pos)):
            c, p = int(chr_[i]), int(pos[i])
            if c < r or (c == r and p < s):
                cur = i
                continue
            if c > r or (c == r and p > e):
                break
            if strand[x] not in (1, 2):                      # the placeholder row: no strand to count it on
                continue
            res[i, NT16_INT[xm[off[x] + p - s] >> 4] + (int(strand[x]) - 1) * 5 + (10 if pass_[x] != 0 else 0)] += 1
    return res


def restated_base_freqs_fast(t, pass_, chr_, pos):
    """The same counts, vectorised (every read x every site inside it), for the large batches."""
    res = np.zeros((len(chr_), 20), np.int64)
    key = chr_.astype(np.int64) * 2 ** 32 + pos.astype(np.int64)
    ln = np.diff(t["off"])
    k0 = t["rname"].astype(np.int64) * 2 ** 32 + t["start"]
    lo = np.searchsorted(key, k0, side="left")
    hi = np.searchsorted(key, k0 + ln, side="left")
    ok = (t["strand"] == 1) | (t["strand"] == 2)
    cnt = np.where(ok, hi - lo, 0)
    rows = np.repeat(np.arange(len(cnt)), cnt)
    first = np.repeat(lo, cnt)
    csum = np.concatenate([[0], np.cumsum(cnt)])
    site = first + (np.arange(rows.size) - np.repeat(csum[:-1], cnt))
    byte = t["xm"][t["off"][rows] + pos[site] - t["start"][rows]]
    col = NT16_INT[byte >> 4] + (t["strand"][rows] - 1) * 5 + np.where(np.asarray(pass_)[rows] != 0, 10, 0)
    np.add.at(res, (site, col), 1)
    return res


def _sites(rng, n_chr, span, every, na_frac=0.0, dup_frac=0.1):
    """sorted sites (code, pos) with duplicated positions (multi-ALT records)"""
    chr_, pos = [], []
    for c in range(1, n_chr + 1):
        p = np.sort(rng.choice(np.arange(1, span + 1), size=max(span // every, 1), replace=False))
        d = p[rng.random(p.size) < dup_frac]
        p = np.sort(np.concatenate([p, d]))
        chr_.append(np.full(p.size, c, np.int32))
        pos.append(p.astype(np.int32))
    chr_, pos = np.concatenate(chr_), np.concatenate(pos)
    return chr_, pos


def _cases():
    rng = np.random.default_rng(2024)
    out = {}
    t = synth_np.random_templates(rng, 4000, 0, 400, 3, 20000)            # ragged, three chromosomes, empty rows
    t["strand"][rng.choice(4000, 40, replace=False)] = 0                 # placeholder rows count nowhere
    out["ragged"] = (t, _sites(rng, 4, 20500, 25))
    t = synth_np.random_templates(rng, 6000, 150, 150, 1, 3)             # > 4096 rows over one site
    t["start"][:] = np.sort(rng.integers(1, 4, 6000)).astype(np.int32)
    out["pileup"] = (t, (np.array([1, 1, 1], np.int32), np.array([100, 100, 152], np.int32)))
    t = synth_np.random_templates(rng, 400, 9000, 10000, 2, 60000)       # 10 kb reads: windows beyond the LDS budget
    out["long"] = (t, _sites(rng, 2, 70000, 6))
    t = synth_np.generate(n_total=3000, read_len=300, n_chr=2, depth=20, seed=9, gap_from=120, gap_len=60)
    out["gapped"] = (t, _sites(rng, 3, int(t["start"].max()) + 400, 7))  # sites in the gaps count as N
    return out


def _bams(ea, t):
    import torch
    yield "uploaded", ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"])
    nb = int(t["off"][-1])
    for realign in (False, True):
        xm = torch.full(((nb + 15) // 16 * 16 + 16,), 0xFB, dtype=torch.uint8, device="cuda:0")
        xm[:nb] = torch.from_numpy(t["xm"]).cuda()
        yield ("realigned" if realign else "adopted"), ea.ProcessedBam.from_device(
            xm, nb, torch.from_numpy(t["off"]).cuda(), torch.from_numpy(t["rname"]).cuda(),
            torch.from_numpy(t["strand"]).cuda(), torch.from_numpy(t["start"]).cuda(), realign=realign)


def _dropin(ea, t, pass_, chr_, pos):
    lib = ea._lib.load()
    n, m = len(t["start"]), len(chr_)
    out = np.empty((20, m), np.float64)
    pass_ = np.ascontiguousarray(pass_, np.int32)
    chr_, pos = np.ascontiguousarray(chr_, np.int32), np.ascontiguousarray(pos, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data) if a.size else None
    rc = lib.epi_get_base_freqs(p(t["xm"]), p(t["off"]), n, p(t["rname"]), p(t["strand"]), p(t["start"]), p(pass_),
                                p(chr_), p(pos), m, p(out))
    return rc, out.T


@pytest.mark.parametrize("case", ["ragged", "pileup", "long", "gapped"])
def test_base_freqs_parity(ea, case):
    t, (chr_, pos) = _cases()[case]
    rng = np.random.default_rng(len(case))
    n = len(t["start"])
    pass_ = rng.integers(0, 2, n).astype(np.int32)
    pass_[rng.random(n) < 0.05] = NA                                      # R's NA: TRUE
    want = restated_base_freqs_fast(t, pass_, chr_, pos)
    if case in ("ragged", "pileup"):
        assert np.array_equal(want, restated_base_freqs(t, pass_, chr_, pos))
    assert want.sum() > 0
    if case == "gapped":
        assert want[:, [4, 9, 14, 19]].sum() > 0                          # N: the filler between mates
    # the caller's order with NA-coded sites: the drop-in and the resident wrapper put them back in place
    perm = rng.permutation(len(chr_))
    na = rng.random(len(chr_)) < 0.1
    c2 = np.where(na, NA, chr_)[perm]
    p2 = pos[perm]
    want2 = np.where(na[:, None], 0, want)[perm]
    for layout, bam in _bams(ea, t):
        got = ea.rcpp_get_base_freqs(bam, pass_, chr_, pos)
        assert np.array_equal(got, want), (case, layout)
        got2 = ea.rcpp_get_base_freqs(bam, pass_, c2, p2)
        assert np.array_equal(got2, want2), (case, layout)
        bam.close()
    srt = np.flatnonzero(~na)
    order = np.lexsort((pos, chr_))
    rc, got = _dropin(ea, t, pass_, np.where(na, NA, chr_)[order], pos[order])
    assert rc == 0 and np.array_equal(got, np.where(na[:, None], 0, want)[order]), case
    assert srt.size


def test_base_freqs_unsorted_sites(ea):
    from epialleler_amd._lib import EPI_ERR_UNSORTED, EpihipError
    t, (chr_, pos) = _cases()["ragged"]
    pass_ = np.ones(len(t["start"]), np.int32)
    c2, p2 = chr_.copy(), pos.copy()
    p2[[10, 11]] = p2[[11, 10]]
    rc, _ = _dropin(ea, t, pass_, c2, p2)
    assert rc == EPI_ERR_UNSORTED
    rc, got = _dropin(ea, t, pass_, np.where(np.arange(len(c2)) == 10, NA, c2), p2)   # an NA-coded site is not in the order
    assert rc == 0
    import torch
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"])
    lib = ea._lib.load()
    d_c, d_p = torch.from_numpy(c2).cuda(), torch.from_numpy(p2).cuda()
    cnt = torch.empty(20 * len(c2), dtype=torch.int32, device="cuda:0")
    rc = lib.epi_batch_base_freqs_dev(bam.batch(), None, C.c_void_p(d_c.data_ptr()), C.c_void_p(d_p.data_ptr()), len(c2),
                                      C.c_void_p(cnt.data_ptr()), None)
    assert rc == EPI_ERR_UNSORTED
    with pytest.raises(EpihipError):
        u = dict(t)
        u["start"] = t["start"][::-1].copy()
        u["rname"] = np.ones_like(t["rname"])
        ea.rcpp_get_base_freqs(ea.ProcessedBam.from_arrays(u["xm"], u["off"], u["rname"], u["strand"], u["start"]),
                               None, chr_, pos)
    bam.close()
