"""generateVcfReport's host half (no GPU): the VCF reader (epi_read_vcf + readVcf's BED filter and seqlevels styles),
the Fisher exact test (epi_fisher_exact) and the report assembly from a base-frequency matrix.  Known answers from
inst/unitTests/test_generateVcfReport.R (tests/golden/vcf_expected.json): the values that depend on the VCF alone."""
import gzip
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
VCF = os.path.join(GOLDEN, "vcf")
NA = -2 ** 31


@pytest.fixture(scope="module")
def ea():
    import epialleler_amd
    return epialleler_amd


def _want(expr):
    with open(os.path.join(GOLDEN, "vcf_expected.json")) as f:
        return json.load(f)["values"][expr]


def _by_allele(v, values=None):
    """data.table's [, f, by=.(REF,ALT)][order(REF, ALT)]: one entry per (REF, ALT) pair present"""
    keys = sorted(set(zip(v.ref.tolist(), v.alt.tolist())))
    if values is None:
        return [int(((v.ref == r) & (v.alt == a)).sum()) for r, a in keys]
    return [int(np.asarray(values, np.int64)[(v.ref == r) & (v.alt == a)].sum()) for r, a in keys]


def test_amplicon_vcf_with_bed(ea):
    v = ea.readVcf(os.path.join(VCF, "amplicon.vcf.gz"), vcf_style="NCBI", bed=os.path.join(GOLDEN, "bam", "amplicon.bed"))
    assert len(v) == _want("dim(amplicon.report)")[0] == 56
    assert _by_allele(v) == _want("amplicon.report[, .N, by=.(REF,ALT)][order(REF, ALT)]$N")
    assert _by_allele(v, v.pos) == _want("amplicon.report[, sum(as.numeric(range)), by=.(REF,ALT)][order(REF,ALT)]$V1")
    assert set(v.seqnames) == {"chr17"}                     # "17" in the file, back in the BED's style
    assert list(v.names[:3]) == ["rs546660277", "rs574263814", "rs8176076"]


def test_amplicon_vcf_without_bed_keeps_file_names(ea):
    v = ea.readVcf(os.path.join(VCF, "amplicon.vcf.gz"))
    assert set(v.seqnames) == {"17"} and len(v) > 56


def test_capture_vcf(ea):
    v = ea.readVcf(os.path.join(VCF, "capture.vcf.gz"))
    assert len(v) == _want("dim(capture.report)")[0] == 26292
    assert _by_allele(v) == _want("capture.report[, .N, by=.(REF,ALT)][order(REF, ALT)]$N")
    assert _by_allele(v, v.pos) == _want("capture.report[, sum(as.numeric(range)), by=.(REF,ALT)][order(REF,ALT)]$V1")
    assert v.levels[:3] == ["chr1", "chr2", "chr3"] and len(v.levels) == 23     # the ##contig lines


def test_plain_text_vcf_and_expansion(ea, tmp_path):
    # a plain VCF with multi-ALT records, an indel, a missing ID, no ##contig lines (first appearance) and CRLF ends
    lines = ["##fileformat=VCFv4.2", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO",
             "chrB\t10\trs1\tG\tA,T\t.\t.\t.", "chrA\t5\t.\tC\tT\t.\t.\t.", "chrB\t12\trs2\tGCT\tG\t.\t.\t.",
             "chrB\t14\trs3\tA\tAT,C\t.\t.\t.", "chrA\t7\trs4\tT\t.\t.\t.\t."]
    p = tmp_path / "x.vcf"
    p.write_bytes(("\r\n".join(lines) + "\r\n").encode())
    v = ea.readVcf(str(p))
    assert v.levels == ["chrB", "chrA"]
    assert list(v.seqnames) == ["chrB", "chrB", "chrA", "chrB"]
    assert v.pos.tolist() == [10, 10, 5, 14]
    assert v.ref.tolist() == ["G", "G", "C", "A"] and v.alt.tolist() == ["A", "T", "T", "C"]
    assert list(v.names) == ["rs1", "rs1", "chrA:5_C/T", "rs3"]     # (the "." naming rule is not pinned by a fixture)
    g = tmp_path / "x.vcf.gz"                                 # plain gzip (not BGZF): the same rows
    with gzip.open(str(g), "wb") as f:
        f.write(p.read_bytes())
    w = ea.readVcf(str(g))
    assert w.pos.tolist() == v.pos.tolist() and list(w.names) == list(v.names)


def test_styles(ea):
    from epialleler_amd import vcf as V
    assert V._rename("17", "UCSC") == "chr17" and V._rename("MT", "UCSC") == "chrM"
    assert V._rename("chr17", "NCBI") == "17" and V._rename("chrM", "Ensembl") == "MT"
    assert V._style_of(["chr1", "chr2"]) == "UCSC" and V._style_of(["1", "X"]) == "NCBI"
    with pytest.raises(ValueError):
        V._rename("1", "RefSeq")


def test_missing_vcf_raises(ea, tmp_path):
    with pytest.raises(ea.EpihipError):
        ea.readVcf(str(tmp_path / "none.vcf"))


def _fisher_tables():
    rng = np.random.default_rng(7)
    T = []
    for k in range(10000):
        kind = k % 5
        if kind == 0:
            t = rng.integers(0, 12, 4)                       # small
        elif kind == 1:
            t = rng.integers(0, 30000, 4)                    # large
        elif kind == 2:                                     # skewed
            t = np.array([rng.integers(0, 5), rng.integers(0, 30000), rng.integers(0, 30), rng.integers(0, 20000)])
        elif kind == 3:                                     # exact ties: the mirrored table is equally probable
            a, b = rng.integers(0, 40, 2)
            t = np.array([a, b, b, a])
        else:
            t = rng.integers(0, 300, 4)
        T.append(t)
    return np.asarray(T, np.int32)


def test_fisher_exact_matches_scipy(ea):
    stats = pytest.importorskip("scipy.stats")
    T = _fisher_tables()
    p = ea.rcpp_fep({"a": T[:, 0], "b": T[:, 1], "c": T[:, 2], "d": T[:, 3]}, ("a", "b", "c", "d"))
    q = np.array([stats.fisher_exact([[a, b], [c, d]], alternative="two-sided")[1] for a, b, c, d in T.tolist()])
    ok = q > 1e-280                                          # (below that both underflow differently)
    assert ok.sum() > 8000
    np.testing.assert_allclose(p[ok], q[ok], rtol=1e-9, atol=0)
    assert np.all(p[~ok] < 1e-270)
    assert np.all((p >= 0) & (p <= 1))


def test_fisher_exact_known_and_na(ea):
    cells = np.array([[3, 1, 1, 3], [0, 0, 0, 0], [5, 0, 0, 5], [NA, 1, 2, 3], [1, 2, NA, 3], [10, 10, 10, 10]], np.int32)
    p = ea.rcpp_fep({k: cells[:, i] for i, k in enumerate("abcd")}, tuple("abcd"))
    assert p[0] == pytest.approx(0.4857142857142857, rel=1e-12)     # fisher.test(matrix(c(3,1,1,3), 2))
    assert p[1] == 1.0
    assert p[2] == pytest.approx(2 / 252, rel=1e-12)
    assert np.isnan(p[3]) and np.isnan(p[4])
    assert p[5] == 1.0
    f = ea.rcpp_fep({"a": [1.0, np.nan], "b": [2.0, 1.0], "c": [3.0, 1.0], "d": [4.0, 1.0]}, tuple("abcd"))   # NA_real_ columns
    assert np.isfinite(f[0]) and np.isnan(f[1])


# ---- report assembly: an independent restatement of R/internal.R:642-669 --------------------------------------------

def _restated_report(freqs, ref, alt):
    # columns of the matrix, R/internal.R:629-633
    names = ["U+A", "U+C", "U+G", "U+T", "U+N", "U-A", "U-C", "U-G", "U-T", "U-N",
             "M+A", "M+C", "M+G", "M+T", "M+N", "M-A", "M-C", "M-G", "M-T", "M-N"]
    F = {k: freqs[:, i] for i, k in enumerate(names)}
    n = freqs.shape[0]
    out = {k: np.full(n, np.nan) for k in ("M+Ref", "U+Ref", "M-Ref", "U-Ref", "M+Alt", "U+Alt", "M-Alt", "U-Alt")}
    NAv = np.full(n, np.nan)

    def put(sel, mpr, upr, mmr, umr, mpa, upa, mma, uma):
        for k, v in zip(("M+Ref", "U+Ref", "M-Ref", "U-Ref", "M+Alt", "U+Alt", "M-Alt", "U-Alt"),
                        (mpr, upr, mmr, umr, mpa, upa, mma, uma)):
            out[k][sel] = v[sel]
    r, a = np.asarray(ref), np.asarray(alt)
    put((r == "A") & (a == "C"), F["M+A"], F["U+A"], F["M-A"], F["U-A"], F["M+C"] + F["M+T"], F["U+C"] + F["U+T"], F["M-C"], F["U-C"])
    put((r == "A") & (a == "T"), F["M+A"], F["U+A"], F["M-A"], F["U-A"], F["M+T"], F["U+T"], F["M-T"], F["U-T"])
    put((r == "A") & (a == "G"), F["M+A"], F["U+A"], NAv, NAv, F["M+G"], F["U+G"], NAv, NAv)
    put((r == "C") & (a == "A"), F["M+C"] + F["M+T"], F["U+C"] + F["U+T"], F["M-C"], F["U-C"], F["M+A"], F["U+A"], F["M-A"], F["U-A"])
    put((r == "C") & (a == "T"), NAv, NAv, F["M-C"], F["U-C"], NAv, NAv, F["M-T"], F["U-T"])
    put((r == "C") & (a == "G"), F["M+C"] + F["M+T"], F["U+C"] + F["U+T"], F["M-C"], F["U-C"], F["M+G"], F["U+G"],
        F["M-A"] + F["M-G"], F["U-A"] + F["U-G"])
    put((r == "T") & (a == "A"), F["M+T"], F["U+T"], F["M-T"], F["U-T"], F["M+A"], F["U+A"], F["M-A"], F["U-A"])
    put((r == "T") & (a == "C"), NAv, NAv, F["M-T"], F["U-T"], NAv, NAv, F["M-C"], F["U-C"])
    put((r == "T") & (a == "G"), F["M+T"], F["U+T"], F["M-T"], F["U-T"], F["M+G"], F["U+G"], F["M-A"] + F["M-G"], F["U-A"] + F["U-G"])
    put((r == "G") & (a == "A"), F["M+G"], F["U+G"], NAv, NAv, F["M+A"], F["U+A"], NAv, NAv)
    put((r == "G") & (a == "C"), F["M+G"], F["U+G"], F["M-A"] + F["M-G"], F["U-A"] + F["U-G"], F["M+C"] + F["M+T"],
        F["U+C"] + F["U+T"], F["M-C"], F["U-C"])
    put((r == "G") & (a == "T"), F["M+G"], F["U+G"], F["M-A"] + F["M-G"], F["U-A"] + F["U-G"], F["M+T"], F["U+T"], F["M-T"], F["U-T"])
    ref4 = np.stack([out["M+Ref"], out["U+Ref"], out["M-Ref"], out["U-Ref"]], 1)
    alt4 = np.stack([out["M+Alt"], out["U+Alt"], out["M-Alt"], out["U-Alt"]], 1)
    out["SumRef"] = np.where(np.isnan(ref4), 0, ref4).sum(1)
    out["SumAlt"] = np.where(np.isnan(alt4), 0, alt4).sum(1)
    return out


def test_report_assembly_matches_restatement(ea):
    from epialleler_amd import vcf as V
    rng = np.random.default_rng(3)
    bases = list("ACGTN")
    pairs = [(r, a) for r in bases for a in bases]             # the 12 SNV pairs, and 13 that get NA everywhere
    n = 2000
    k = rng.integers(0, len(pairs), n)
    ref = np.array([pairs[i][0] for i in k])
    alt = np.array([pairs[i][1] for i in k])
    freqs = rng.integers(0, 50, (n, 20)).astype(np.float64)
    got = V.base_freq_columns(freqs, ref, alt)
    want = _restated_report(freqs, ref, alt)
    for c in want:
        np.testing.assert_array_equal(got[c], want[c], err_msg=c)
    unknown = np.array([(r, a) not in V._ALLELE_TABLE for r, a in zip(ref, alt)])
    assert unknown.any() and np.isnan(got["M+Ref"][unknown]).all() and (got["SumRef"][unknown] == 0).all()
    p = ea.rcpp_fep(got, ("M+Ref", "U+Ref", "M+Alt", "U+Alt"))
    assert np.array_equal(np.isnan(p), np.isnan(got["M+Ref"]) | np.isnan(got["M+Alt"]))
