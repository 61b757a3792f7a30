"""generateBedReport / generateAmpliconReport / generateCaptureReport / generateBedEcdf through the GPU
path.  On the reference's two fixtures: the known-answer values of the reference's tests
(inst/unitTests/test_generateBedReport.R, test_generateBedEcdf.R) -- they pin rcpp_threshold_reads,
rcpp_get_xm_beta and rcpp_match_amplicon/_capture.  On the synthetic batch of helpers.match_templates(): every
column of the report and every ECDF against plain restatements (helpers.bed_report_np on helpers.threshold_np and
helpers.match_target_np; helpers.ecdf_np on helpers.beta_np), for both bed types, with and without an NA row, with
regions that no read hits, at ties of the step function, and for bed_rows in any order.  The matching kernel itself
(LDS chunks, first-match order, both comparison operators at and around their limits, batch layouts) is covered in
tests/test_gpu_match_target.py, readBed and the restatements in tests/test_bed_host.py."""
import os

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu
BAM = os.path.join(H.GOLDEN, "bam")
S = "generateBedReport"


def test_amplicon_and_capture_reports():
    import epialleler_amd as ea
    amp_bam, amp_bed = os.path.join(BAM, "amplicon010meth.bam"), os.path.join(BAM, "amplicon.bed")
    rep = ea.generateAmpliconReport(amp_bam, amp_bed)
    assert [rep.nrow, len(rep)] == H.expected_values(S, "dim(amplicon.report)")                     # c(5, 9)
    assert [int(np.nansum(rep["nreads-"]))] == H.expected_values(S, "sum(amplicon.report$`nreads-`)")
    assert [int(np.nansum(rep["nreads+"]) + np.nansum(rep["nreads-"]))] == H.expected_values(S, "sum(amplicon.report[")
    np.testing.assert_allclose(rep["VEF"], H.expected_values(S, "amplicon.report$VEF"), rtol=1e-9)
    assert list(rep.keys()) == ["seqnames", "start", "end", "width", "strand", "amplicon", "nreads+", "nreads-", "VEF"]
    assert rep["seqnames"][-1] is None and rep["amplicon"][0] == "CpG00-13"
    nothr = ea.generateAmpliconReport(amp_bam, amp_bed, threshold_reads=False)
    assert [nothr.nrow, len(nothr)] == H.expected_values(S, "dim(nothreshold.report)") and np.all(np.isnan(nothr["VEF"]))
    q = ea.generateAmpliconReport(amp_bam, amp_bed, min_mapq=30, min_baseq=20)
    assert [int(np.nansum(q["nreads-"]))] == H.expected_values(S, "sum(quality.report$`nreads-`)")
    assert [int(np.nansum(q["nreads+"]) + np.nansum(q["nreads-"]))] == H.expected_values(S, "sum(quality.report[")
    np.testing.assert_allclose(q["VEF"], H.expected_values(S, "quality.report$VEF"), rtol=1e-9)
    assert np.sum(rep["VEF"][:4]) == np.sum(q["VEF"][:4]) and rep["VEF"][4] != q["VEF"][4]
    cap = ea.generateCaptureReport(os.path.join(BAM, "capture.bam"), os.path.join(BAM, "capture.bed"))
    assert [cap.nrow, len(cap)] == H.expected_values(S, "dim(capture.report)")                       # c(565, 9)
    assert [int(np.nansum(cap["nreads-"]))] == H.expected_values(S, "sum(capture.report$`nreads-`")
    assert [int(np.nansum(cap["nreads+"]) + np.nansum(cap["nreads-"]))] == H.expected_values(S, "sum(capture.report[")
    same = ea.generateBedReport(os.path.join(BAM, "capture.bam"), os.path.join(BAM, "capture.bed"), bed_type="capture")
    for k in cap:
        a, b = cap[k], same[k]
        assert np.array_equal(a, b) or (a.dtype.kind == "f" and np.array_equal(a, b, equal_nan=True)), k


def test_matching_equals_restatement():
    import epialleler_amd as ea
    from epialleler_amd import bed as B
    for name, bedf, typ in (("amplicon010meth.bam", "amplicon.bed", "amplicon"), ("capture.bam", "capture.bed", "capture")):
        t = H.bam(name)
        bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"], t["levels"])
        bd = ea.readBed(os.path.join(BAM, bedf))
        got = B._match_target(bam, bd, typ, 1, 1).cpu().numpy()
        codes = np.asarray([t["levels"].index(c) + 1 for c in bd.chrom], np.int64)
        want = H.match_target_loop(t, (codes, bd.start, bd.end), typ == "capture", 1)     # src/rcpp_match_target.cpp:30-44 / 63-76
        assert np.array_equal(got, want), name


def test_bed_ecdf():
    import epialleler_amd as ea
    amp_bam, amp_bed = os.path.join(BAM, "amplicon010meth.bam"), os.path.join(BAM, "amplicon.bed")
    e = ea.generateBedEcdf(amp_bam, amp_bed, bed_rows=[1, 2])
    vals = [f(0.5) for d in e.values() for f in (d["context"], d["out.of.context"])]
    np.testing.assert_allclose(vals, [0.916666666667, 1, 0.885245901639, 1], atol=1e-8)           # test_generateBedEcdf.R:8-12
    assert list(e.keys()) == ["chr17:43125624-43126026", "chr17:43125270-43125640"]
    e = ea.generateBedEcdf(amp_bam, amp_bed, bed_rows=None, min_mapq=30, min_baseq=20)
    vals = [f(0.5) for d in e.values() for f in (d["context"], d["out.of.context"])]
    np.testing.assert_allclose(vals, [0.916666666667, 1, 0.885245901639, 1, 0.946236559140, 1, 0.892857142857, 1,
                                      0.868131868132, 1], atol=1e-8)                                   # :21-26
    assert list(e.keys())[-1] is None


def test_bed_report_file_has_fwrite_na_fields(tmp_path):
    """generateBedReport(report.file=...): the file data.table::fwrite would write -- NA fields empty (the last row
    collects the reads that match no amplicon: NA seqnames/start/end/width/strand/name), counts without a fraction."""
    import epialleler_amd as ea
    amp_bam, amp_bed = os.path.join(BAM, "amplicon010meth.bam"), os.path.join(BAM, "amplicon.bed")
    out = tmp_path / "amp.tsv"
    assert ea.generateAmpliconReport(amp_bam, amp_bed, report_file=str(out)) is None
    rep = ea.generateAmpliconReport(amp_bam, amp_bed)
    lines = out.read_text().rstrip("\n").split("\n")
    assert lines[0].split("\t") == list(rep.keys()) and len(lines) == 1 + rep.nrow
    last = lines[-1].split("\t")
    assert last[:6] == [""] * 6 and last[6] == "%d" % rep["nreads+"][-1] and last[7] == "%d" % rep["nreads-"][-1]
    assert float(last[8]) == pytest.approx(rep["VEF"][-1], rel=1e-14)
    first = lines[1].split("\t")
    assert first[0] == rep["seqnames"][0] and first[1] == "%d" % rep["start"][0] and first[4] == "*" and "nan" not in out.read_text().lower()
    nothr = tmp_path / "nothr.tsv"
    ea.generateAmpliconReport(amp_bam, amp_bed, threshold_reads=False, report_file=str(nothr))
    assert all(l.split("\t")[8] == "" for l in nothr.read_text().rstrip("\n").split("\n")[1:])      # VEF is NA without thresholding


def test_placeholder_template_is_harmless():
    """A paired-end file without a usable pair gives the reference's placeholder template (strand code 0, no bases,
    src/rcpp_read_bam.cpp:155): reports are empty tables, the BED report counts it on neither strand."""
    import epialleler_amd as ea
    t = {"xm": np.zeros(0, np.uint8), "off": np.zeros(2, np.int64), "rname": np.ones(1, np.int32),
         "strand": np.zeros(1, np.int32), "start": np.ones(1, np.int32)}
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"], levels=["chr17"])
    assert ea.generateCytosineReport(bam).nrow == 0 and ea.generateMhlReport(bam).nrow == 0
    bed = ea.Bed(["chr17"], [1], [100])
    rep = ea.generateBedReport(bam, bed, bed_type="capture")
    assert rep.nrow == 1 and np.isnan(rep["nreads+"][0]) and np.isnan(rep["nreads-"][0])
    bam.close()


# ---- the synthetic batch of the kernel tests: every column and every ECDF against a restatement -------------------------

REPORT_COLS = ["seqnames", "start", "end", "width", "strand", "name", "score", "nreads+", "nreads-", "VEF"]


@pytest.fixture(scope="module")
def ea():
    import epialleler_amd
    return epialleler_amd


@pytest.fixture(scope="module")
def synth_bam(ea):
    t = H.match_templates()
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"], H.MATCH_LEVELS)
    yield bam
    bam.close()


def _small_bed(ea, spanning=False):
    """40 unsorted rows with two extra columns: wide random ranges on c1..c3, on c4 (a chromosome without reads) and on
    chrUn (not among the BAM's levels), 15 rows that are a read's own range, one duplicated row.  spanning: the first
    three rows cover c1, c2 and c3 whole, so that every read touches one of them."""
    t = H.match_templates()
    rng = np.random.default_rng(7)
    lens = np.diff(t["off"])
    chrom = [("c1", "c2", "c3", "c4", "chrUn")[i] for i in rng.choice(5, size=40, p=[0.3, 0.3, 0.3, 0.05, 0.05])]
    chrom[5], chrom[6] = "c4", "chrUn"
    start = rng.integers(1, 58000, size=40).astype(np.int64)
    end = start + rng.integers(200, 2500, size=40)
    rows = rng.choice(np.arange(7, 40), size=15, replace=False)
    reads = rng.choice(np.flatnonzero(lens > 0), size=15, replace=False)
    for r, x in zip(rows, reads):
        chrom[r], start[r], end[r] = "c%d" % t["rname"][x], t["start"][x], int(t["start"][x]) + int(lens[x]) - 1
    chrom[rows[1]], start[rows[1]], end[rows[1]] = chrom[rows[0]], start[rows[0]], end[rows[0]]
    if spanning:
        chrom[:3], start[:3], end[:3] = ["c1", "c2", "c3"], 1, 70000
    return ea.Bed(chrom, start, end, extra={"name": ["t%02d" % i for i in range(40)], "score": [str(3 * i) for i in range(40)]})


def _restated_match(bed, bed_type, param):
    return H.match_target_np(H.match_templates(), (H.match_codes(bed.chrom), bed.start, bed.end), bed_type == "capture", param)


# (shape, bed_type, tolerance or overlap, threshold_context, (min_context_sites, min_context_beta, max_outofcontext_beta)
#  or None for threshold_reads=False)
REPORT_CASES = [
    ("some", "amplicon", 5, "CG", (2, 0.5, 0.1)), ("some", "capture", 1, "CG", (2, 0.5, 0.1)),
    ("some", "capture", 1, "CHG", H.THRESHOLD_GRID[1]), ("some", "amplicon", 5, "CX", H.THRESHOLD_GRID[3]),
    ("some", "capture", 30, "CX", (2, 0.5, 0.1)), ("some", "amplicon", 0, "CHG", (2, 0.5, 0.1)),
    ("some", "capture", 1, "CG", (3, 0.5, 0.45)), ("some", "amplicon", 5, "CHG", (1, 0.6, 0.5)),     # about half the reads pass
    ("some", "capture", 1, "CG", None), ("some", "amplicon", 5, "CG", None),
    ("all", "capture", 0, "CG", (2, 0.5, 0.1)), ("all", "capture", -50, "CX", None),
    ("none", "amplicon", -1, "CG", (2, 0.5, 0.1)), ("none", "capture", 400, "CHG", H.THRESHOLD_GRID[1]),
]


@pytest.mark.parametrize("shape,bed_type,param,ctx,thr", REPORT_CASES)
def test_bed_report_equals_restatement(ea, synth_bam, shape, bed_type, param, ctx, thr):
    t = H.match_templates()
    bed = _small_bed(ea, spanning=(shape == "all"))
    nbed = len(bed)
    match = _restated_match(bed, bed_type, param)
    pass_ = np.ones(3001, np.int32) if thr is None else H.threshold_np(t["xm"], t["off"], H.cls4(ctx), *thr)
    r = H.bed_report_np(t, pass_, match, nbed)
    counted = int(np.isin(t["strand"], (1, 2)).sum())
    assert counted < 3001 and np.nansum(r["nreads+"]) + np.nansum(r["nreads-"]) == counted       # strand 0 counted nowhere
    hit = ~np.isnan(r["nreads+"][:nbed])
    if shape == "some":
        assert r["has_na"] and hit.any() and not hit.all()
        assert thr is None or 0 < pass_.sum() < 3001
    elif shape == "all":
        assert not r["has_na"] and hit[:3].all() and not hit[3:].any()
    else:
        assert r["has_na"] and not hit.any() and r["nreads+"][nbed] + r["nreads-"][nbed] == counted
    rows = np.arange(nbed + (1 if r["has_na"] else 0))
    obj = lambda v: np.asarray(list(v) + [None], object)[rows]
    num = lambda v: np.append(np.asarray(v, np.float64), np.nan)[rows]
    want = {"seqnames": obj(bed.chrom), "start": num(bed.start), "end": num(bed.end), "width": num(bed.end - bed.start + 1),
            "strand": obj(["*"] * nbed), "name": obj(bed.extra["name"]), "score": obj(bed.extra["score"]),
            "nreads+": r["nreads+"][rows], "nreads-": r["nreads-"][rows],
            "VEF": r["VEF"][rows] if thr is not None else np.full(rows.size, np.nan)}
    kw = {} if thr is None else dict(min_context_sites=thr[0], min_context_beta=thr[1], max_outofcontext_beta=thr[2])
    rep = ea.generateBedReport(synth_bam, bed, bed_type=bed_type, match_tolerance=param if bed_type == "amplicon" else -7,
                               match_min_overlap=param if bed_type == "capture" else 77, threshold_reads=thr is not None,
                               threshold_context=ctx, **kw)
    assert list(rep.keys()) == REPORT_COLS and rep.nrow == rows.size
    floats = ("start", "end", "width", "nreads+", "nreads-", "VEF")
    assert all(rep[k].dtype == np.float64 for k in floats)
    H.assert_reports_equal(rep, want, float_cols=floats)
    if r["has_na"]:
        assert all(rep[k][-1] is None for k in ("seqnames", "strand", "name", "score")) and np.isnan(rep["width"][-1])
    alias = (ea.generateAmpliconReport if bed_type == "amplicon" else ea.generateCaptureReport)(
        synth_bam, bed, bed_type="no such type", match_tolerance=param, match_min_overlap=param, threshold_reads=thr is not None,
        threshold_context=ctx, **kw)
    assert list(alias.keys()) == REPORT_COLS
    H.assert_reports_equal(alias, want, float_cols=floats)


def _check_ecdfs(got, bed, match, beta, keys):
    """got: generateBedEcdf's result; keys: the 1-based rows (None: the unmatched reads) it must hold, in order."""
    names = [None if r is None else "%s:%d-%d" % (bed.chrom[r - 1], bed.start[r - 1], bed.end[r - 1]) for r in keys]
    assert list(got.keys()) == names
    for r, name in zip(keys, names):
        sel = (match < 0) if r is None else (match == r)
        assert sel.any()
        assert list(got[name].keys()) == ["context", "out.of.context"]
        for which, f in got[name].items():
            x = np.sort(beta[which][sel])
            assert f.x.dtype == np.float64 and np.array_equal(f.x.view(np.uint64), x.view(np.uint64)), (name, which)
            ties = np.unique(x)
            q = np.concatenate([ties, np.nextafter(ties, -np.inf), np.nextafter(ties, np.inf), [-1.0, 0.0, 1.0, 2.0]])
            v = f(q)
            assert v.shape == q.shape and np.array_equal(v, H.ecdf_np(x, q)), (name, which)
            for s in (float(ties[0]), 0.5):
                assert isinstance(f(s), float) and f(s) == H.ecdf_np(x, s)[0], (name, which, s)


@pytest.mark.parametrize("ctx,bed_type,param", [("CG", "amplicon", 5), ("CxG", "capture", 1), ("CxG", "amplicon", 0),
                                                ("CG", "capture", 150)])
def test_bed_ecdf_equals_restatement(ea, synth_bam, ctx, bed_type, param):
    t = H.match_templates()
    bed = _small_bed(ea)
    match = _restated_match(bed, bed_type, param)
    c = H.CONTEXT_TO_BASES[ctx]
    beta = {"context": H.beta_np(t["xm"], t["off"], c["ctx_meth"], c["ctx_unmeth"]),
            "out.of.context": H.beta_np(t["xm"], t["off"], c["ooctx_meth"], c["ooctx_unmeth"])}
    assert np.unique(beta["context"]).size > 10 and (np.diff(np.sort(beta["context"])) == 0).any()   # many steps, with ties
    hit = sorted(int(m) for m in np.unique(match[match > 0]))
    assert (match < 0).any() and len(hit) >= 4
    nohit = [r for r in range(1, len(bed) + 1) if r not in hit]
    assert nohit
    kw = dict(bed_type=bed_type, match_tolerance=param if bed_type == "amplicon" else -7,
              match_min_overlap=param if bed_type == "capture" else 77, ecdf_context=ctx)
    # sort(unique(match), na.last=TRUE); intersect(bed.rows, that) keeps bed.rows' order and drops repeats
    perm = [hit[i] for i in np.random.default_rng(3).permutation(len(hit))]
    perm.insert(2, None)
    for bed_rows, keys in ((None, hit + [None]),
                           (perm, perm),
                           ([hit[2], hit[0], hit[2], None, hit[0], None], [hit[2], hit[0], None]),
                           ([nohit[0], hit[1], len(bed) + 1, 1000, nohit[-1], hit[0]], [hit[1], hit[0]]),
                           ([nohit[0], len(bed) + 5], []),
                           ((hit[3],), [hit[3]])):
        _check_ecdfs(ea.generateBedEcdf(synth_bam, bed, bed_rows=bed_rows, **kw), bed, match, beta, keys)


def test_bed_ecdf_without_unmatched_reads_has_no_na_group(ea, synth_bam):
    t = H.match_templates()
    bed = _small_bed(ea, spanning=True)
    match = _restated_match(bed, "capture", 0)
    assert (match > 0).all() and sorted(np.unique(match)) == [1, 2, 3]
    c = H.CONTEXT_TO_BASES["CG"]
    beta = {"context": H.beta_np(t["xm"], t["off"], c["ctx_meth"], c["ctx_unmeth"]),
            "out.of.context": H.beta_np(t["xm"], t["off"], c["ooctx_meth"], c["ooctx_unmeth"])}
    for bed_rows, keys in ((None, [1, 2, 3]), ([None, 3, 1], [3, 1])):
        got = ea.generateBedEcdf(synth_bam, bed, bed_type="capture", bed_rows=bed_rows, match_min_overlap=0, ecdf_context="CG")
        _check_ecdfs(got, bed, match, beta, keys)
