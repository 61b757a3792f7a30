"""generateAsmReport on the host side: the exported symbols, the column tuples and the functions' signatures, allele_masks by
hand, argument checks before any I/O, the event buffer's size as a function of its own, the loud failure without a device
(there is no CPU path), and the restatement of the definitions (tests/asm_np.py) against tables written by hand and on the
reference's two fixtures."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import helpers as H
import asm_np as A
import epialleler_amd as ea
from epialleler_amd import _lib

NEW_SYMBOLS = ("epi_batch_asm_report_dev", "epi_batch_asm_fetch_dev", "epi_asm_event_bytes")
EMPTY = inspect.Parameter.empty
NAN = float("nan")


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_symbols_declared_exported_and_listed():
    _lib.build()
    with open(os.path.join(H.GOLDEN, "..", "..", "include", "epihip.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(_lib.load(), name)
        assert re.search(r"\bint %s\(" % name, hdr)
    assert ea.ASM_COLUMNS == ("name", "REF", "ALT") + A.PAIR_COLUMNS
    assert ea.ASM_SNV_COLUMNS == ("name", "REF", "ALT") + A.SNV_COLUMNS
    assert A.PAIR_COLUMNS == ("snv", "rname", "snv_pos", "strand", "pos", "context", "meth_ref", "unmeth_ref", "meth_alt", "unmeth_alt",
                              "beta_ref", "beta_alt", "delta_beta", "p")
    assert A.SNV_COLUMNS == ("rname", "pos", "reads_ref", "reads_alt", "reads_other", "npairs", "meth_ref", "unmeth_ref", "meth_alt",
                             "unmeth_alt", "beta_ref", "beta_alt", "delta_beta", "p")
    assert isinstance(ea.ASM_COLUMNS, tuple) and isinstance(ea.ASM_SNV_COLUMNS, tuple)


def test_signatures_and_defaults():
    want = [("bam", EMPTY), ("vcf", EMPTY), ("vcf_style", None), ("bed", None), ("report_file", None), ("zero_based_bed", False),
            ("asm_context", None), ("max_distance", 0), ("min_coverage", 1), ("max_outofcontext_beta", 0.1), ("gzip", False),
            ("verbose", False), ("as_device", False)]
    for fn in (ea.generateAsmReport, ea.generateAsmSnvReport):
        p = inspect.signature(fn).parameters
        assert [(k, v.default) for k, v in p.items() if v.kind is not v.VAR_KEYWORD] == want
        assert [k for k, v in p.items() if v.kind is v.VAR_KEYWORD] == ["preprocess_args"]
    q = inspect.signature(ea.rcpp_asm_report).parameters
    assert [(k, v.default) for k, v in q.items()] == [
        ("df", EMPTY), ("site_chr", EMPTY), ("site_pos", EMPTY), ("site_alleles", EMPTY), ("ctx", EMPTY), ("max_distance", EMPTY),
        ("min_coverage", EMPTY), ("max_ooctx_meth_frac", EMPTY), ("as_device", False)]
    assert [(k, v.default) for k, v in inspect.signature(ea.allele_masks).parameters.items()] == [("ref", EMPTY), ("alt", EMPTY)]


def test_allele_masks_by_hand():
    """bits 0-3 REF '+', 4-7 ALT '+', 8-11 REF '-', 12-15 ALT '-'; A = 1, C = 2, G = 4, T = 8"""
    m = ea.allele_masks(["C", "A", "G", "A", "N", "A"], ["T", "C", "A", "A", "T", "-"])
    assert m.dtype == np.int32 and m.shape == (6,)
    assert m[0] & 0xFF == 0 and (m[0] >> 8) & 15 == 2 and (m[0] >> 12) & 15 == 8          # C>T: '+' cannot tell; '-' REF = C, ALT = T
    assert (m[1] >> 4) & 15 == (2 | 8) and m[1] & 15 == 1 and (m[1] >> 8) & 15 == 1 and (m[1] >> 12) & 15 == 2    # A>C: '+' ALT = C|T
    assert m[2] == 0x14                                                                   # G>A: '+' only
    assert m[3:].tolist() == [0, 0, 0]                                                    # not in the table
    for (r, a) in A.ALLELES:
        v = int(ea.allele_masks([r], [a])[0])
        assert v == A.mask_of(r, a) and v >> 16 == 0 and v & (v >> 4) & 0x0F0F == 0, (r, a)
    assert ea.allele_masks([], []).shape == (0,)


BAD = [dict(max_distance=-1), dict(max_distance=0.5), dict(max_distance=True), dict(max_distance=2 ** 31), dict(min_coverage=-1),
       dict(min_coverage=1.5), dict(min_coverage=2 ** 31), dict(asm_context="CpG"), dict(asm_context="cg")]
R_NAME = {"max_distance": "max.distance", "min_coverage": "min.coverage"}


@pytest.mark.parametrize("fn", ["generateAsmReport", "generateAsmSnvReport"])
@pytest.mark.parametrize("kw", BAD, ids=lambda kw: ",".join("%s=%s" % it for it in kw.items()))
def test_bad_arguments_raise_before_io(fn, kw):
    with pytest.raises(ValueError) as ei:
        getattr(ea, fn)("no-such-file.bam", "no-such-file.vcf", **kw)
    msg = str(ei.value)
    name = list(kw)[-1]
    if name == "asm_context":
        assert "'asm.context' should be one of 'CG', 'CHG', 'CHH', 'CxG', 'CX'" in msg
    else:
        assert "'%s' should be an integer from 0 to 2147483647" % R_NAME[name] in msg
    assert "no-such-file" not in msg and "open" not in msg


def test_good_edge_values_reach_the_file():
    for kw in (dict(max_distance=0), dict(max_distance=2 ** 31 - 1), dict(min_coverage=0), dict(min_coverage=2 ** 31 - 1),
               dict(max_distance=np.int64(3), min_coverage=5.0), dict(asm_context="CX")):
        for fn in (ea.generateAsmReport, ea.generateAsmSnvReport):
            with pytest.raises(Exception) as ei:
                fn("no-such-file.bam", "no-such-file.vcf", **kw)                  # the VCF is read before the BAM
            assert "should be" not in str(ei.value) and "no-such-file.vcf" in str(ei.value), kw


def test_event_bytes():
    """24 bytes per event: the 64-bit key, the sort's 32-bit value and the second buffer of each; 0 .. 2^32 - 1 events"""
    lib = _lib.load()
    out = C.c_int64(-1)
    for n in (0, 1, 2 ** 32 - 1):
        assert lib.epi_asm_event_bytes(n, C.byref(out)) == _lib.EPI_OK and out.value == 24 * n, n
    for n in (-1, 2 ** 32, 2 ** 40):
        assert lib.epi_asm_event_bytes(n, C.byref(out)) == _lib.EPI_ERR_ARG and out.value == 0, n
    assert b"events" in lib.epi_last_error()
    assert lib.epi_asm_event_bytes(1, None) == _lib.EPI_ERR_ARG


def test_fails_loudly_without_gpu():
    if _has_gpu():
        pytest.skip("GPU present")
    t, (chr_, pos, masks), kw = A.hand_cases()["rules"]
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"], levels=["chr1"])
    vcf = ea.Vcf(["chr1"], [0], [A.SNV_POS], ["A"], ["T"], ["rs1"])
    for call in (lambda: ea.rcpp_asm_report(bam, chr_, pos, masks, "Zz", 0, 1, 0.1), lambda: ea.generateAsmReport(bam, vcf),
                 lambda: ea.generateAsmSnvReport(bam, vcf)):
        with pytest.raises(ea.EpihipError) as ei:
            call()
        assert ei.value.code == 5 and "no CPU fallback" in str(ei.value)


# ---- the restatement against tables written by hand ---------------------------------------------------------------------------

def table(tab, cols):
    return [tuple(int(tab[k][i]) for k in cols) for i in range(len(tab[cols[0]]))]


def run(name):
    t, (chr_, pos, masks), kw = A.hand_cases()[name]
    return A.restate(t, chr_, pos, masks, **kw)


def test_hand_rules():
    """The filler at the SNV, the call at the SNV itself, the dropped row, the strand-0 row, a third base, an ALT-only group"""
    pairs, snvs = run("rules")
    assert table(pairs, A.PAIR_INT) == [(0, 1, 105, 1, 100, 7, 1, 0, 0, 1), (0, 1, 105, 1, 109, 7, 1, 0, 0, 1)]
    assert pairs["beta_ref"].tolist() == [1.0, 1.0] and pairs["beta_alt"].tolist() == [0.0, 0.0] and pairs["delta_beta"].tolist() == [-1.0, -1.0]
    assert table(snvs, A.SNV_INT) == [(1, 105, 1, 2, 2, 2, 2, 0, 0, 2)]
    assert snvs["beta_ref"][0] == 1.0 and snvs["beta_alt"][0] == 0.0 and snvs["delta_beta"][0] == -1.0
    assert all(pairs[k].dtype == np.int32 for k in A.PAIR_INT) and pairs["beta_ref"].dtype == np.float64


def test_hand_distance():
    """max_distance = 4: the calls at 101 and 109 are in, those at 100 and 110 out"""
    pairs, snvs = run("distance")
    assert table(pairs, A.PAIR_INT) == [(0, 1, 105, 1, 101, 7, 1, 0, 0, 1), (0, 1, 105, 1, 109, 7, 1, 0, 0, 1)]
    assert table(snvs, A.SNV_INT) == [(1, 105, 1, 1, 0, 2, 2, 0, 0, 2)]
    t, (chr_, pos, masks), kw = A.hand_cases()["distance"]
    assert [len(A.restate(t, chr_, pos, masks, "Zz", max_distance=d)[0]["pos"]) for d in (0, 3, 4, 5)] == [4, 0, 2, 4]


def test_hand_two_alts_at_one_position():
    """A>T and A>C at 105: a T on '+' is ALT for both (bisulfite: ALT C reads as C or T), a T on '-' only for A>T"""
    pairs, snvs = run("two_alts")
    rows = [(1, 105, 1, 100, 7, 1, 0, 0, 1), (1, 105, 1, 109, 7, 1, 0, 0, 1)]
    assert table(pairs, A.PAIR_INT) == [(0,) + r for r in rows] + [(1,) + r for r in rows]
    assert table(snvs, A.SNV_INT) == [(1, 105, 1, 2, 2, 2, 2, 0, 0, 2), (1, 105, 1, 1, 3, 2, 2, 0, 0, 2)]


def test_hand_na_site():
    pairs, snvs = run("na_site")
    assert pairs["snv"].tolist() == [1, 1] and pairs["pos"].tolist() == [100, 109]
    assert table(snvs, A.SNV_INT) == [(A.NA_INT, 7, 0, 0, 0, 0, 0, 0, 0, 0), (1, 105, 1, 2, 2, 2, 2, 0, 0, 2)]
    assert np.isnan(snvs["beta_ref"][0]) and np.isnan(snvs["beta_alt"][0]) and np.isnan(snvs["delta_beta"][0])


def test_hand_min_coverage():
    """At 100 both alleles have two calls, at 109 one: min_coverage 2 keeps 100 alone, 1 (and 0) both, 3 nothing"""
    pairs, snvs = run("coverage_1")
    assert table(pairs, A.PAIR_INT) == [(0, 1, 105, 1, 100, 7, 1, 1, 1, 1), (0, 1, 105, 1, 109, 7, 1, 0, 0, 1)]
    assert table(snvs, A.SNV_INT) == [(1, 105, 2, 2, 0, 2, 2, 1, 1, 2)]
    assert snvs["beta_ref"][0] == 2 / 3 and snvs["beta_alt"][0] == 1 / 3 and snvs["delta_beta"][0] == np.float64(1) / 3 - np.float64(2) / 3
    pairs, snvs = run("coverage_2")
    assert table(pairs, A.PAIR_INT) == [(0, 1, 105, 1, 100, 7, 1, 1, 1, 1)]
    assert table(snvs, A.SNV_INT) == [(1, 105, 2, 2, 0, 1, 1, 1, 1, 1)] and snvs["delta_beta"][0] == 0.0
    pairs, snvs = run("coverage_3")
    assert table(pairs, A.PAIR_INT) == [] and table(snvs, A.SNV_INT) == [(1, 105, 2, 2, 0, 0, 0, 0, 0, 0)]
    assert np.isnan(snvs["beta_ref"][0]) and np.isnan(snvs["delta_beta"][0])
    t, (chr_, pos, masks), kw = A.hand_cases()["coverage_1"]
    assert len(A.restate(t, chr_, pos, masks, "Zz", min_coverage=0)[0]["pos"]) == 2


# ---- the restatement on the reference's fixtures ----------------------------------------------------------------------------------

def fixture_sites(which):
    """(templates, (site_chr, site_pos, site_alleles), the sorted Vcf) of a reference fixture, as generateAsmReport prepares them"""
    bam, vcf, bed, style = {"amplicon": ("amplicon010meth.bam", "amplicon.vcf.gz", "amplicon.bed", "NCBI"),
                            "capture": ("capture.bam", "capture.vcf.gz", "capture.bed", None)}[which]
    t = H.bam(bam)
    v = ea.readVcf(os.path.join(H.GOLDEN, "vcf", vcf), vcf_style=style, bed=os.path.join(H.GOLDEN, "bam", bed))
    v = v.subset(np.lexsort((v.pos, v.chrom)))
    code = {s: i + 1 for i, s in enumerate(t["levels"])}
    seq = np.asarray([code.get(s, A.NA_INT) for s in v.levels], np.int32)[v.chrom]
    return t, (seq, v.pos, ea.allele_masks(v.ref, v.alt)), v


def test_restatement_on_the_fixtures():
    """The amplicon fixture reports pair rows; the capture fixture has no read with an ALT base at any of its SNVs and none"""
    t, sites, v = fixture_sites("amplicon")
    pairs, snvs = A.restate(t, *sites, "Zz")
    assert len(v) == 56 and len(pairs["snv"]) == 181 and snvs["npairs"].max() == 21
    assert (snvs["reads_ref"].sum(), snvs["reads_alt"].sum(), snvs["reads_other"].sum()) == (5267, 13, 2155)
    for k in A.CELLS:                                        # the SNV table is a group-by of the pair table
        assert np.array_equal(np.bincount(pairs["snv"], pairs[k], len(v)), snvs[k]), k
    assert np.array_equal(np.bincount(pairs["snv"], minlength=len(v)), snvs["npairs"])
    order = list(zip(pairs["snv"], pairs["pos"], pairs["strand"], pairs["context"]))
    assert order == sorted(order) and len(set(order)) == len(order)
    assert np.all(pairs["meth_ref"] + pairs["unmeth_ref"] >= 1) and np.all(pairs["meth_alt"] + pairs["unmeth_alt"] >= 1)
    assert np.all(pairs["pos"] != pairs["snv_pos"])
    t, sites, v = fixture_sites("capture")
    pairs, snvs = A.restate(t, *sites, "Zz")
    assert len(v) == 26292 and len(pairs["snv"]) == 0 and snvs["reads_alt"].sum() == 0 and snvs["reads_ref"].sum() == 12883
