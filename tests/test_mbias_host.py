"""generateMbiasReport on the host side: the exported symbol, the functions' signatures, argument checks before any I/O, the
loud failure without a device (there is no CPU path), the restatement of the definition (tests/mbias_np.py) against facts
that do not come from it, and suggestTrim on crafted count tables.  The three tests of the restatement alone (tests/mbias_np.py
against the fixtures' letter counts, the identities and the toy) exercise no code of the library: they would pass without the
report and are here to pin the reference that the GPU tests compare with."""
import inspect
import os
import re

import numpy as np
import pytest

import helpers as H
import mbias_np as MB
import epialleler_amd as ea
from epialleler_amd import _lib

EMPTY = inspect.Parameter.empty
LETTERS = {"Z": (2, 0), "z": (2, 1), "X": (1, 0), "x": (1, 1), "H": (0, 0), "h": (0, 1)}    # letter -> (context index, state)


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_symbol_declared_exported_and_listed():
    _lib.build()
    with open(os.path.join(H.GOLDEN, "..", "..", "include", "epihip.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    name = "epi_batch_mbias_report_dev"
    assert name in _lib.EXPORTED_SYMBOLS
    assert hasattr(_lib.load(), name)
    assert re.search(r"\bint %s\(epi_batch \*b, int32_t max_offset, int64_t \*d_counts, int64_t \*d_totals, void \*stream\);" % name, hdr)


def test_signatures_defaults_and_columns():
    assert ea.MBIAS_COLUMNS == ("end", "strand", "context", "offset", "meth", "unmeth", "beta") == MB.COLUMNS
    p = inspect.signature(ea.generateMbiasReport).parameters
    assert [(k, v.default) for k, v in p.items() if v.kind is not v.VAR_KEYWORD] == [
        ("bam", EMPTY), ("report_file", None), ("report_context", "CX"), ("max_offset", 150), ("gzip", False), ("verbose", False),
        ("as_device", False)]
    assert [k for k, v in p.items() if v.kind is v.VAR_KEYWORD] == ["preprocess_args"]
    q = inspect.signature(ea.rcpp_mbias_report).parameters
    assert [(k, v.default) for k, v in q.items()] == [("df", EMPTY), ("max_offset", EMPTY), ("as_device", False)]
    r = inspect.signature(ea.suggestTrim).parameters
    assert [(k, v.default) for k, v in r.items()] == [("report", EMPTY), ("context", "CG"), ("max_delta", 0.05), ("min_calls", 100), ("run", 3)]


@pytest.mark.parametrize("kw", [dict(max_offset=0), dict(max_offset=1025), dict(max_offset=2.5), dict(max_offset=True), dict(report_context="cg")],
                         ids=lambda kw: ",".join("%s=%s" % it for it in kw.items()))
def test_bad_arguments_raise_before_io(kw):
    with pytest.raises(ValueError) as ei:
        ea.generateMbiasReport("no-such-file.bam", **kw)               # (opening it would raise another error)
    msg = str(ei.value)
    if "report_context" in kw:
        assert "'report.context' should be one of 'CG', 'CHG', 'CHH', 'CxG', 'CX'" in msg
    else:
        assert "'max.offset' should be an integer from 1 to 1024" in msg
    assert "no-such-file" not in msg and "open" not in msg


def test_good_edge_values_reach_the_file():
    report = ea.generateMbiasReport                                    # (resolved here: a missing function is no "file not found")
    for kw in (dict(max_offset=1), dict(max_offset=1024), dict(max_offset=np.int64(17)), dict(max_offset=16.0), dict(report_context="CxG")):
        with pytest.raises(ValueError) as ei:                          # the producer's own error for a file that is not there
            report("no-such-file.bam", **kw)
        assert "Unable to open BAM file" in str(ei.value) and "should be" not in str(ei.value), kw


def test_fails_loudly_without_gpu():
    if _has_gpu():
        pytest.skip("GPU present")
    t = H.templates_from_xm(["Z.z.Z.z", "z.Z.z.Z"], [1, 1], [1, 2])
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"], levels=["chr1"])
    for call in (lambda: ea.generateMbiasReport(bam), lambda: ea.rcpp_mbias_report(bam, 16)):
        with pytest.raises(ea.EpihipError) as ei:
            call()
        assert ei.value.code == 5 and "no CPU fallback" in str(ei.value)


# ---- the restatement against facts that are not its own ---------------------------------------------------------------------

@pytest.mark.parametrize("name", ["capture.bam", "amplicon010meth.bam"])
def test_restatement_on_the_fixtures(name):
    t = H.load_bam(name)
    lens = np.diff(t["off"])
    longest = int(lens.max())
    tab, tot = MB.counts(t["xm"], t["off"], t["strand"], longest)
    assert tot.sum() > 1000
    for letter, (k, state) in LETTERS.items():                          # totals: the per-row letter counts, summed by strand
        per_row = H.class_counts(t["xm"], t["off"], letter)
        for s in (1, 2):
            assert tot[s - 1, k, state] == per_row[t["strand"] == s].sum(), (letter, s)
    # max_offset at the longest row: every byte is in both tables
    assert np.array_equal(tab[0].sum(axis=2), tot) and np.array_equal(tab[1].sum(axis=2), tot)
    # a smaller max_offset is a prefix of the larger table; the totals do not depend on it
    small, tot_small = MB.counts(t["xm"], t["off"], t["strand"], 17)
    assert np.array_equal(small, tab[:, :, :, :17]) and np.array_equal(tot_small, tot)
    # rows of one length L: start[d] == end[L - 1 - d]
    L = int(np.bincount(lens).argmax())
    sub = H.subset(t, lens == L)
    assert sub["strand"].size >= 2
    eq, _ = MB.counts(sub["xm"], sub["off"], sub["strand"], L)
    assert eq.sum() > 0 and np.array_equal(eq[0], eq[1][:, :, ::-1])


def test_restatement_on_a_toy():
    """Three rows, max_offset = 3, the table written out: row 1 '+' "Zx.hZ" (5 bytes: its middle byte is in both tables), row 2 '-'
    "zH" (2 bytes: both in both tables), row 3 '+' "U-Z" (U and the filler have no class)."""
    t = H.templates_from_xm(["Zx.hZ", "zH", "U-Z"], [1, 2, 3], [1, 2, 1])
    rep, totals = MB.restate(t, 3)
    cells = {(int(e), int(s), int(c), int(d)): (int(m), int(u)) for e, s, c, d, m, u in
             zip(rep["end"], rep["strand"], rep["context"], rep["offset"], rep["meth"], rep["unmeth"])}
    want = {(1, 1, 7, 0): (1, 0), (1, 1, 6, 1): (0, 1), (1, 1, 7, 2): (1, 0),           # start, '+': Z at 0; x at 1; row 3's Z at 2
            (2, 1, 7, 0): (2, 0), (2, 1, 2, 1): (0, 1),                                  # end, '+': both rows end in Z; h one before
            (1, 2, 7, 0): (0, 1), (1, 2, 2, 1): (1, 0),                                  # start, '-': z, H
            (2, 2, 2, 0): (1, 0), (2, 2, 7, 1): (0, 1)}                                  # end, '-': H, z
    assert len(cells) == 36 and rep["end"].dtype == np.int32 and rep["meth"].dtype == np.int32 and rep["beta"].dtype == np.float64
    for key, v in cells.items():
        assert v == want.get(key, (0, 0)), key
    assert rep["end"].tolist() == [1] * 18 + [2] * 18 and rep["strand"].tolist() == ([1] * 9 + [2] * 9) * 2
    assert rep["context"].tolist() == ([2] * 3 + [6] * 3 + [7] * 3) * 4 and rep["offset"].tolist() == [0, 1, 2] * 12
    tot = {(int(s), int(c)): (int(m), int(u)) for s, c, m, u in zip(totals["strand"], totals["context"], totals["meth"], totals["unmeth"])}
    assert tot == {(1, 2): (0, 1), (1, 6): (0, 1), (1, 7): (3, 0), (2, 2): (1, 0), (2, 6): (0, 0), (2, 7): (0, 1)}
    assert totals["meth"].dtype == np.int64 and totals["strand"].tolist() == [1, 1, 1, 2, 2, 2]
    b = dict(zip(zip(rep["end"].tolist(), rep["strand"].tolist(), rep["context"].tolist(), rep["offset"].tolist()), rep["beta"]))
    assert b[(2, 1, 7, 0)] == 1.0 and b[(1, 2, 7, 0)] == 0.0 and np.isnan(b[(1, 1, 2, 0)])
    sub, sub_tot = MB.restate(t, 3, "CxG")
    assert sub["context"].tolist() == ([6] * 3 + [7] * 3) * 4 and sub_tot["context"].tolist() == [6, 7, 6, 7]


# ---- suggestTrim on crafted count tables --------------------------------------------------------------------------------------

M = 40                                                       # D0 = 20


def crafted(start, end, other_context=None):
    """A dense report of max_offset = M whose CG rows hold start[d] / end[d] = (meth, unmeth): the methylated calls on '+', the
    unmethylated on '-' (only the pooled strands give the betas meant); other_context: the same cells for CHH, or zeros"""
    tab = np.zeros((2, 2, 3, M, 2), np.int64)
    for e, cells in enumerate((start, end)):
        for d, (m, u) in enumerate(cells):
            tab[e, 0, 2, d, 0] = m
            tab[e, 1, 2, d, 1] = u
            if other_context:
                tab[e, 0, 0, d] = other_context
    return MB.table(tab)


def both(rep, **kw):
    a, b = ea.suggestTrim(rep, **kw), MB.suggest_trim(rep, **kw)
    assert a == b and all(isinstance(v, int) for v in a)
    return a


CLEAN = [(800, 200)] * M


def test_suggest_trim_clean():
    assert both(crafted(CLEAN, CLEAN)) == (0, 0)
    assert both(crafted(CLEAN, CLEAN, other_context=(0, 500))) == (0, 0)           # another context's rows do not pool in
    assert both(crafted(CLEAN, CLEAN, other_context=(0, 500)), context="CHH") == (0, 0)
    assert both(crafted([(840, 160)] * 20 + [(800, 200)] * 20, CLEAN)) == (0, 0)   # 0.84 against 0.8: inside max_delta


def test_suggest_trim_one_biased_end():
    biased = [(300, 700)] * 5 + CLEAN[5:]
    assert both(crafted(biased, CLEAN)) == (5, 0)
    assert both(crafted(CLEAN, biased)) == (0, 5)
    assert both(crafted(biased, CLEAN), max_delta=0.6) == (0, 0)
    assert both(crafted([(740, 260)] * 5 + CLEAN[5:], CLEAN)) == (5, 0)            # 0.74: outside 0.05
    assert both(crafted([(740, 260)] * 5 + CLEAN[5:], CLEAN), max_delta=0.07) == (0, 0)


def test_suggest_trim_ignores_low_coverage():
    outlier = CLEAN[:1] + [(0, 99)] + CLEAN[2:]                                    # offset 1: inside the first run
    assert both(crafted(outlier, CLEAN)) == (0, 0)
    assert both(crafted(outlier, CLEAN), min_calls=99) == (2, 0)                   # 99 calls count once min_calls is 99
    assert both(crafted(CLEAN[:1] + [(0, 100)] + CLEAN[2:], CLEAN)) == (2, 0)
    assert both(crafted(CLEAN[:7] + [(0, 100)] + CLEAN[8:], CLEAN)) == (0, 0)      # (a deviating offset behind a whole run is not looked at)


def test_suggest_trim_needs_a_whole_run():
    bad = (300, 700)
    cells = [bad, bad, CLEAN[0], CLEAN[0], bad] + CLEAN[5:]                        # offsets 2 and 3 conform, 4 does not
    assert both(crafted(cells, CLEAN)) == (5, 0)
    assert both(crafted(cells, CLEAN), run=2) == (2, 0)
    assert both(crafted(cells, CLEAN), run=1) == (2, 0)
    near_d0 = [bad] * 19 + CLEAN[19:]                                              # the run is cut at D0: t = 19 looks at 19 alone
    assert both(crafted(near_d0, CLEAN)) == (19, 0)


def test_suggest_trim_everything_deviating_gives_d0():
    cells = [(300, 700)] * 20 + CLEAN[20:]
    assert both(crafted(cells, cells)) == (20, 20)
    assert both(crafted([(300, 700)] * 30 + CLEAN[30:], CLEAN)) == (20, 0)         # offsets past D0 are the plateau, never trimmed


def test_suggest_trim_empty_plateau_raises():
    empty = CLEAN[:20] + [(0, 0)] * 20
    for rep in (crafted(empty, CLEAN), crafted(CLEAN, empty)):
        with pytest.raises(ValueError):
            ea.suggestTrim(rep)
        with pytest.raises(ValueError):
            MB.suggest_trim(rep)
    with pytest.raises(ValueError):
        ea.suggestTrim(crafted(CLEAN, CLEAN), context="CHG")                       # no CHG call at all
    with pytest.raises(ValueError):
        ea.suggestTrim(crafted(CLEAN, CLEAN), context="cg")
