"""generateHeterogeneityReport against a plain restatement of its definitions (include/epihip.h): loops over rows and
numpy.  The restatement's site table is the CPU restatement's cx_report with an all-ones pass vector, its kept rows are
helpers.mhl_keep_np; nothing in it reads the GPU's own cytosine report.  Integer columns and the pattern histograms
compare exactly; the four float columns within 1e-12 absolute: each is a sum of at most 64 terms of magnitude below 1,
every term within a few ulp (2.2e-16) of the float64 value."""
import ctypes as C
import functools

import numpy as np
import pytest

import helpers as H
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

INT_COLS = ("rname", "strand", "pos", "end", "context", "nreads", "npatterns")
FLOAT_COLS = ("beta", "epipolymorphism", "entropy", "pdr")
ATOL = 1e-12


@pytest.fixture(scope="module")
def ea():
    import epialleler_amd
    return epialleler_amd


# ---- the restatement -------------------------------------------------------------------------------------------------

def restate(t, ctx, k, max_oo=0.1, min_reads=1, max_span=0):
    """The report of the templates t for the named context: dict of the eleven columns plus `counts` [nrow, 2^k] and
    `sites` (the site table's rname, strand, pos, context)."""
    c = H.CONTEXT_TO_BASES[ctx]
    n = t["off"].size - 1
    xm = np.asarray(t["xm"], np.uint8)
    cx = orc.cx_report(xm, t["off"], t["rname"], t["strand"], t["start"], np.ones(max(n, 1), np.int32)[:n], c["ctx_meth"])
    keep = H.mhl_keep_np(xm, t["off"], c["ctx_meth"] + c["ctx_unmeth"], 0, max_oo) if n else np.zeros(0, bool)
    N = cx["pos"].size
    nb = 1 << k
    counts = np.zeros((N, nb), np.int64)                 # by CX row: the window that starts there
    end = np.zeros(N, np.int64)
    is_window = np.zeros(N, bool)
    weights = 1 << np.arange(k)
    for r in np.unique(cx["rname"]):
        for s in (1, 2):
            rows = np.flatnonzero((cx["rname"] == r) & (cx["strand"] == s))
            P = cx["pos"][rows].astype(np.int64)
            assert np.all(np.diff(P) > 0)
            code = cx["context"][rows]
            m = rows.size
            if m < k:
                continue
            is_window[rows[:m - k + 1]] = True
            end[rows[:m - k + 1]] = P[k - 1:]
            for x in np.flatnonzero((t["rname"] == r) & (t["strand"] == s) & keep):
                st, o0, o1 = int(t["start"][x]), int(t["off"][x]), int(t["off"][x + 1])
                a, b = np.searchsorted(P, st), np.searchsorted(P, st + (o1 - o0))
                if b - a < k:
                    continue
                nib = xm[o0 + (P[a:b] - st)] & 15
                valid = (nib & 7) == code[a:b]
                meth = valid & (nib < 8)
                wv = np.lib.stride_tricks.sliding_window_view(valid, k).all(axis=1)
                wp = (np.lib.stride_tricks.sliding_window_view(meth, k) * weights).sum(axis=1)
                j = np.flatnonzero(wv)
                np.add.at(counts, (rows[a + j], wp[j]), 1)
    nreads = counts.sum(axis=1)
    span = end - cx["pos"].astype(np.int64) + 1
    rep = is_window & (nreads >= max(min_reads, 1)) & ((span <= max_span) if max_span else True)
    cn = counts[rep]
    nr = cn.sum(axis=1).astype(np.float64)
    popc = np.asarray([bin(p).count("1") for p in range(nb)], np.float64)
    p = cn / nr[:, None] if cn.size else np.zeros((0, nb))
    with np.errstate(divide="ignore", invalid="ignore"):
        plogp = np.where(p > 0, p * np.log2(p), 0.0)
    out = {"rname": cx["rname"][rep], "strand": cx["strand"][rep], "pos": cx["pos"][rep], "end": end[rep].astype(np.int32),
           "context": cx["context"][rep], "nreads": cn.sum(axis=1).astype(np.int32), "npatterns": (cn > 0).sum(axis=1).astype(np.int32),
           "beta": (cn * popc).sum(axis=1) / (nr * k), "epipolymorphism": 1.0 - (p * p).sum(axis=1),
           "entropy": -plogp.sum(axis=1) / k, "pdr": 1.0 - (cn[:, 0] + cn[:, nb - 1]) / nr,
           "counts": cn.astype(np.int32), "sites": {q: cx[q] for q in ("rname", "strand", "pos", "context")}}
    return out


def as_bam(ea, t, levels=None):
    return ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"], levels or t.get("levels"))


def gpu_report(ea, bam, ctx, k, max_oo=0.1, min_reads=1, max_span=0):
    c = H.CONTEXT_TO_BASES[ctx]
    return ea.rcpp_heterogeneity_report(bam, c["ctx_meth"] + c["ctx_unmeth"], k, max_oo, min_reads, max_span, with_counts=True)


def assert_same(got, want, what=""):
    assert list(got.keys()) == list(INT_COLS + FLOAT_COLS)
    for q in INT_COLS:
        assert got[q].dtype == np.int32 and np.array_equal(got[q], want[q]), (what, q)
    for q in FLOAT_COLS:
        assert got[q].dtype == np.float64 and got[q].shape == want[q].shape, (what, q)
        err = float(np.max(np.abs(got[q] - want[q]))) if want[q].size else 0.0
        assert err <= ATOL, (what, q, err)
    assert got.counts.dtype == np.int32 and np.array_equal(got.counts, want["counts"]), (what, "counts")


def check(ea, t, ctx, k, nonempty=True, **kw):
    want = restate(t, ctx, k, **kw)
    if nonempty:                                         # (two empty tables would compare equal)
        assert want["pos"].size > 0 and np.any(want["npatterns"] > 1), "the case exercises nothing"
    got = gpu_report(ea, as_bam(ea, t), ctx, k, **kw)
    assert_same(got, want, (ctx, k, kw))
    return got, want


# ---- the reference's fixtures ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def fixture_want(name, ctx, k):
    return restate(H.bam(name), ctx, k)


# windows with reads as the restatement gives them on the CPU: (k = 2, 4, 6)
FIXTURE_WINDOWS = {"capture.bam": (13622, 10563, 8257), "amplicon010meth.bam": (406, 298, 215)}


@pytest.mark.parametrize("k", [2, 4, 6])
@pytest.mark.parametrize("name", ["capture.bam", "amplicon010meth.bam"])
def test_fixtures_cg(ea, name, k):
    t = H.bam(name)
    want = fixture_want(name, "CG", k)
    assert want["pos"].size == FIXTURE_WINDOWS[name][k // 2 - 1] and np.any(want["npatterns"] > 1)
    if k == 4:
        multi, deepest = {"capture.bam": (225, 9), "amplicon010meth.bam": (60, 155)}[name]
        assert int(np.count_nonzero(want["npatterns"] > 1)) == multi and int(want["nreads"].max()) == deepest
    assert_same(gpu_report(ea, as_bam(ea, t), "CG", k), want, (name, k))


def test_fixture_three_contexts(ea):
    t = H.bam("capture.bam")
    want = fixture_want("capture.bam", "CX", 3)
    assert set(np.unique(want["sites"]["context"])) == {2, 6, 7} and np.any(want["npatterns"] > 1)
    assert_same(gpu_report(ea, as_bam(ea, t), "CX", 3), want)


# ---- hand-made batches ----------------------------------------------------------------------------------------------------

def every_other(rng, nsites, p_meth=0.5):
    """A row with a CG call at every other position: Z / z at 0, 2, 4, ..., '.' between."""
    calls = np.where(rng.random(nsites) < p_meth, "Z", "z")
    return "".join(ch + "." for ch in calls)


@pytest.mark.parametrize("k", [2, 6])
def test_rounds_of_64_sites(ea, k):
    """Rows of 200 bytes = 100 sites, piled at starts 1, 3, 5, ...: more than one round of 16 and of 64 sites per row, and
    windows that straddle the 64th site of a row (the rows start at different sites, so every site is a 64th somewhere)."""
    rng = np.random.default_rng(11)
    xms = [every_other(rng, 100, 0.3 + 0.4 * (i % 2)) for i in range(50)]
    t = H.templates_from_xm(xms, [1 + 2 * i for i in range(50)], [1] * 50)
    got, want = check(ea, t, "CG", k)
    # the windows over the 64th and the 128th site of the first row are there, with all the rows that cover them
    for site in (64, 128):
        first = 1 + 2 * (site - k + 1)                  # a window whose last site is the row's site number `site` (0-based)
        i = np.flatnonzero(want["pos"] == first)
        assert i.size == 1 and want["nreads"][i[0]] >= 1


def test_long_rows_take_a_wave_each(ea):
    """Rows of 1200 to 3000 bytes (mean above 512: a whole wave takes a row), sites every third position."""
    rng = np.random.default_rng(12)
    xms = ["".join(("Z" if rng.random() < 0.6 else "z") + ".." for _ in range(int(rng.integers(400, 1000)))) for _ in range(40)]
    t = H.templates_from_xm(xms, [1 + 3 * int(v) for v in rng.integers(0, 300, 40)], [int(v) for v in rng.integers(1, 3, 40)])
    for k in (2, 5):
        check(ea, t, "CG", k)


def test_one_long_row_among_short_ones(ea):
    rng = np.random.default_rng(13)
    long_row = "".join(rng.choice(list("Zz....."), 10000, p=[0.1, 0.05, 0.17, 0.17, 0.17, 0.17, 0.17]))
    assert 1300 < sum(ch in "Zz" for ch in long_row) < 1700
    xms, starts = [long_row], [1]
    for _ in range(200):
        s = int(rng.integers(1, 9900))
        ln = int(rng.integers(40, 120))
        # the short rows repeat the long row's contexts with their own methylation, so the sites stay sites
        xms.append("".join((("Z" if rng.random() < 0.5 else "z") if ch in "Zz" else ".") for ch in long_row[s - 1:s - 1 + ln]))
        starts.append(s)
    t = H.templates_from_xm(xms, starts, [1] * 201)
    check(ea, t, "CG", 4)


def test_strands_interleaved_and_sequence_ends(ea):
    """'+' sites at even, '-' sites at odd positions on two sequences; the last sites of sequence 1 and the first of
    sequence 2 are neighbours in each strand's site table: no window joins them."""
    rng = np.random.default_rng(14)
    xms, starts, strands, rnames = [], [], [], []
    for r in (1, 2):
        for s in (1, 2):
            for _ in range(30):
                nsite = int(rng.integers(3, 12))
                xms.append(every_other(rng, nsite))
                starts.append(2 * int(rng.integers(1, 20)) + (s - 1))
                strands.append(s)
                rnames.append(r)
    t = H.templates_from_xm(xms, starts, strands, rnames)
    for k in (3, 6):
        got, want = check(ea, t, "CG", k)
        assert np.all(got["end"] > got["pos"])
        sites = want["sites"]
        for r in (1, 2):
            for s in (1, 2):
                m = np.count_nonzero((sites["rname"] == r) & (sites["strand"] == s))
                assert m >= k
        # a window that joined two sequences would end before it starts, or be one too many for its (rname, strand)
        for r in (1, 2):
            for s in (1, 2):
                sel = (got["rname"] == r) & (got["strand"] == s)
                m = np.count_nonzero((sites["rname"] == r) & (sites["strand"] == s))
                assert np.count_nonzero(sel) <= m - k + 1
        assert np.array_equal(got["pos"] % 2, (got["strand"] - 1) % 2)


def test_gaps(ea):
    xms = ["Z.z.Z.z.Z.z",       # six sites at 1, 3, ..., 11
           "Z.z.Z.z.Z.z",
           "z.Z.z.Z.z.Z",
           "Z.-.Z.z.Z.z",       # '-' on the second site
           "Z.z...z.Z.z",       # '.' on the third
           "Z.z.h.z.Z.z",       # another context where the majority is z
           "Z.zzZ.z.Z.z",       # a z at position 4, where most rows have '.': not a site, the windows step over it
           "z.Z.z",             # starts inside the windows of the others (position 5) ...
           "Z.z.Z.z",           # ... ends inside them
           "Z"]
    starts = [1, 1, 1, 1, 1, 1, 1, 5, 1, 11]
    t = H.templates_from_xm(xms, starts, [1] * len(xms))
    for k in (2, 3, 4):
        got, want = check(ea, t, "CG", k, max_oo=1.0)
        assert 4 not in want["sites"]["pos"] and np.array_equal(want["sites"]["pos"], [1, 3, 5, 7, 9, 11])
    want = restate(t, "CG", 3, max_oo=1.0)
    # window 1-3-5: the rows with '-' at 3, with '.' at 5 and with h at 5 do not count; the row with the stray z does
    assert want["nreads"][0] == 5 and want["pos"][0] == 1 and want["end"][0] == 5


def oo_row(o_m, o_a, body="Z.z.Z.z.Z"):
    return body + "." + "X" * o_m + "x" * (o_a - o_m)


def test_row_filter(ea):
    """Out-of-context methylation just below, at and above max_outofcontext_beta; a row without out-of-context calls."""
    rows = [oo_row(0, 0), oo_row(1, 10), oo_row(2, 10), oo_row(0, 10), oo_row(3, 30), oo_row(4, 30), oo_row(2, 30),
            oo_row(1, 10, "z.Z.z.Z.z"), oo_row(2, 10, "z.Z.z.Z.z"), oo_row(10, 10, "z.z.z.z.z")]
    t = H.templates_from_xm(rows, [1] * len(rows), [1] * len(rows))
    keep = H.mhl_keep_np(t["xm"], t["off"], "Zz", 0, 0.1)
    assert keep.tolist() == [True, True, False, True, True, False, True, True, False, False]
    got, want = check(ea, t, "CG", 3, max_oo=0.1)
    assert want["nreads"].tolist() == [6, 6, 6]
    got1, want1 = check(ea, t, "CG", 3, max_oo=1.0)
    assert want1["nreads"].tolist() == [10, 10, 10]
    for q in ("rname", "strand", "pos", "context"):      # the filter never changes the site table
        assert np.array_equal(want["sites"][q], want1["sites"][q])
    assert np.array_equal(got["pos"], got1["pos"])
    check(ea, t, "CG", 3, max_oo=0.0, nonempty=False)
    # CHG windows on the same rows: the X / x calls are the context now, Z / z out of it
    check(ea, t, "CHG", 2, max_oo=0.5, nonempty=False)


def test_contention(ea):
    a, b = "Z.Z.z.Z.z", "z.z.Z.z.Z"
    t = H.templates_from_xm([a] * 20000 + [b] * 20000, [100] * 40000, [1] * 40000)
    got, want = check(ea, t, "CG", 4)
    assert got.nrow == 2 and np.all(got["nreads"] == 40000) and np.all(got["npatterns"] == 2)
    assert np.all(np.sort(got.counts, axis=1)[:, -2:] == 20000)


def test_min_reads_and_span(ea):
    rng = np.random.default_rng(15)
    xms, starts = [], []
    track = "".join(rng.choice(list("C..."), 600))      # where the CpGs are: spacing varies, so spans do
    for _ in range(300):
        s = int(rng.integers(1, 500))
        xms.append("".join((("Z" if rng.random() < 0.5 else "z") if ch == "C" else ".") for ch in track[s - 1:s - 1 + int(rng.integers(30, 100))]))
        starts.append(s)
    t = H.templates_from_xm(xms, starts, [1] * 300)
    full, wfull = check(ea, t, "CG", 4)
    span = full["end"] - full["pos"] + 1
    cut = int(np.median(span))
    sel = (full["nreads"] >= 3) & (span <= cut)
    assert 0 < np.count_nonzero(sel) < sel.size and np.any(full["nreads"] < 3) and np.any(span > cut)
    got, want = check(ea, t, "CG", 4, min_reads=3, max_span=cut)
    for q in INT_COLS + FLOAT_COLS:
        assert np.array_equal(got[q], full[q][sel]), q
    assert np.array_equal(got.counts, full.counts[sel])
    got0 = gpu_report(ea, as_bam(ea, t), "CG", 4, min_reads=0)       # below 1: as 1
    assert np.array_equal(got0["pos"], full["pos"])


@pytest.mark.parametrize("case", ["empty", "no_site", "short_strand"])
def test_degenerate(ea, case):
    k = 4
    if case == "empty":
        t = H.templates_from_xm([], [], [])
    elif case == "no_site":
        t = H.templates_from_xm(["....", "..x..h"], [1, 3], [1, 2])
    else:
        t = H.templates_from_xm(["Z.z.Z", "z.Z.z"], [1, 1], [1, 1])     # k - 1 sites
    want = restate(t, "CG", k)
    assert want["pos"].size == 0
    got = gpu_report(ea, as_bam(ea, t), "CG", k)
    assert_same(got, want)
    assert got.nrow == 0 and got.counts.shape == (0, 16)


def test_short_strand_beside_a_long_one(ea):
    """k - 1 sites on '-', k + 1 on '+': only '+' has windows."""
    t = H.templates_from_xm(["Z.z.Z.z.Z", "z.Z.z.Z.z", ".Z.z.Z", ".z.Z.z"], [1, 1, 1, 1], [1, 1, 2, 2])
    got, want = check(ea, t, "CG", 4)
    assert got["strand"].tolist() == [1, 1] and got["pos"].tolist() == [1, 3] and got["end"].tolist() == [7, 9]


def test_rows_are_cytosine_report_rows(ea):
    t = H.bam("amplicon010meth.bam")
    bam = as_bam(ea, t)
    for ctx, k in (("CG", 3), ("CX", 5)):
        cx = ea.generateCytosineReport(bam, threshold_reads=False, report_context=ctx)
        got = gpu_report(ea, bam, ctx, k)
        assert got.nrow > 0
        key = lambda r: [tuple(v) for v in zip(r["rname"].tolist(), r["strand"].tolist(), r["pos"].tolist(), r["context"].tolist())]
        index = {q: i for i, q in enumerate(key(cx))}
        at = np.asarray([index[q] for q in key(got)])                  # KeyError: a row that is no cytosine report row
        assert np.all(np.diff(at) > 0)                                  # in the cytosine report's order
        for i, row in enumerate(at):
            same = np.flatnonzero((cx["rname"] == cx["rname"][row]) & (cx["strand"] == cx["strand"][row]))
            j = int(np.searchsorted(same, row))
            assert cx["pos"][same[j + k - 1]] == got["end"][i]


def test_sequence_leaves_the_batch_fit(ea):
    t = H.bam("capture.bam")
    bam = as_bam(ea, t)
    cx0 = ea.generateCytosineReport(bam)
    het = gpu_report(ea, bam, "CG", 4)
    cx1 = ea.generateCytosineReport(bam)
    H.assert_reports_equal(cx0, cx1)
    cxu0 = ea.generateCytosineReport(bam, threshold_reads=False, report_context="CX")
    gpu_report(ea, bam, "CHG", 2)
    H.assert_reports_equal(cxu0, ea.generateCytosineReport(bam, threshold_reads=False, report_context="CX"))
    m0 = ea.generateMhlReport(bam)
    het2 = gpu_report(ea, bam, "CG", 4)
    m1 = ea.generateMhlReport(bam)
    H.assert_reports_equal(m0, m1, float_cols=("length", "lmhl"))
    for q in INT_COLS + FLOAT_COLS:
        assert np.array_equal(het[q], het2[q]), q
    # the lMHL fetch right after a heterogeneity report: a call sequence error
    import torch
    from epialleler_amd import _lib, api
    gpu_report(ea, bam, "CG", 4)
    ic = list(torch.empty((5, 8), dtype=torch.int32, device="cuda").unbind(0))
    dc = list(torch.empty((2, 8), dtype=torch.float64, device="cuda").unbind(0))
    rc = _lib.load().epi_batch_mhl_fetch_dev(bam.batch(), api._ptr_array(ic), api._ptr_array(dc), None)
    assert rc == _lib.EPI_ERR_STATE
    cxcols = list(torch.empty((6, 8), dtype=torch.int32, device="cuda").unbind(0))
    assert _lib.load().epi_batch_cx_fetch_dev(bam.batch(), api._ptr_array(cxcols), None) == _lib.EPI_ERR_STATE
    nrow = C.c_int64(0)
    assert _lib.load().epi_batch_heterogeneity_report_dev(bam.batch(), b"Zz", 7, 0.1, 1, 0, None, C.byref(nrow)) == _lib.EPI_ERR_ARG
    assert _lib.load().epi_batch_heterogeneity_report_dev(bam.batch(), b"Zz", 1, 0.1, 1, 0, None, C.byref(nrow)) == _lib.EPI_ERR_ARG


@pytest.mark.parametrize("seed,k", [(1, 2), (2, 4), (3, 6)])
def test_fuzz(ea, seed, k):
    """3000 rows of 30 to 400 bytes on two sequences, contexts fixed per position, 5 % of the bytes replaced."""
    rng = np.random.default_rng(900 + seed)
    glen = 6000
    letters = np.asarray(list(".zxh"))
    track = [letters[rng.choice(4, glen, p=[0.7, 0.15, 0.08, 0.07])] for _ in range(2)]
    noise = np.asarray(list(".-zZxXhHuU"))
    xms, starts, strands, rnames = [], [], [], []
    for _ in range(3000):
        r, s = int(rng.integers(0, 2)), int(rng.integers(1, 3))
        ln = int(rng.integers(30, 401))
        st = int(rng.integers(1, glen - ln))
        row = track[r][st - 1:st - 1 + ln].copy()
        if s == 2:                                       # the '-' strand has its own sites: the track shifted by one
            row = np.roll(row, 1)
        # CpG calls methylated at the row's own rate; the other contexts rarely, so that the row filter splits the rows
        up = rng.random(ln) < np.where(row == "z", 0.2 + 0.6 * rng.random(), rng.choice([0.0, 0.05, 0.15, 0.4]))
        row = np.where(up, np.char.upper(row), row)
        bad = rng.random(ln) < 0.05
        row[bad] = noise[rng.integers(0, noise.size, int(bad.sum()))]
        xms.append("".join(row))
        starts.append(st)
        strands.append(s)
        rnames.append(r + 1)
    t = H.templates_from_xm(xms, starts, strands, rnames)
    check(ea, t, "CG", k)
    check(ea, t, "CxG" if seed & 1 else "CX", k, max_oo=0.3)


def test_file_output(ea, tmp_path):
    t = H.bam("amplicon010meth.bam")
    levels = t.get("levels") or ["chr%d" % i for i in range(1, 100)]
    bam = as_bam(ea, t, levels)
    want = fixture_want("amplicon010meth.bam", "CG", 4)
    rep = ea.generateHeterogeneityReport(bam, window_context="CG", window_sites=4)
    assert list(rep.keys()) == list(INT_COLS + FLOAT_COLS) and not hasattr(rep, "counts")
    for q in INT_COLS:
        assert np.array_equal(rep[q], want[q]), q
    with_counts = ea.rcpp_heterogeneity_report(bam, "Zz", 4, 0.1, with_counts=True)
    assert np.array_equal(with_counts.counts, want["counts"]) and with_counts.counts.sum(axis=1).tolist() == want["nreads"].tolist()
    p, q = tmp_path / "het.tsv", tmp_path / "ref.tsv"
    assert ea.generateHeterogeneityReport(bam, report_file=str(p), window_context="CG", window_sites=4) is None
    ea.writeReport(rep, str(q))
    text = p.read_text()
    assert text == q.read_text()
    lines = text.split("\n")
    assert lines[0] == "\t".join(INT_COLS + FLOAT_COLS) and len(lines) == rep.nrow + 2
    assert lines[1].split("\t")[4] == "CG" and lines[1].split("\t")[1] in "+-"
    dev = ea.generateHeterogeneityReport(bam, window_context="CG", window_sites=4, as_device=True)
    assert dev["entropy"].is_cuda and np.array_equal(dev["entropy"].cpu().numpy(), rep["entropy"])
