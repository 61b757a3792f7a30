"""generateFdrpReport against the plain restatement of its definitions (tests/fdrp_np.py; include/epihip.h,
epi_batch_fdrp_report_dev).  Integer columns compare equal; fdrp and qfdrp compare with np.array_equal: they are computed
from integer counts by the same IEEE operations in the same order on both sides, so they agree bit for bit.

Rows of a batch are sorted by (rname, start) -- the engine refuses anything else -- so "rows that are not in start order"
cannot be built.  The selection tests instead give the covering rows ragged starts and lengths and interleave them, in
batch order, with rows of the other strand, rows that end in front of the site, rows without a call at it and rows the read
rule drops, between rows of two more sequences: the list of covering rows is then far from a run of the batch, and the
result depends on the index being sorted by site, stably, in ascending row order."""
import ctypes as C
import gzip

import numpy as np
import pytest

import fdrp_np
import helpers as H

pytestmark = pytest.mark.gpu

INT_COLS, FLOAT_COLS = fdrp_np.INT_COLS, fdrp_np.FLOAT_COLS


@pytest.fixture(scope="module")
def ea():
    import epialleler_amd
    return epialleler_amd


def as_bam(ea, t, levels=None):
    return ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"], levels)


def gpu_report(ea, bam, ctx, W=8, m=40, min_overlap=1, max_distance=0, max_oo=0.1, min_reads=2):
    c = H.CONTEXT_TO_BASES[ctx]
    return ea.rcpp_fdrp_report(bam, c["ctx_meth"] + c["ctx_unmeth"], W, m, min_overlap, max_distance, max_oo, min_reads)


def assert_same(got, want, label=""):
    for q in INT_COLS:
        assert got[q].dtype == np.int32 and np.array_equal(got[q], want[q]), (label, q, got[q][:12], want[q][:12])
    for q in FLOAT_COLS:
        assert got[q].dtype == np.float64 and np.array_equal(got[q], want[q]), (label, q, got[q][:12], want[q][:12])


def check(ea, t, ctx="CG", nonempty=True, **kw):
    names = {"W": "flank_sites", "m": "max_reads"}
    want = fdrp_np.restate(t, ctx, **{names.get(k, k): v for k, v in kw.items()})
    got = gpu_report(ea, as_bam(ea, t), ctx, **kw)
    assert_same(got, want, str(kw))
    if nonempty:
        assert got.nrow > 0, "two empty tables would compare equal"
    return got, want


def random_xm(rng, L, p_site=0.5, p_meth=0.5, p_gap=0.0, other="", p_other=0.0, phase=0, step=2):
    """A row of L bytes whose positions phase, phase + step, ... hold a CpG call (or, with p_gap, '.' or '-'); elsewhere
    '.', or with p_other a byte of `other` (another context)."""
    out = []
    for j in range(L):
        if (j - phase) % step == 0 and rng.random() < p_site:
            out.append(rng.choice(list(".-")) if rng.random() < p_gap else ("Z" if rng.random() < p_meth else "z"))
        else:
            out.append(rng.choice(list(other)) if other and rng.random() < p_other else ".")
    return "".join(out)


def ragged(rng, nrow, span=120, lmin=8, lmax=90, rnames=(1,), strands=(1, 2), **kw):
    """nrow rows with random starts in [1, span], lengths in [lmin, lmax]; CpG positions are the even ones on every
    sequence, so that a position has one context whichever row covers it."""
    xms, starts, strs, rns = [], [], [], []
    for _ in range(nrow):
        st, L = int(rng.integers(1, span + 1)), int(rng.integers(lmin, lmax + 1))
        xms.append(random_xm(rng, L, phase=st % 2, **kw))
        starts.append(st); strs.append(int(rng.choice(strands))); rns.append(int(rng.choice(rnames)))
    return H.templates_from_xm(xms, starts, strs, rns)


# ---- a case by hand ----------------------------------------------------------------------------------------------------------

def test_by_hand(ea):
    """Sites at 1, 3, 5; W = 1.  Calls (site 1, 3, 5): r0 = M M M, r1 = M u M, r2 = u u M, r3 = - M u.
    Site 1, window {1, 3}, rows r0 r1 r2: (r0, r1) o = 2 h = 1, (r0, r2) o = 2 h = 2, (r1, r2) o = 2 h = 1.
    Site 3, window {1, 3, 5}, all rows: o, h = (3, 1) (3, 2) (2, 1) (3, 1) (2, 2) (2, 2): H[2] = 5, H[3] = 4.
    Site 5, window {3, 5}, all rows: h = 1 1 1 0 2 2, every o = 2: H[2] = 7, five discordant pairs of six."""
    t = H.templates_from_xm(["Z.Z.Z", "Z.z.Z", "z.z.Z", "..Z.z"], [1, 1, 1, 1], [1, 1, 1, 1])
    got = gpu_report(ea, as_bam(ea, t), "CG", W=1)
    assert got["rname"].tolist() == [1, 1, 1] and got["strand"].tolist() == [1, 1, 1] and got["pos"].tolist() == [1, 3, 5]
    assert got["coverage"].tolist() == [3, 4, 4] and got["nreads"].tolist() == [3, 4, 4]
    assert got["npairs"].tolist() == [3, 6, 6] and got["ndiscordant"].tolist() == [3, 6, 5]
    assert got["fdrp"].tolist() == [1.0, 1.0, 5.0 / 6.0]
    assert got["qfdrp"].tolist() == [(4.0 / 2.0) / 3.0, (5.0 / 2.0 + 4.0 / 3.0) / 6.0, (7.0 / 2.0) / 6.0]
    assert_same(got, fdrp_np.restate(t, "CG", flank_sites=1))


# ---- the closed form without flanking sites -----------------------------------------------------------------------------------

def test_closed_form_against_the_gpu_cx_report(ea):
    """flank_sites = 0 on rows that the read rule keeps (Z, z and '.' only): npairs = c (c - 1) / 2, ndiscordant = meth *
    unmeth of the GPU's own un-thresholded cytosine report, qfdrp == fdrp."""
    rng = np.random.default_rng(11)
    t = ragged(rng, 150, span=60, lmin=5, lmax=50, p_site=0.8)
    bam = as_bam(ea, t)
    cx = ea.rcpp_cx_report(bam, None, "Z")
    got = gpu_report(ea, bam, "CG", W=0, m=64)
    cov = cx["meth"].astype(np.int64) + cx["unmeth"]
    want = cov >= 2
    assert cov.max() <= 64 and want.sum() > 20
    for q in ("rname", "strand", "pos", "context"):
        assert np.array_equal(got[q], cx[q][want]), q
    c = cov[want]
    assert np.array_equal(got["coverage"], c) and np.array_equal(got["nreads"], c) and np.array_equal(got["npairs"], c * (c - 1) // 2)
    assert np.array_equal(got["ndiscordant"], cx["meth"][want].astype(np.int64) * cx["unmeth"][want]) and got["ndiscordant"].max() > 0
    assert np.array_equal(got["qfdrp"], got["fdrp"])
    assert np.array_equal(got["fdrp"], got["ndiscordant"].astype(np.float64) / got["npairs"].astype(np.float64))


# ---- selection -------------------------------------------------------------------------------------------------------------------

def selection_batch(c, seed=3):
    """Position 200 of sequence 2, '+', is covered by exactly c kept rows with a call (the docstring of the module has the rest)."""
    rng = np.random.default_rng(seed)
    xms, starts, strs, rns = [], [], [], []

    def add(xm, st, strand, rn=2):
        xms.append(xm); starts.append(st); strs.append(strand); rns.append(rn)

    def row_over(st, L, call):
        x = list(random_xm(rng, L, p_site=0.7, phase=st % 2))
        x[200 - st] = call
        return "".join(x)
    for _ in range(c):
        st = int(rng.integers(140, 201))
        add(row_over(st, 200 - st + int(rng.integers(1, 70)), "Z" if rng.random() < 0.5 else "z"), st, 1)
    for _ in range(60):
        st = int(rng.integers(140, 201))
        add(row_over(st, 200 - st + int(rng.integers(1, 70)), "Z" if rng.random() < 0.5 else "z"), st, 2)      # the other strand
    for _ in range(30):
        st = int(rng.integers(140, 199))
        add(row_over(st, 200 - st + int(rng.integers(1, 70)), "."), st, 1)                                      # no call at the site
        add(random_xm(rng, 200 - st, p_site=0.7, phase=st % 2), st, 1)                                          # ends in front of it
        x = row_over(st, 200 - st + 40, "Z")
        add(x[:-6] + "HHHHHH", st, 1)                                                                           # dropped by the read rule
    for rn in (1, 3):
        for _ in range(25):
            st = int(rng.integers(150, 230))
            add(random_xm(rng, int(rng.integers(10, 60)), p_site=0.7, phase=st % 2), st, int(rng.integers(1, 3)), rn)
    return H.templates_from_xm(xms, starts, strs, rns)


@pytest.mark.parametrize("c,m", [(100, 7), (100, 40), (100, 64), (40, 40), (64, 64), (41, 40), (8, 7), (65, 64), (100, 2)])
def test_selection(ea, c, m):
    t = selection_batch(c)
    got, want = check(ea, t, W=8, m=m)
    i = np.flatnonzero((want["rname"] == 2) & (want["strand"] == 1) & (want["pos"] == 200))
    assert i.size == 1 and want["coverage"][i[0]] == c and want["nreads"][i[0]] == min(c, m)
    used = want["used"][i[0]]
    assert used == sorted(used) and np.any(np.diff(used) > 1), "the covering rows are not a run of the batch"
    assert got["coverage"][i[0]] == c and got["npairs"][i[0]] == min(c, m) * (min(c, m) - 1) // 2


# ---- bit packing -----------------------------------------------------------------------------------------------------------------

def dense(rng, ns, p_gap=0.1, step=1):
    """ns sites, one every `step` positions"""
    return ("." * (step - 1)).join("." if rng.random() < p_gap else ("Z" if rng.random() < 0.5 else "z") for _ in range(ns))


def packing_batch(seed, step=1):
    """Rows of 16 .. 129 sites that start at the first site, and the same lengths again from starts inside the windows of
    the first ones: sites at bit 63 and bit 64 of a row, windows over two words, windows that start in front of a row.
    step: positions from one site to the next (9: rows above 512 bytes on average, a wave per row)."""
    rng = np.random.default_rng(seed)
    xms, starts = [], []
    for ns in (16, 17, 63, 64, 65, 128, 129):
        for first in (0, 0, int(rng.integers(1, 31)), 39, 63, 64):
            xms.append(dense(rng, ns, step=step))
            starts.append(1 + first * step)
    return H.templates_from_xm(xms, starts, [1] * len(xms))


@pytest.mark.parametrize("W,m", [(31, 64), (31, 7), (8, 40), (1, 64)])
def test_bit_packing(ea, W, m):
    t = packing_batch(17)
    got, want = check(ea, t, W=W, m=m)
    assert {64, 65, 128, 129}.issubset(set(got["pos"].tolist())) and got["coverage"].max() > 20


def test_bit_packing_long_rows(ea):
    """mean row length above 512 bytes: the kernels that take a row per wave"""
    t = packing_batch(19, step=9)
    assert t["off"][-1] > 512 * (t["off"].size - 1)
    check(ea, t, W=31, m=64)
    check(ea, t, W=5, m=9, min_overlap=3)


def test_one_long_row_among_short_ones(ea):
    rng = np.random.default_rng(23)
    xms = [dense(rng, 20) for _ in range(30)] + [dense(rng, 700, p_gap=0.3)]
    starts = [int(rng.integers(1, 60)) for _ in range(30)] + [5]
    check(ea, H.templates_from_xm(xms, starts, [1] * 31), W=31, m=64)


# ---- segments --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", [0, 3, 31])
def test_segments(ea, W):
    """Both strands of two sequences: windows are clipped at the ends of a (rname, strand) segment, and the last '+' site is
    the table neighbour of the first '-' site."""
    rng = np.random.default_rng(29)
    t = ragged(rng, 240, span=40, lmin=6, lmax=30, rnames=(1, 2), p_site=0.8)
    got, want = check(ea, t, W=W, m=64)
    s = want["sites"]
    for r in (1, 2):
        for st in (1, 2):
            P = s["pos"][(s["rname"] == r) & (s["strand"] == st)]
            G = got["pos"][(got["rname"] == r) & (got["strand"] == st)]
            assert P.size > 2 * 3 + 1 and G.size > 0
    # every site of this batch is deep enough to be reported except possibly a few at the very ends: the first and last
    # reported site of a segment have clipped windows
    assert got.nrow > 0.8 * s["pos"].size


# ---- gaps, other contexts, min_overlap -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("min_overlap", [1, 2, 5])
def test_gaps_and_min_overlap(ea, min_overlap):
    rng = np.random.default_rng(31)
    t = ragged(rng, 160, span=50, lmin=6, lmax=40, p_site=0.95, p_gap=0.25, other="xh-", p_other=0.3)
    got, want = check(ea, t, W=4, m=64, min_overlap=min_overlap)
    if min_overlap == 5:
        loose = fdrp_np.restate(t, "CG", flank_sites=4, max_reads=64)
        assert got["npairs"].sum() < loose["npairs"].sum() and got.nrow <= loose["pos"].size


def test_site_without_a_counted_pair_is_absent(ea):
    """Two rows share only the site at 9: with min_overlap = 2 its one pair does not count and the site is left out, while
    the sites that three rows share stay."""
    t = H.templates_from_xm(["Z.z.Z...Z", "........z.Z.z", "Z.Z.z", "z.Z.Z"], [1, 1, 1, 1], [1, 1, 1, 1])
    got1, _ = check(ea, t, W=2, min_overlap=1)
    got2, _ = check(ea, t, W=2, min_overlap=2)
    assert 9 in got1["pos"].tolist() and 9 not in got2["pos"].tolist() and got2["pos"].tolist() == [1, 3, 5]


# ---- max_distance, min_reads, the read rule ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_distance", [0, 1, 4, 5])
def test_max_distance(ea, max_distance):
    """Sites two bases apart, W = 4: 1 leaves the site alone (qfdrp == fdrp), 4 and 5 cut the window in half (two sites on
    either side where every even position is a site)"""
    rng = np.random.default_rng(37)
    t = ragged(rng, 120, span=40, lmin=10, lmax=40, p_site=0.9)
    got, want = check(ea, t, W=4, m=64, max_distance=max_distance)
    whole = fdrp_np.restate(t, "CG", flank_sites=4, max_reads=64)
    if max_distance == 0:
        assert_same(got, whole)
    else:
        assert np.array_equal(got["pos"], whole["pos"]) and not np.array_equal(got["qfdrp"], whole["qfdrp"])
    if max_distance == 1:
        assert np.array_equal(got["qfdrp"], got["fdrp"])


@pytest.mark.parametrize("min_reads", [0, 2, 3, 9])
def test_min_reads(ea, min_reads):
    rng = np.random.default_rng(41)
    t = ragged(rng, 60, span=80, lmin=6, lmax=30, p_site=0.8)
    got, want = check(ea, t, W=3, m=5, min_reads=min_reads, nonempty=min_reads <= 5)
    if min_reads > 5:
        assert got.nrow == 0                                  # nreads <= max_reads = 5
    else:
        assert got["nreads"].min() == max(min_reads, 2) and got["nreads"].max() == 5


def test_rows_dropped_by_the_read_rule_do_not_cover(ea):
    rng = np.random.default_rng(43)
    xms, starts = [], []
    for i in range(60):
        x = random_xm(rng, 30, p_site=0.9)
        xms.append(x[:24] + ("HHHhhh" if i % 3 == 0 else "hhhhhh"))          # 3 of 6 out-of-context calls methylated: dropped
        starts.append(1 + 2 * int(rng.integers(0, 5)))
    t = H.templates_from_xm(xms, starts, [1] * 60)
    bam = as_bam(ea, t)
    got, want = check(ea, t, W=3, m=64)
    cx = ea.rcpp_cx_report(bam, None, "Z")
    both = np.isin(cx["pos"], got["pos"])
    cov_all = (cx["meth"] + cx["unmeth"])[both]
    assert np.all(got["coverage"] <= cov_all) and (got["coverage"] < cov_all).sum() > got.nrow // 2
    got_all, _ = check(ea, t, W=3, m=64, max_oo=1.0)
    assert np.array_equal(got_all["coverage"], (cx["meth"] + cx["unmeth"])[np.isin(cx["pos"], got_all["pos"])])


@pytest.mark.parametrize("case", ["empty", "no_site", "one_row", "no_kept_row"])
def test_degenerate(ea, case):
    t = {"empty": H.templates_from_xm([], [], []),
         "no_site": H.templates_from_xm(["....", "..x..h"], [1, 3], [1, 2]),
         "one_row": H.templates_from_xm(["Z.z.Z"], [1], [1]),
         "no_kept_row": H.templates_from_xm(["Z.z.HH", "z.Z.HH"], [1, 1], [1, 1])}[case]
    got, want = check(ea, t, nonempty=False)
    assert got.nrow == 0 and want["pos"].size == 0


def test_bad_arguments_at_the_c_level(ea):
    from epialleler_amd import _lib
    t = H.templates_from_xm(["Z.z.Z", "z.Z.z"], [1, 1], [1, 1])
    bam = as_bam(ea, t)
    lib, nrow = _lib.load(), C.c_int64(0)
    for W, m, ov, dist in ((-1, 40, 1, 0), (32, 40, 1, 0), (8, 1, 1, 0), (8, 65, 1, 0), (8, 40, 0, 0), (8, 40, 18, 0), (0, 40, 2, 0), (8, 40, 1, -1)):
        assert lib.epi_batch_fdrp_report_dev(bam.batch(), b"Zz", W, m, ov, dist, 0.1, 2, None, C.byref(nrow)) == _lib.EPI_ERR_ARG
    assert lib.epi_batch_fdrp_report_dev(bam.batch(), b"Zz", 8, 40, 17, 0, 0.1, 2, None, C.byref(nrow)) == _lib.EPI_OK and nrow.value == 0
    assert lib.epi_batch_fdrp_report_dev(bam.batch(), b"Zz", 31, 64, 1, 0, 0.1, 2, None, C.byref(nrow)) == _lib.EPI_OK and nrow.value == 3


# ---- fuzz ------------------------------------------------------------------------------------------------------------------------

FUZZ_SEEDS = (1, 2, 3, 4, 5)


def fuzz_case(seed):
    """(templates, context, the arguments) of a seed"""
    rng = np.random.default_rng(1000 + seed)
    t = ragged(rng, int(rng.integers(200, 400)), span=int(rng.integers(30, 200)), lmin=1, lmax=int(rng.integers(30, 200)),
               rnames=(1, 2, 3)[:int(rng.integers(1, 4))], p_site=float(rng.uniform(0.7, 1.0)), p_meth=float(rng.uniform(0.1, 0.9)),
               p_gap=float(rng.uniform(0, 0.2)), other="xhXH", p_other=float(rng.uniform(0, 0.1)))
    W = int(rng.integers(0, 32))
    max_distance = int(rng.choice([0, 0, 3, 10, 40]))
    widest = 2 * min(W, max_distance // 2 if max_distance else W) + 1          # sites of a window (every other position is one)
    kw = dict(W=W, m=int(rng.integers(2, 65)), min_overlap=int(rng.integers(1, min(widest, 6) + 1)), max_distance=max_distance,
              min_reads=int(rng.integers(0, 6)), max_oo=float(rng.choice([0.1, 0.5, 1.0])))
    return t, str(rng.choice(["CG", "CG", "CX"])), kw


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzz(ea, seed):
    t, ctx, kw = fuzz_case(seed)
    check(ea, t, ctx=ctx, **kw)


# ---- call sequences on one batch ---------------------------------------------------------------------------------------------------

def test_sequences_on_one_batch(ea):
    import torch
    from epialleler_amd import _lib, api
    rng = np.random.default_rng(53)
    t = ragged(rng, 200, span=60, lmin=6, lmax=50, p_site=0.8)
    bam = as_bam(ea, t)
    lib, b = _lib.load(), bam.batch()
    want = fdrp_np.restate(t, "CG", flank_sites=5, max_reads=16)
    het0 = ea.rcpp_heterogeneity_report(as_bam(ea, t), "Zz", 3, 0.1)
    cx0 = ea.rcpp_cx_report(as_bam(ea, t), None, "Z")

    # report, then fetch twice
    nrow = C.c_int64(0)
    _lib.check(lib.epi_batch_fdrp_report_dev(b, b"Zz", 5, 16, 1, 0, 0.1, 2, None, C.byref(nrow)))
    first = api._fetch_table(bam, lib.epi_batch_fdrp_fetch_dev, nrow.value, 8, api.FDRP_COLUMNS, False)
    second = api._fetch_table(bam, lib.epi_batch_fdrp_fetch_dev, nrow.value, 8, api.FDRP_COLUMNS, False)
    assert_same(first, want)
    assert_same(second, want)

    # another report's fetch after this report: a call sequence error; and this fetch after another report
    ic = list(torch.empty((11, 8), dtype=torch.int32, device="cuda").unbind(0))
    dc = list(torch.empty((4, 8), dtype=torch.float64, device="cuda").unbind(0))
    assert lib.epi_batch_mhl_fetch_dev(b, api._ptr_array(ic[:5]), api._ptr_array(dc[:2]), None) == _lib.EPI_ERR_STATE
    assert lib.epi_batch_cx_fetch_dev(b, api._ptr_array(ic[:6]), None) == _lib.EPI_ERR_STATE
    assert lib.epi_batch_heterogeneity_fetch_dev(b, api._ptr_array(ic[:7]), api._ptr_array(dc), None, None) == _lib.EPI_ERR_STATE
    assert lib.epi_batch_linkage_fetch_dev(b, api._ptr_array(ic), api._ptr_array(dc[:3]), None) == _lib.EPI_ERR_STATE
    assert_same(api._fetch_table(bam, lib.epi_batch_fdrp_fetch_dev, nrow.value, 8, api.FDRP_COLUMNS, False), want)

    # a heterogeneity report, this report, a CX report: each gives its stand-alone result
    het1 = ea.rcpp_heterogeneity_report(bam, "Zz", 3, 0.1)
    assert lib.epi_batch_fdrp_fetch_dev(b, api._ptr_array(ic[:8]), api._ptr_array(dc[:2]), None) == _lib.EPI_ERR_STATE
    assert_same(gpu_report(ea, bam, "CG", W=5, m=16), want)
    cx1 = ea.rcpp_cx_report(bam, None, "Z")
    assert lib.epi_batch_fdrp_fetch_dev(b, api._ptr_array(ic[:8]), api._ptr_array(dc[:2]), None) == _lib.EPI_ERR_STATE
    het2 = ea.rcpp_heterogeneity_report(bam, "Zz", 3, 0.1)
    for q in het0:
        assert np.array_equal(het0[q], het1[q]) and np.array_equal(het0[q], het2[q]), q
    H.assert_reports_equal(cx0, cx1)
    ea.generateLinkageReport(bam, max_neighbours=2)
    assert lib.epi_batch_fdrp_fetch_dev(b, api._ptr_array(ic[:8]), api._ptr_array(dc[:2]), None) == _lib.EPI_ERR_STATE
    assert_same(gpu_report(ea, bam, "CG", W=5, m=16), want)
    assert_same(gpu_report(ea, bam, "CG", W=0, m=64), fdrp_np.restate(t, "CG", flank_sites=0, max_reads=64))     # other arguments, same batch


def test_adjust_p_values_is_untouched(ea):
    """The sort behind adjustPValues is the one this report calls: the same column gives the same bytes before and after"""
    rng = np.random.default_rng(59)
    p = rng.random(20000)
    p[rng.integers(0, p.size, 300)] = np.nan
    p[rng.integers(0, p.size, 300)] = p[rng.integers(0, p.size, 300)]
    before = {meth: np.asarray(ea.adjustPValues(p, method=meth)) for meth in ("BH", "holm", "BY")}
    t = packing_batch(61)
    check(ea, t, W=31, m=64)
    for meth, q in before.items():
        assert np.asarray(ea.adjustPValues(p, method=meth)).tobytes() == q.tobytes(), meth


# ---- call sequences that regrow, reuse and share the index buffers -------------------------------------------------------------------

def report_dev(ea, bam, ctx, W, m, min_overlap=1, max_distance=0, max_oo=0.1, min_reads=2, stream=None):
    """epi_batch_fdrp_report_dev on its own -> the table's rows"""
    from epialleler_amd import _lib
    c = H.CONTEXT_TO_BASES[ctx]
    nrow = C.c_int64(0)
    _lib.check(_lib.load().epi_batch_fdrp_report_dev(bam.batch(), (c["ctx_meth"] + c["ctx_unmeth"]).encode(), W, m, min_overlap, max_distance,
                                                     max_oo, min_reads, stream, C.byref(nrow)))
    return nrow.value


def fetch_dev(ea, bam, nrow):
    """epi_batch_fdrp_fetch_dev on its own (on torch's current stream)"""
    from epialleler_amd import _lib, api
    return api._fetch_table(bam, _lib.load().epi_batch_fdrp_fetch_dev, nrow, 8, api.FDRP_COLUMNS, False)


def other_contexts_batch(seed, nrow=250):
    return ragged(np.random.default_rng(seed), nrow, span=80, lmin=6, lmax=60, rnames=(1, 2), p_site=0.8, p_gap=0.1, other="hH", p_other=0.5)


def test_changing_contexts_on_one_batch(ea):
    """CG, CX, CHH, then CG again on one batch: tables of other sizes over the same index buffers"""
    t = other_contexts_batch(67)
    bam = as_bam(ea, t)
    sizes = []
    for ctx in ("CG", "CX", "CHH", "CG"):
        want = fdrp_np.restate(t, ctx, flank_sites=4, max_reads=16, max_oo=1.0)
        assert want["pos"].size > 20 and want["ndiscordant"].max() > 0
        assert_same(gpu_report(ea, bam, ctx, W=4, m=16, max_oo=1.0), want, ctx)
        sizes.append(int(want["sites"]["pos"].size))
    assert len(set(sizes)) == 3


def test_a_small_table_after_a_large_one_and_back(ea):
    """The 65537-site batch of test_gpu_fdrp_seams.py with four rows of a further sequence that hold the batch's only CHH
    calls: 3 sites, 65537 sites (every index buffer regrown), 3 sites (reused by a smaller call), 65537 sites"""
    import test_gpu_fdrp_seams as S
    big = S.table_batch(65537)
    tail = H.templates_from_xm(["H.h.H", "h.H.h", "H.H.h", "h.h.H"], [1, 1, 1, 1], [1, 1, 1, 1], [9, 9, 9, 9])
    t = {"xm": np.concatenate((big["xm"], tail["xm"])), "off": np.concatenate((big["off"], big["off"][-1] + tail["off"][1:]))}
    for q in ("rname", "strand", "start"):
        t[q] = np.concatenate((big[q], tail[q]))
    want_big = fdrp_np.restate_indexed(t, "CG", flank_sites=8, max_reads=40)
    want_small = fdrp_np.restate(t, "CHH", flank_sites=1, max_reads=3, max_oo=1.0)
    assert want_big["sites"]["pos"].size == 65537 == want_big["pos"].size
    assert want_small["sites"]["pos"].size == 3 == want_small["pos"].size and want_small["ndiscordant"].min() > 0
    bam = as_bam(ea, t)
    for _ in range(2):
        assert_same(gpu_report(ea, bam, "CHH", W=1, m=3, max_oo=1.0), want_small, "3 sites")
        assert_same(gpu_report(ea, bam, "CG", W=8, m=40), want_big, "65537 sites")


def test_after_an_empty_report(ea):
    """An empty table with its fetch, then a table with rows, on one batch: empty because no site has min_reads rows (the
    whole report runs), and empty because the read rule drops every row (the report ends after its first step)"""
    import torch
    from epialleler_amd import _lib, api
    rng = np.random.default_rng(71)
    xms, starts = [], []
    for _ in range(150):
        st = int(rng.integers(1, 60))
        xms.append(random_xm(rng, int(rng.integers(8, 50)), p_site=0.85, phase=st % 2) + "H")
        starts.append(st)
    t = H.templates_from_xm(xms, starts, [1] * 150)
    bam = as_bam(ea, t)
    lib, b = _lib.load(), bam.batch()
    ic = list(torch.empty((8, 0), dtype=torch.int32, device="cuda").unbind(0))
    dc = list(torch.empty((2, 0), dtype=torch.float64, device="cuda").unbind(0))
    want = fdrp_np.restate(t, "CG", flank_sites=6, max_reads=5, max_oo=1.0)
    assert want["pos"].size > 20 and want["ndiscordant"].max() > 0
    for empty in (dict(min_reads=9, max_oo=1.0), dict(max_oo=0.0), dict(min_reads=9, max_oo=1.0)):
        assert fdrp_np.restate(t, "CG", flank_sites=6, max_reads=5, **empty)["pos"].size == 0
        assert report_dev(ea, bam, "CG", 6, 5, **empty) == 0
        assert lib.epi_batch_fdrp_fetch_dev(b, api._ptr_array(ic), api._ptr_array(dc), None) == _lib.EPI_OK
        assert_same(gpu_report(ea, bam, "CG", W=6, m=5, max_oo=1.0), want, str(empty))


def test_two_batches_interleaved(ea):
    """report A, report B, fetch A, fetch B: every batch has its own index"""
    ta, tb = other_contexts_batch(73, 300), other_contexts_batch(79, 90)
    a, b = as_bam(ea, ta), as_bam(ea, tb)
    wa = fdrp_np.restate(ta, "CG", flank_sites=8, max_reads=40, max_oo=1.0)
    wb = fdrp_np.restate(tb, "CX", flank_sites=2, max_reads=7, max_oo=1.0)
    assert min(wa["pos"].size, wb["pos"].size) > 20 and wa["pos"].size != wb["pos"].size
    for _ in range(2):
        na = report_dev(ea, a, "CG", 8, 40, max_oo=1.0)
        nb = report_dev(ea, b, "CX", 2, 7, max_oo=1.0)
        assert_same(fetch_dev(ea, a, na), wa, "A")
        assert_same(fetch_dev(ea, b, nb), wb, "B")
        nb = report_dev(ea, b, "CX", 2, 7, max_oo=1.0)
        na = report_dev(ea, a, "CG", 8, 40, max_oo=1.0)
        assert_same(fetch_dev(ea, a, na), wa, "A after B")
        assert_same(fetch_dev(ea, b, nb), wb, "B before A")


def test_on_a_side_stream(ea):
    """The report and the fetch queued through the C entry points on a stream that is not the default one"""
    import torch
    t = packing_batch(83)
    want = fdrp_np.restate(t, "CG", flank_sites=31, max_reads=64)
    s = torch.cuda.Stream()
    assert s.cuda_stream != torch.cuda.default_stream().cuda_stream
    with torch.cuda.stream(s):
        bam = as_bam(ea, t)
        nrow = report_dev(ea, bam, "CG", 31, 64, stream=C.c_void_p(s.cuda_stream))
        got = fetch_dev(ea, bam, nrow)
    s.synchronize()
    assert got.nrow > 0
    assert_same(got, want)
    assert_same(gpu_report(ea, bam, "CG", W=31, m=64), want, "then on the default stream")


def test_a_batch_set_up_for_a_sharded_report_is_refused(ea):
    """Shared tiles attached (the setup of test_gpu_sharded.py's single-rank worker): EPI_ERR_STATE, and the batch still
    serves the sharded CX report and, once that has detached the tiles, this report"""
    from epialleler_amd import _lib, distributed as D
    t = H.bam("amplicon010meth.bam")
    bam = as_bam(ea, t, t.get("levels"))
    eng = D.HipShardEngine(bam)
    first, last = eng.key_range()
    keys = np.array([k for k in range(first, first + 4) if (k >> 32) == (first >> 32) and k <= last], dtype=np.int64)
    owned = np.ones(keys.size, dtype=np.int32)
    assert keys.size > 0
    eng._attach_cx_slab(keys, owned, "Z")
    nrow = C.c_int64(7)
    assert _lib.load().epi_batch_fdrp_report_dev(bam.batch(), b"Zz", 8, 40, 1, 0, 0.1, 2, None, C.byref(nrow)) == _lib.EPI_ERR_STATE
    assert nrow.value == 0 and b"sharded" in _lib.load().epi_last_error()
    slab = eng.cx_accumulate(None, "Z", keys, owned)
    assert int(slab.abs().sum()) > 0
    cols = eng.cx_finish("Z")
    sites = fdrp_np.site_table(t, "CG")
    for i, q in enumerate(("rname", "strand", "pos", "context", "meth", "unmeth")):
        assert np.array_equal(cols[i].cpu().numpy(), sites[q]), q
    want = fdrp_np.restate(t, "CG")
    assert want["pos"].size > 0
    assert_same(gpu_report(ea, bam, "CG"), want)


def test_adjust_p_values_between_report_and_fetch(ea):
    """adjustPValues on 70 000 values (18 sorting tiles, its own pass plan) between this report and its fetch, on one engine"""
    import padjust_np
    p = np.random.default_rng(89).random(70000)
    t = other_contexts_batch(97, 300)
    want = fdrp_np.restate(t, "CG", flank_sites=8, max_reads=40, max_oo=1.0)
    assert want["pos"].size > 20
    bam = as_bam(ea, t)
    nrow = report_dev(ea, bam, "CG", 8, 40, max_oo=1.0)
    q = np.asarray(ea.adjustPValues(p, method="BH"))
    assert_same(fetch_dev(ea, bam, nrow), want)
    np.testing.assert_array_equal(q, padjust_np.adjust_np(p, "BH")[0])


# ---- delivery ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gz", [False, True])
def test_file_output_and_device_table(ea, tmp_path, gz):
    t = H.bam("amplicon010meth.bam")
    levels = t.get("levels") or ["chr%d" % i for i in range(1, 100)]
    bam = as_bam(ea, t, levels)
    want = fdrp_np.restate(t, "CG")
    rep = ea.generateFdrpReport(bam)
    assert_same(rep, want)
    assert rep.nrow > 0
    p = tmp_path / ("fdrp.tsv.gz" if gz else "fdrp.tsv")
    assert ea.generateFdrpReport(bam, report_file=str(p), gzip=gz) is None
    lines = (gzip.open(p, "rt") if gz else open(p)).read().split("\n")
    assert lines[0] == "\t".join(INT_COLS + FLOAT_COLS) and len(lines) == rep.nrow + 2 and lines[-1] == ""
    cells = [ln.split("\t") for ln in lines[1:-1]]
    assert all(c[1] in "+-" and c[3] == "CG" for c in cells)
    for j, q in enumerate(INT_COLS):
        if q not in ("rname", "strand", "context"):
            assert [int(c[j]) for c in cells] == rep[q].tolist(), q
    for j, q in ((8, "fdrp"), (9, "qfdrp")):
        assert np.allclose([float(c[j]) for c in cells], rep[q], atol=1e-12), q
    dev = ea.generateFdrpReport(bam, as_device=True)
    for q in INT_COLS + FLOAT_COLS:
        assert dev[q].is_cuda and np.array_equal(dev[q].cpu().numpy(), rep[q]), q
