"""compareHeterogeneity against a plain restatement of its definitions (include/epihip.h,
epi_batch_heterogeneity_compare_dev): loops over rows and numpy.  The restatement's site tables are the CPU restatement's
cx_report with an all-ones pass vector, its kept rows are helpers.mhl_keep_np, the common sites a set intersection on
(rname, strand, pos, context); nothing in it reads a GPU result.  Integer columns, df and the histograms compare
exactly.  The float columns bounded by 1 in magnitude within 1e-12 absolute: each is a sum of at most 128 terms below 1,
every term within a few ulp (2.2e-16) of the float64 value (or the difference of two such sums).  g within
1e-12 N max(1, ln N), N = n_a + n_b: at most 128 terms, each bounded by N ln N and a few ulp wide."""
import ctypes as C
import functools

import numpy as np
import pytest

import helpers as H
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

INT_COLS = ("rname", "strand", "pos", "end", "context", "nreads_a", "nreads_b", "npatterns_a", "npatterns_b", "df")
SAMPLE_COLS = ("beta", "entropy", "epipolymorphism", "pdr")
FLOAT_COLS = tuple(q + s for q in SAMPLE_COLS for s in ("_a", "_b")) + ("delta_beta", "delta_entropy", "jsd", "tvd", "g")
ATOL = 1e-12


@pytest.fixture(scope="module")
def ea():
    import epialleler_amd
    return epialleler_amd


# ---- the restatement -------------------------------------------------------------------------------------------------

def site_table(t, ctx):
    """The un-thresholded cytosine report's rname, strand, pos, context."""
    n = t["off"].size - 1
    cx = orc.cx_report(np.asarray(t["xm"], np.uint8), t["off"], t["rname"], t["strand"], t["start"], np.ones(max(n, 1), np.int32)[:n],
                       H.CONTEXT_TO_BASES[ctx]["ctx_meth"])
    return {q: np.asarray(cx[q]) for q in ("rname", "strand", "pos", "context")}


def site_keys(s):
    return list(zip(s["rname"].tolist(), s["strand"].tolist(), s["pos"].tolist(), s["context"].tolist()))


def window_counts(t, ctx, sites, k, max_oo):
    """counts [site row][2^k] of the kept rows of t for the window that starts at each row of `sites`, the window's last
    position and whether the row starts a window at all."""
    c = H.CONTEXT_TO_BASES[ctx]
    n = t["off"].size - 1
    xm = np.asarray(t["xm"], np.uint8)
    keep = H.mhl_keep_np(xm, t["off"], c["ctx_meth"] + c["ctx_unmeth"], 0, max_oo) if n else np.zeros(0, bool)
    N = sites["pos"].size
    counts = np.zeros((N, 1 << k), np.int64)
    end = np.zeros(N, np.int64)
    is_window = np.zeros(N, bool)
    weights = 1 << np.arange(k)
    for r in np.unique(sites["rname"]):
        for s in (1, 2):
            rows = np.flatnonzero((sites["rname"] == r) & (sites["strand"] == s))
            P = sites["pos"][rows].astype(np.int64)
            assert np.all(np.diff(P) > 0)
            code = sites["context"][rows]
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
    return counts, end, is_window


def sample_metrics(cn, k):
    nb = 1 << k
    nr = cn.sum(axis=1).astype(np.float64)
    popc = np.asarray([bin(p).count("1") for p in range(nb)], np.float64)
    p = cn / nr[:, None] if cn.size else np.zeros((0, nb))
    with np.errstate(divide="ignore", invalid="ignore"):
        plogp = np.where(p > 0, p * np.log2(p), 0.0)
    return {"nreads": cn.sum(axis=1).astype(np.int32), "npatterns": (cn > 0).sum(axis=1).astype(np.int32),
            "beta": (cn * popc).sum(axis=1) / (nr * k), "entropy": -plogp.sum(axis=1) / k,
            "epipolymorphism": 1.0 - (p * p).sum(axis=1), "pdr": 1.0 - (cn[:, 0] + cn[:, nb - 1]) / nr}, p, nr


def restate(ta, tb, ctx, k, max_oo=0.1, min_reads=1, max_span=0):
    """The comparison of the templates ta and tb: dict of the 23 columns plus counts_a, counts_b [nrow, 2^k], `sites` (the
    common table) and sites_a, sites_b (either sample's own)."""
    sa, sb = site_table(ta, ctx), site_table(tb, ctx)
    in_b = set(site_keys(sb))
    common = np.asarray([q in in_b for q in site_keys(sa)], bool)
    sites = {q: sa[q][common] for q in sa}
    ca, end, is_window = window_counts(ta, ctx, sites, k, max_oo)
    cb, end_b, is_window_b = window_counts(tb, ctx, sites, k, max_oo)
    assert np.array_equal(end, end_b) and np.array_equal(is_window, is_window_b)
    span = end - sites["pos"].astype(np.int64) + 1
    lo = max(min_reads, 1)
    rep = is_window & (ca.sum(axis=1) >= lo) & (cb.sum(axis=1) >= lo) & ((span <= max_span) if max_span else True)
    ca, cb = ca[rep], cb[rep]
    out = {"rname": sites["rname"][rep], "strand": sites["strand"][rep], "pos": sites["pos"][rep], "end": end[rep].astype(np.int32),
           "context": sites["context"][rep]}
    (ma, p, na), (mb, q, nb) = sample_metrics(ca, k), sample_metrics(cb, k)
    for name in ma:
        out[name + "_a"], out[name + "_b"] = ma[name], mb[name]
    out["df"] = ((ca + cb) > 0).sum(axis=1).astype(np.int32) - 1
    out["delta_beta"] = mb["beta"] - ma["beta"]
    out["delta_entropy"] = mb["entropy"] - ma["entropy"]
    m = (p + q) / 2
    tot = (na + nb)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        js = np.where(p > 0, 0.5 * p * np.log2(p / m), 0.0) + np.where(q > 0, 0.5 * q * np.log2(q / m), 0.0)
        ea_, eb_ = na[:, None] * (ca + cb) / tot, nb[:, None] * (ca + cb) / tot
        g = np.where(ca > 0, ca * np.log(ca / ea_), 0.0).sum(axis=1) + np.where(cb > 0, cb * np.log(cb / eb_), 0.0).sum(axis=1)
    out["jsd"] = np.clip(js.sum(axis=1), 0.0, 1.0)
    out["tvd"] = 0.5 * np.abs(p - q).sum(axis=1)
    out["g"] = 2.0 * g
    out.update(counts_a=ca.astype(np.int32), counts_b=cb.astype(np.int32), sites=sites, sites_a=sa, sites_b=sb,
               ncommon=int(common.sum()))
    return out


def as_bam(ea, t, levels=None):
    """(No levels unless asked for: the fixtures of different experiments name different sequences.)"""
    return ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"], levels)


def gpu_compare(ea, bam_a, bam_b, ctx, k, max_oo=0.1, min_reads=1, max_span=0):
    c = H.CONTEXT_TO_BASES[ctx]
    return ea.rcpp_heterogeneity_compare(bam_a, bam_b, c["ctx_meth"] + c["ctx_unmeth"], k, max_oo, min_reads, max_span, with_counts=True)


def gpu_single(ea, bam, ctx, k, max_oo=0.1, min_reads=1, max_span=0):
    c = H.CONTEXT_TO_BASES[ctx]
    return ea.rcpp_heterogeneity_report(bam, c["ctx_meth"] + c["ctx_unmeth"], k, max_oo, min_reads, max_span, with_counts=True)


def g_tol(want):
    n = (want["nreads_a"].astype(np.float64) + want["nreads_b"])
    return 1e-12 * n * np.maximum(1.0, np.log(n))


def assert_same(got, want, what=""):
    assert list(got.keys()) == list(INT_COLS + FLOAT_COLS)
    assert got.ncommon == want["ncommon"], (what, "ncommon")
    for q in INT_COLS:
        assert got[q].dtype == np.int32 and np.array_equal(got[q], want[q]), (what, q)
    for q in FLOAT_COLS:
        assert got[q].dtype == np.float64 and got[q].shape == want[q].shape, (what, q)
        err = np.abs(got[q] - want[q])
        print(what, q, "max error", float(err.max()) if err.size else 0.0)
        assert np.all(err <= (g_tol(want) if q == "g" else ATOL)), (what, q, float(err.max()))
    assert np.all((got["jsd"] >= 0) & (got["jsd"] <= 1))
    for s in ("a", "b"):
        c = getattr(got, "counts_" + s)
        assert c.dtype == np.int32 and np.array_equal(c, want["counts_" + s]), (what, "counts_" + s)


def exercises(want):
    """(Two empty tables would compare equal.)"""
    return want["pos"].size > 0 and bool(np.any(want["jsd"] > 0)) and bool(np.any(want["npatterns_a"] > 1) or np.any(want["npatterns_b"] > 1))


def check(ea, ta, tb, ctx, k, nonempty=True, **kw):
    want = restate(ta, tb, ctx, k, **kw)
    if nonempty:
        assert exercises(want), "the case exercises nothing"
    got = gpu_compare(ea, as_bam(ea, ta), as_bam(ea, tb), ctx, k, **kw)
    assert_same(got, want, (ctx, k, kw))
    return got, want


def assert_empty(got, k, ncommon):
    assert list(got.keys()) == list(INT_COLS + FLOAT_COLS) and got.nrow == 0 and got.ncommon == ncommon
    assert got.counts_a.shape == (0, 1 << k) and got.counts_b.shape == (0, 1 << k)


# ---- the reference's fixtures ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def fixture_want(name_a, name_b, ctx, k):
    return restate(H.bam(name_a + ".bam"), H.bam(name_b + ".bam"), ctx, k)


PAIRS = {"000-010": ("amplicon000meth", "amplicon010meth"), "010-100": ("amplicon010meth", "amplicon100meth")}
# what the restatement gives on the CPU: common CG sites, and per k = 2, 4, 6 (reported windows, of which jsd > 0)
FIXTURE_COMMON = {"000-010": 128, "010-100": 160}
FIXTURE_WINDOWS = {"000-010": ((115, 75), (91, 61), (75, 51)), "010-100": ((143, 140), (110, 110), (84, 84))}


@pytest.mark.parametrize("k", [2, 4, 6])
@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_fixture_pairs_cg(ea, pair, k):
    na, nb = PAIRS[pair]
    want = fixture_want(na, nb, "CG", k)
    assert exercises(want)
    assert want["ncommon"] == FIXTURE_COMMON[pair]
    nwin, npos = FIXTURE_WINDOWS[pair][k // 2 - 1]
    assert want["pos"].size == nwin
    assert int(np.count_nonzero(want["jsd"] > 0)) == npos
    if pair == "000-010":
        assert (want["sites_a"]["pos"].size, want["sites_b"]["pos"].size) == (543, 478)
        if k == 4:
            assert (int(want["nreads_a"].max()), int(want["nreads_b"].max())) == (154, 155)       # the deepest windows
    assert_same(gpu_compare(ea, as_bam(ea, H.bam(na + ".bam")), as_bam(ea, H.bam(nb + ".bam")), "CG", k), want, (pair, k))


def test_fixture_pair_three_contexts(ea):
    """CX, k = 3: one position has another majority context in the second sample and is not common."""
    na, nb = PAIRS["000-010"]
    want = fixture_want(na, nb, "CX", 3)
    assert exercises(want) and (want["ncommon"], want["pos"].size) == (1217, 1190)
    pos_of = lambda s: {q[:3]: q[3] for q in site_keys(s)}
    pa, pb = pos_of(want["sites_a"]), pos_of(want["sites_b"])
    differ = [q for q in pa if q in pb and pa[q] != pb[q]]
    assert len(differ) == 1
    assert differ[0] not in pos_of(want["sites"])
    assert_same(gpu_compare(ea, as_bam(ea, H.bam(na + ".bam")), as_bam(ea, H.bam(nb + ".bam")), "CX", 3), want, "CX")


# ---- a batch against itself ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("second_upload", [False, True])
def test_batch_against_itself(ea, second_upload):
    t = H.bam("amplicon010meth.bam")
    bam = as_bam(ea, t)
    other = as_bam(ea, t) if second_upload else bam
    for ctx, k in (("CG", 4), ("CX", 2)):
        single = gpu_single(ea, bam, ctx, k)
        assert single.nrow > 0 and np.any(single["npatterns"] > 1)
        got = gpu_compare(ea, bam, other, ctx, k)
        assert got.ncommon == site_table(t, ctx)["pos"].size
        for q in ("rname", "strand", "pos", "end", "context"):
            assert np.array_equal(got[q], single[q]), q
        for s in ("_a", "_b"):
            for q in ("nreads", "npatterns") + SAMPLE_COLS:
                assert np.array_equal(got[q + s], single[q]), q + s
        assert np.array_equal(got.counts_a, single.counts) and np.array_equal(got.counts_b, single.counts)
        assert np.array_equal(got["df"], single["npatterns"] - 1)
        for q in ("jsd", "tvd", "g", "delta_beta", "delta_entropy"):
            assert np.all(got[q] == 0.0), q


# ---- hand-made batches ----------------------------------------------------------------------------------------------------

def every_other(rng, nsites, p_meth=0.5, step=2, only=None):
    """A row with a CG call at every step-th position, '.' between; only: the site numbers that get a call at all."""
    calls = np.where(rng.random(nsites) < p_meth, "Z", "z")
    if only is not None:
        calls = np.where(np.isin(np.arange(nsites), only), calls, ".")
    return "".join(ch + "." * (step - 1) for ch in calls)


def test_no_common_site(ea):
    ta, tb = H.bam("amplicon010meth.bam"), H.bam("capture.bam")
    want = restate(ta, tb, "CG", 4)
    assert want["ncommon"] == 0 and want["sites_a"]["pos"].size > 0 and want["sites_b"]["pos"].size > 0
    assert_empty(gpu_compare(ea, as_bam(ea, ta), as_bam(ea, tb), "CG", 4), 4, 0)
    assert_empty(gpu_compare(ea, as_bam(ea, tb), as_bam(ea, ta), "CG", 4), 4, 0)


def test_fewer_common_sites_than_a_window(ea):
    k = 4
    ta = H.templates_from_xm(["Z.z.Z.z.Z.z", "z.Z.z.Z.z.Z"], [1, 1], [1, 1])            # sites 1, 3, ..., 11
    tb = H.templates_from_xm(["Z...Z...Z", "z...z...Z", ".Z"], [1, 1, 20], [1, 1, 1])    # sites 1, 5, 9 common, and 21
    want = restate(ta, tb, "CG", k)
    assert want["ncommon"] == k - 1 and want["pos"].size == 0
    bam_a, bam_b = as_bam(ea, ta), as_bam(ea, tb)
    assert_empty(gpu_compare(ea, bam_a, bam_b, "CG", k), k, k - 1)
    check(ea, ta, tb, "CG", 3)                                                          # ... and exactly a window
    # a batch without a row, and one without a site
    for tz in (H.templates_from_xm([], [], []), H.templates_from_xm(["....", "..x..h"], [1, 3], [1, 2])):
        assert_empty(gpu_compare(ea, bam_a, as_bam(ea, tz), "CG", k), k, 0)
        assert_empty(gpu_compare(ea, as_bam(ea, tz), bam_a, "CG", k), k, 0)


def test_strands(ea):
    rng = np.random.default_rng(21)
    plus = lambda n, s=1: ([every_other(rng, 8) for _ in range(n)], [1 + 2 * int(v) for v in rng.integers(0, 4, n)], [s] * n)
    join = lambda *parts: H.templates_from_xm(*[sum((list(p[i]) for p in parts), []) for i in range(3)])
    # '+' rows only in a, '-' rows only in b: both have sites, none is common
    ta, tb = join(plus(12, 1)), join(plus(12, 2))
    want = restate(ta, tb, "CG", 3)
    assert want["ncommon"] == 0 and want["sites_a"]["pos"].size > 3 and want["sites_b"]["pos"].size > 3
    assert_empty(gpu_compare(ea, as_bam(ea, ta), as_bam(ea, tb), "CG", 3), 3, 0)
    # common sites on one strand only, either one; the other strand's sites are a's (or b's) alone
    for s in (1, 2):
        ta, tb = join(plus(12, 1), plus(12, 2)), join(plus(12, s))
        for x, y in ((ta, tb), (tb, ta)):
            got, want = check(ea, x, y, "CG", 3)
            assert set(got["strand"].tolist()) == {s}


def test_sequence_end_inside_a_window(ea):
    """Two sequences; in each strand's table the last sites of sequence 1 and the first of sequence 2 are neighbours: no
    window joins them, also where the intersection has removed every other site of sequence 2 (b's rows start at multiples
    of 4 there and call every other site of a's)."""
    rng = np.random.default_rng(22)
    xa, xb, starts, strands, rnames = [], [], [], [], []
    for r in (1, 2):
        for s in (1, 2):
            for _ in range(12):
                starts.append((2 if r == 1 else 4) * int(rng.integers(1, 6)) + (s - 1)); strands.append(s); rnames.append(r)
                xa.append(every_other(rng, 10, 0.3))
                xb.append(every_other(rng, 10, 0.7, only=np.arange(0, 10) if r == 1 else np.arange(0, 10, 2)))
    ta, tb = H.templates_from_xm(xa, starts, strands, rnames), H.templates_from_xm(xb, starts, strands, rnames)
    for k in (3, 5):
        got, want = check(ea, ta, tb, "CG", k)
        sites = want["sites"]
        for r in (1, 2):
            for s in (1, 2):
                m = np.count_nonzero((sites["rname"] == r) & (sites["strand"] == s))
                assert m >= k and np.count_nonzero((got["rname"] == r) & (got["strand"] == s)) <= m - k + 1
        assert np.all(got["end"] > got["pos"])


def test_windows_span_a_site_the_other_sample_lacks(ea):
    a_rows = ["Z.z.Z.z.Z.z",       # six sites at 1, 3, ..., 11
              "z.Z.z.Z.z.Z",
              "Z.z.z.Z.z.Z",       # position 5, which b lacks: a call ...
              "Z.z...Z.Z.z",       # ... a '.'
              "z.Z.h.z.z.Z",       # ... another context: all three count in the windows over it
              "Z.z.-.z.Z.z"]
    b_rows = ["Z.z...z.Z.z",       # no call at 5 in any row: not a site of b
              "z.z...Z.z.Z",
              "Z.Z...Z.Z.z"]
    ta = H.templates_from_xm(a_rows, [1] * 6, [1] * 6)
    tb = H.templates_from_xm(b_rows, [1] * 3, [1] * 3)
    for k in (2, 3):
        got, want = check(ea, ta, tb, "CG", k, max_oo=1.0)
        assert want["sites_a"]["pos"].tolist() == [1, 3, 5, 7, 9, 11] and want["sites"]["pos"].tolist() == [1, 3, 7, 9, 11]
    got, want = check(ea, ta, tb, "CG", 3, max_oo=1.0)
    assert got["pos"].tolist() == [1, 3, 7] and got["end"].tolist() == [7, 9, 11]
    assert got["nreads_a"].tolist() == [6, 6, 6] and got["nreads_b"].tolist() == [3, 3, 3]
    # the span is that of the common sites: 1 .. 7 is 7 wide, 3 .. 9 too, 7 .. 11 is 5 wide
    got, want = check(ea, ta, tb, "CG", 3, max_oo=1.0, max_span=6, nonempty=False)
    assert got["pos"].tolist() == [7]
    got, want = check(ea, ta, tb, "CG", 3, max_oo=1.0, max_span=7)
    assert got["pos"].tolist() == [1, 3, 7]
    single = gpu_single(ea, as_bam(ea, ta), "CG", 3, max_oo=1.0)
    assert single["end"].tolist()[:2] == [5, 7]           # (a's own windows are others)


@pytest.mark.parametrize("k", [2, 6])
def test_table_sparser_than_a_rows_own_sites(ea, k):
    """a's rows have 100 sites of their own; b has every eighth of them, so a row of a finds about 13 common sites (less than
    one round of 16 lanes) among its bytes.  Swapped, b's sparse rows are counted on the same table."""
    rng = np.random.default_rng(23)
    starts = [1 + 16 * int(v) for v in rng.integers(0, 6, 40)]
    xa = [every_other(rng, 100, 0.35) for _ in range(40)]
    xb = [every_other(rng, 100, 0.65, only=np.arange(0, 100, 8)) for _ in range(40)]
    ta, tb = H.templates_from_xm(xa, starts, [1] * 40), H.templates_from_xm(xb, starts, [1] * 40)
    got, want = check(ea, ta, tb, "CG", k)
    assert want["sites_a"]["pos"].size > 64 * 2 and 13 <= want["ncommon"] <= 64 and np.all(np.diff(want["sites"]["pos"]) == 16)
    check(ea, tb, ta, "CG", k)


@pytest.mark.parametrize("k", [2, 6])
def test_rounds_of_64_common_sites(ea, k):
    """Rows of 100 sites in both samples, piled at starts 1, 3, 5, ...: more than one round of 16 and of 64 common sites
    per row, and windows that straddle the 64th site (the carry between rounds)."""
    rng = np.random.default_rng(24)
    starts = [1 + 2 * i for i in range(40)]
    ta = H.templates_from_xm([every_other(rng, 100, 0.3 + 0.4 * (i % 2)) for i in range(40)], starts, [1] * 40)
    tb = H.templates_from_xm([every_other(rng, 100, 0.6) for i in range(40)], starts, [1] * 40)
    got, want = check(ea, ta, tb, "CG", k)
    assert want["ncommon"] == 139
    for site in (64, 128):
        i = np.flatnonzero(want["pos"] == 1 + 2 * (site - k + 1))
        assert i.size == 1 and want["nreads_a"][i[0]] >= 1 and want["nreads_b"][i[0]] >= 1


def test_lane_shapes_differ(ea):
    """a: rows of 40 to 120 bytes (16 lanes take a row); b: rows of 1200 to 2400 bytes, mean above 512 (a wave takes a row).
    Both orders."""
    rng = np.random.default_rng(25)
    xb = ["".join(("Z" if rng.random() < 0.6 else "z") + ".." for _ in range(int(rng.integers(400, 800)))) for _ in range(30)]
    sb = [1 + 3 * int(v) for v in rng.integers(0, 200, 30)]
    xa, sa = [], []
    for _ in range(300):
        sa.append(1 + 3 * int(rng.integers(0, 700)))
        xa.append("".join(("Z" if rng.random() < 0.3 else "z") + ".." for _ in range(int(rng.integers(14, 40)))))
    ta, tb = H.templates_from_xm(xa, sa, [1] * 300), H.templates_from_xm(xb, sb, [1] * 30)
    assert ta["xm"].size <= 512 * 300 and tb["xm"].size > 512 * 30
    for k in (2, 5):
        check(ea, ta, tb, "CG", k)
        check(ea, tb, ta, "CG", k)


def test_min_reads_on_both_sides(ea):
    rng = np.random.default_rng(26)
    track = "".join(rng.choice(list("C..."), 400))
    def rows(n, lo, hi, p):
        xms, starts = [], []
        for _ in range(n):
            s = int(rng.integers(lo, hi))
            xms.append("".join((("Z" if rng.random() < p else "z") if ch == "C" else ".") for ch in track[s - 1:s - 1 + int(rng.integers(40, 100))]))
            starts.append(s)
        return H.templates_from_xm(xms, starts, [1] * n)
    ta, tb = rows(300, 1, 300, 0.4), rows(25, 1, 300, 0.6)          # deep everywhere; shallow
    full, wfull = check(ea, ta, tb, "CG", 4)
    sel = (full["nreads_a"] >= 4) & (full["nreads_b"] >= 4)
    assert np.any(sel) and np.any((full["nreads_a"] >= 4) & (full["nreads_b"] < 4)) and np.all(full["nreads_a"][~sel] >= 4)
    for x, y, sfx in ((ta, tb, ("_a", "_b")), (tb, ta, ("_b", "_a"))):
        got, want = check(ea, x, y, "CG", 4, min_reads=4)
        assert np.array_equal(got["pos"], full["pos"][sel])
        assert np.array_equal(got["nreads" + sfx[0]], full["nreads_a"][sel]) and np.array_equal(got["nreads" + sfx[1]], full["nreads_b"][sel])
    span = full["end"] - full["pos"] + 1
    cut = int(np.median(span))
    got, want = check(ea, ta, tb, "CG", 4, min_reads=2, max_span=cut)
    keep = (full["nreads_a"] >= 2) & (full["nreads_b"] >= 2) & (span <= cut)
    assert 0 < np.count_nonzero(keep) < keep.size
    for q in INT_COLS + FLOAT_COLS:
        assert np.array_equal(got[q], full[q][keep]), q
    assert np.array_equal(got.counts_b, full.counts_b[keep])
    for mr in (0, -3):                                              # below 1: as 1
        got0 = gpu_compare(ea, as_bam(ea, ta), as_bam(ea, tb), "CG", 4, min_reads=mr)
        assert np.array_equal(got0["pos"], full["pos"]) and np.array_equal(got0["g"], full["g"])


def test_contention_on_a_foreign_table(ea):
    """2 000 identical rows in one sample, a handful of different ones in the other: the rows of a wave hold the same counter
    of a table that is not their batch's own (it lacks the pile's site at 104)."""
    pile = "Z.Z.zzZ.z.Z"                                   # sites 100, 102, 104, 105, 106, 108, 110 of the pile alone
    few = ["z.z...Z.z.Z", "Z.Z...z.Z.z", "Z.Z..zZ.z.z", "z.Z..zz.z.Z", "Z.z..ZZ.Z.z"]
    ta = H.templates_from_xm([pile] * 2000, [100] * 2000, [1] * 2000)
    tb = H.templates_from_xm(few, [100] * 5, [1] * 5)
    for x, y, deep in ((ta, tb, "nreads_a"), (tb, ta, "nreads_b")):
        got, want = check(ea, x, y, "CG", 4)
        assert want["sites"]["pos"].tolist() == [100, 102, 105, 106, 108, 110] and 104 in site_table(ta, "CG")["pos"]
        assert got.nrow == 3 and np.all(got[deep] == 2000)


def swapped(rep):
    out = {}
    for q in rep.keys():
        if q.endswith("_a"):
            out[q] = rep[q[:-2] + "_b"]
        elif q.endswith("_b"):
            out[q] = rep[q[:-2] + "_a"]
        elif q.startswith("delta_"):
            out[q] = -rep[q]
        else:
            out[q] = rep[q]
    return out


def fuzz_pair(seed, nrows=(400, 300)):
    """Two batches over one grid of sites on two sequences and both strands: either sample drops a tenth of the sites (its
    rows show '.' there) and a few change context; rows of 30 to 300 bytes, methylated at the sample's own rate, 4 % of the
    bytes replaced."""
    rng = np.random.default_rng(7100 + seed)
    glen = 3000
    letters = np.asarray(list(".zxh"))
    track = [letters[rng.choice(4, glen, p=[0.72, 0.16, 0.07, 0.05])] for _ in range(2)]
    noise = np.asarray(list(".-zZxXhHuU"))
    out = []
    for smp in range(2):
        own = [tr.copy() for tr in track]
        for tr in own:
            site = np.flatnonzero(tr != ".")
            tr[site[rng.random(site.size) < 0.10]] = "."
            swap = site[rng.random(site.size) < 0.02]
            tr[swap] = letters[rng.integers(1, 4, swap.size)]
        rate = (0.25, 0.65)[smp]
        xms, starts, strands, rnames = [], [], [], []
        for _ in range(nrows[smp]):
            r, s = int(rng.integers(0, 2)), int(rng.integers(1, 3))
            ln = int(rng.integers(30, 301))
            st = int(rng.integers(1, glen - ln))
            row = own[r][st - 1:st - 1 + ln].copy()
            if s == 2:
                row = np.roll(row, 1)
            up = rng.random(ln) < np.where(row == "z", rate + 0.2 * rng.random(), rng.choice([0.0, 0.05, 0.15, 0.4]))
            row = np.where(up, np.char.upper(row), row)
            bad = rng.random(ln) < 0.04
            row[bad] = noise[rng.integers(0, noise.size, int(bad.sum()))]
            xms.append("".join(row)); starts.append(st); strands.append(s); rnames.append(r + 1)
        out.append(H.templates_from_xm(xms, starts, strands, rnames))
    return out


def test_symmetry(ea):
    ta, tb = fuzz_pair(0)
    bam_a, bam_b = as_bam(ea, ta), as_bam(ea, tb)
    for ctx, k in (("CG", 3), ("CX", 4)):
        ab, ba = gpu_compare(ea, bam_a, bam_b, ctx, k), gpu_compare(ea, bam_b, bam_a, ctx, k)
        assert ab.nrow > 0 and np.any(ab["jsd"] > 0) and np.any(ab["npatterns_a"] > 1) and ab.ncommon == ba.ncommon
        want = swapped(ba)
        tol = g_tol(ab)
        for q in INT_COLS:
            assert np.array_equal(ab[q], want[q]), q
        for q in FLOAT_COLS:
            assert np.all(np.abs(ab[q] - want[q]) <= (tol if q == "g" else ATOL)), q
        assert np.array_equal(ab.counts_a, ba.counts_b) and np.array_equal(ab.counts_b, ba.counts_a)


@pytest.mark.parametrize("k", [2, 4, 6])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_fuzz(ea, seed, k):
    ta, tb = fuzz_pair(seed)
    got, want = check(ea, ta, tb, "CG", k)
    assert 0 < want["ncommon"] < min(want["sites_a"]["pos"].size, want["sites_b"]["pos"].size)
    if k == 4:
        check(ea, ta, tb, "CxG" if seed & 1 else "CX", k, max_oo=0.3)


# ---- state and call sequences ------------------------------------------------------------------------------------------------

def _fetch_codes(ea, bam, others=True):
    """The return codes of every report's fetch on the batch, the comparison's last (others = False: of that one alone).
    A fetch that is refused writes nothing; the comparison's has room for 4096 rows."""
    import torch
    from epialleler_amd import _lib, api
    lib = _lib.load()
    ic = list(torch.empty((11, 4096), dtype=torch.int32, device="cuda").unbind(0))
    dc = list(torch.empty((13, 4096), dtype=torch.float64, device="cuda").unbind(0))
    ip, dp, b = api._ptr_array(ic), api._ptr_array(dc), bam.batch()
    if not others:
        return [lib.epi_batch_heterogeneity_compare_fetch_dev(b, ip, dp, None, None, None)]
    return [lib.epi_batch_cx_fetch_dev(b, ip, None), lib.epi_batch_mhl_fetch_dev(b, ip, dp, None),
            lib.epi_batch_heterogeneity_fetch_dev(b, ip, dp, None, None), lib.epi_batch_linkage_fetch_dev(b, ip, dp, None),
            lib.epi_batch_linkage_blocks_fetch_dev(b, ip, dp, None),
            lib.epi_batch_heterogeneity_compare_fetch_dev(b, ip, dp, None, None, None)]


def test_state(ea):
    from epialleler_amd import _lib
    lib = _lib.load()
    ta, tb = H.bam("amplicon000meth.bam"), H.bam("amplicon010meth.bam")
    bam_a, bam_b = as_bam(ea, ta), as_bam(ea, tb)
    nc, nr = C.c_int64(0), C.c_int64(0)
    run = lambda a, b, k=4, span=0, ctx=b"Zz": lib.epi_batch_heterogeneity_compare_dev(a, b, ctx, k, 0.1, 1, span, None, C.byref(nc), C.byref(nr))
    E, S, OK = _lib.EPI_ERR_ARG, _lib.EPI_ERR_STATE, _lib.EPI_OK
    assert run(bam_a.batch(), bam_b.batch()) == OK and (nc.value, 0 < nr.value <= 4096) == (128, True)
    assert _fetch_codes(ea, bam_a) == [S, S, S, S, S, OK]           # only the comparison's fetch may follow on a
    assert _fetch_codes(ea, bam_b) == [S, S, S, S, S, S]            # b holds no report
    # the comparison's fetch after any other report on a
    for other in (lambda: ea.generateCytosineReport(bam_a), lambda: ea.generateMhlReport(bam_a),
                  lambda: gpu_single(ea, bam_a, "CG", 4), lambda: ea.generateLinkageReport(bam_a)):
        assert run(bam_a.batch(), bam_b.batch()) == OK
        other()
        assert _fetch_codes(ea, bam_a, others=False) == [S]
    # arguments
    assert run(bam_a.batch(), bam_b.batch(), k=1) == E and run(bam_a.batch(), bam_b.batch(), k=7) == E
    assert run(bam_a.batch(), bam_b.batch(), span=-1) == E
    assert run(None, bam_b.batch()) == E and run(bam_a.batch(), None) == E and run(bam_a.batch(), bam_b.batch(), ctx=None) == E
    assert lib.epi_batch_heterogeneity_compare_dev(bam_a.batch(), bam_b.batch(), b"Zz", 4, 0.1, 1, 0, None, None, C.byref(nr)) == E
    assert lib.epi_batch_heterogeneity_compare_dev(bam_a.batch(), bam_b.batch(), b"Zz", 4, 0.1, 1, 0, None, C.byref(nc), None) == E
    assert run(bam_a.batch(), bam_b.batch()) == OK
    assert lib.epi_batch_heterogeneity_compare_fetch_dev(bam_a.batch(), None, None, None, None, None) == E


def test_report_on_b_between_report_and_fetch(ea):
    import torch
    from epialleler_amd import _lib, api
    lib = _lib.load()
    ta, tb = H.bam("amplicon000meth.bam"), H.bam("amplicon010meth.bam")
    bam_a, bam_b = as_bam(ea, ta), as_bam(ea, tb)
    want = gpu_compare(ea, bam_a, bam_b, "CG", 4)
    nc, nr = C.c_int64(0), C.c_int64(0)
    assert lib.epi_batch_heterogeneity_compare_dev(bam_a.batch(), bam_b.batch(), b"Zz", 4, 0.1, 1, 0, None, C.byref(nc), C.byref(nr)) == 0
    n = nr.value
    assert n == want.nrow > 0
    single_b = gpu_single(ea, bam_b, "CG", 6)                       # other windows, b's own table, b's own counters
    link_b = ea.generateLinkageReport(bam_b)
    ic = list(torch.empty((10, n), dtype=torch.int32, device="cuda").unbind(0))
    dc = list(torch.empty((13, n), dtype=torch.float64, device="cuda").unbind(0))
    cnt = [torch.empty((n, 16), dtype=torch.int32, device="cuda") for _ in range(2)]
    assert lib.epi_batch_heterogeneity_compare_fetch_dev(bam_a.batch(), api._ptr_array(ic), api._ptr_array(dc), C.c_void_p(cnt[0].data_ptr()),
                                                         C.c_void_p(cnt[1].data_ptr()), None) == 0
    for q, col in zip(INT_COLS + FLOAT_COLS, ic + dc):
        assert np.array_equal(col.cpu().numpy(), want[q]), q
    assert np.array_equal(cnt[0].cpu().numpy(), want.counts_a) and np.array_equal(cnt[1].cpu().numpy(), want.counts_b)
    # either histogram may be left out
    assert lib.epi_batch_heterogeneity_compare_fetch_dev(bam_a.batch(), api._ptr_array(ic), api._ptr_array(dc), None, None, None) == 0
    assert np.array_equal(dc[12].cpu().numpy(), want["g"])
    fresh = as_bam(ea, tb)
    assert np.array_equal(single_b["entropy"], gpu_single(ea, fresh, "CG", 6)["entropy"])
    H.assert_reports_equal(link_b, ea.generateLinkageReport(fresh), float_cols=("cov", "r2", "dprime"))


def test_later_reports_are_those_of_fresh_batches(ea):
    ta, tb = H.bam("amplicon000meth.bam"), H.bam("amplicon010meth.bam")
    bam_a, bam_b = as_bam(ea, ta), as_bam(ea, tb)
    first = gpu_compare(ea, bam_a, bam_b, "CG", 4)
    for used, t in ((bam_a, ta), (bam_b, tb)):
        fresh = as_bam(ea, t)
        for _ in range(2):                                          # (the second un-thresholded report runs in direct mode)
            H.assert_reports_equal(ea.generateCytosineReport(used, threshold_reads=False), ea.generateCytosineReport(fresh, threshold_reads=False))
        H.assert_reports_equal(ea.generateCytosineReport(used), ea.generateCytosineReport(fresh))
        H.assert_reports_equal(ea.generateMhlReport(used), ea.generateMhlReport(fresh), float_cols=("length", "lmhl"))
        H.assert_reports_equal(ea.generateHeterogeneityReport(used), ea.generateHeterogeneityReport(fresh),
                               float_cols=("beta", "epipolymorphism", "entropy", "pdr"))
        H.assert_reports_equal(ea.generateLinkageReport(used), ea.generateLinkageReport(fresh), float_cols=("cov", "r2", "dprime"))
        gpu_compare(ea, bam_a, bam_b, "CX", 2)                      # ... and a comparison between them
    again = gpu_compare(ea, bam_a, bam_b, "CG", 4)
    for q in INT_COLS + FLOAT_COLS:
        assert np.array_equal(first[q], again[q]), q


# ---- the interface ---------------------------------------------------------------------------------------------------------

def test_file_output_and_device_columns(ea, tmp_path):
    ta, tb = H.bam("amplicon000meth.bam"), H.bam("amplicon010meth.bam")
    assert ta["levels"] == tb["levels"]
    bam_a, bam_b = as_bam(ea, ta, ta["levels"]), as_bam(ea, tb, tb["levels"])
    want = fixture_want("amplicon000meth", "amplicon010meth", "CG", 4)
    rep = ea.compareHeterogeneity(bam_a, bam_b, window_context="CG", window_sites=4)
    assert list(rep.keys()) == list(INT_COLS + FLOAT_COLS) and rep.ncommon == 128 and not hasattr(rep, "counts_a")
    assert rep.levels["rname"] == tuple(ta["levels"])
    for q in INT_COLS:
        assert np.array_equal(rep[q], want[q]), q
    p, q = tmp_path / "cmp.tsv", tmp_path / "ref.tsv"
    assert ea.compareHeterogeneity(bam_a, bam_b, report_file=str(p), window_context="CG", window_sites=4) is None
    ea.writeReport(rep, str(q))
    text = p.read_text()
    assert text == q.read_text()
    lines = text.split("\n")
    assert lines[0] == "\t".join(INT_COLS + FLOAT_COLS) and len(lines) == rep.nrow + 2
    assert lines[1].split("\t")[0] == ta["levels"][int(rep["rname"][0]) - 1] and lines[1].split("\t")[4] == "CG" and lines[1].split("\t")[1] in "+-"
    back = np.genfromtxt(str(p), delimiter="\t", skip_header=1, usecols=range(5, 23))
    for j, name in enumerate((INT_COLS + FLOAT_COLS)[5:]):
        assert np.allclose(back[:, j], rep[name], rtol=1e-14, atol=1e-15), name
    dev = ea.compareHeterogeneity(bam_a, bam_b, window_context="CG", window_sites=4, as_device=True)
    for name in INT_COLS + FLOAT_COLS:
        assert dev[name].is_cuda and np.array_equal(dev[name].cpu().numpy(), rep[name]), name
    devc = ea.rcpp_heterogeneity_compare(bam_a, bam_b, "Zz", 4, 0.1, as_device=True, with_counts=True)
    assert devc.counts_a.is_cuda and np.array_equal(devc.counts_b.cpu().numpy(), want["counts_b"])
    assert ea.compareHeterogeneity(bam_a, bam_a, window_sites=2).ncommon == want["sites_a"]["pos"].size
