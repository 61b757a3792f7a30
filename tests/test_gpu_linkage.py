"""generateLinkageReport and generateHaplotypeBlocks against a plain restatement of their definitions (include/epihip.h):
loops over rows and numpy.  The restatement's site table is the CPU restatement's cx_report with an all-ones pass vector,
its kept rows are helpers.mhl_keep_np; nothing in it reads the GPU's own cytosine report.  Integer columns compare exactly;
the float columns within 1e-12 absolute (the project's value for the heterogeneity metrics): cov, r2 and dprime are each
fewer than ten roundings of 2^-53 away from the exact value and at most 1 in magnitude.  NaNs must sit at equal places."""
import ctypes as C
import functools
import gzip

import numpy as np
import pytest

import helpers as H
import test_gpu_heterogeneity as HT
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

INT_COLS = ("rname", "strand", "pos", "pos2", "context", "neighbour", "nreads", "n_uu", "n_mu", "n_um", "n_mm")
FLOAT_COLS = ("cov", "r2", "dprime")
BLOCK_INT_COLS = ("rname", "strand", "start", "end", "nsites")
BLOCK_FLOAT_COLS = ("mean_r2",)
ATOL = 1e-12


@pytest.fixture(scope="module")
def ea():
    import epialleler_amd
    return epialleler_amd


# ---- the restatement -------------------------------------------------------------------------------------------------

def metrics(counts):
    """cov, r2, dprime of [..., 4] integer bins n_uu, n_mu, n_um, n_mm."""
    c = counts.astype(np.int64)
    uu, mu, um, mm = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    n = uu + mu + um + mm
    A, a, B, b = mm + mu, um + uu, mm + um, mu + uu
    num = mm * uu - mu * um
    nf, numf = n.astype(np.float64), num.astype(np.float64)
    ok = (A > 0) & (a > 0) & (B > 0) & (b > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        cov = numf / (nf * nf)
        den = ((A.astype(np.float64) * a.astype(np.float64)) * B.astype(np.float64)) * b.astype(np.float64)
        r2 = np.where(ok, (numf * numf) / den, np.nan)
        lim = np.where(num > 0, np.minimum(A * b, a * B), np.minimum(A * B, a * b)).astype(np.float64)
        dprime = np.where(ok, np.where(num == 0, 0.0, numf / lim), np.nan)
    return cov, r2, dprime


def restate(t, ctx, D, max_oo=0.1, min_reads=1, max_distance=0):
    """The pair table of the templates t for the named context: dict of the fourteen columns, plus `sites` (the site
    table) and `grid`: per CX row and d the counts, pos2, whether the pair exists and whether it is reported."""
    c = H.CONTEXT_TO_BASES[ctx]
    n = t["off"].size - 1
    xm = np.asarray(t["xm"], np.uint8)
    cx = orc.cx_report(xm, t["off"], t["rname"], t["strand"], t["start"], np.ones(max(n, 1), np.int32)[:n], c["ctx_meth"])
    keep = H.mhl_keep_np(xm, t["off"], c["ctx_meth"] + c["ctx_unmeth"], 0, max_oo) if n else np.zeros(0, bool)
    N = cx["pos"].size
    counts = np.zeros((N, D, 4), np.int64)               # by CX row of the pair's first site, then d - 1
    pos2 = np.zeros((N, D), np.int64)
    is_pair = np.zeros((N, D), bool)
    strands = []                                          # the CX rows of every (rname, strand), in site order
    for r in np.unique(cx["rname"]):
        for s in (1, 2):
            rows = np.flatnonzero((cx["rname"] == r) & (cx["strand"] == s))
            if rows.size == 0:
                continue
            strands.append(rows)
            P = cx["pos"][rows].astype(np.int64)
            assert np.all(np.diff(P) > 0)
            code = cx["context"][rows]
            m = rows.size
            for d in range(1, min(D, m - 1) + 1):
                is_pair[rows[:m - d], d - 1] = True
                pos2[rows[:m - d], d - 1] = P[d:]
            for x in np.flatnonzero((t["rname"] == r) & (t["strand"] == s) & keep):
                st, o0, o1 = int(t["start"][x]), int(t["off"][x]), int(t["off"][x + 1])
                a, b = np.searchsorted(P, st), np.searchsorted(P, st + (o1 - o0))
                if b - a < 2:
                    continue
                nib = xm[o0 + (P[a:b] - st)] & 15
                valid = (nib & 7) == code[a:b]
                meth = (valid & (nib < 8)).astype(np.int64)
                for d in range(1, min(D, b - a - 1) + 1):
                    j = np.flatnonzero(valid[:-d] & valid[d:])
                    np.add.at(counts, (rows[a + j], d - 1, meth[j] + 2 * meth[j + d]), 1)
    assert not counts[~is_pair].any()
    nreads = counts.sum(axis=2)
    dist = pos2 - cx["pos"].astype(np.int64)[:, None]
    rep = is_pair & (nreads >= max(min_reads, 1)) & ((dist <= max_distance) if max_distance else True)
    i, dd = np.nonzero(rep)                               # C order: CX row, then d
    cn = counts[i, dd]
    cov, r2, dprime = metrics(cn) if cn.size else (np.zeros(0),) * 3
    i32 = lambda v: np.asarray(v).astype(np.int32)
    out = {"rname": cx["rname"][i], "strand": cx["strand"][i], "pos": cx["pos"][i], "pos2": i32(pos2[i, dd]), "context": cx["context"][i],
           "neighbour": i32(dd + 1), "nreads": i32(nreads[i, dd]), "n_uu": i32(cn[:, 0]), "n_mu": i32(cn[:, 1]), "n_um": i32(cn[:, 2]),
           "n_mm": i32(cn[:, 3]), "cov": cov, "r2": r2, "dprime": dprime,
           "sites": {q: cx[q] for q in ("rname", "strand", "pos", "context")},
           "grid": {"counts": counts, "rep": rep, "strands": strands, "D": D}}
    return out


def restate_blocks(want, min_r2, min_sites):
    """The blocks of a restated pair table: dict of the six columns."""
    g, sites = want["grid"], want["sites"]
    D = g["D"]
    with np.errstate(invalid="ignore"):
        r2 = metrics(g["counts"])[1]
        linked = g["rep"] & (r2 >= min_r2)                # [CX row of the first site, d - 1]; NaN compares false
    found = []
    for rows in g["strands"]:
        m = rows.size
        back = np.zeros(m, np.int64)
        for e in range(m):
            while back[e] < min(D, e) and linked[rows[e - back[e] - 1], back[e]]:
                back[e] += 1
        s = 0
        while s < m:
            e = s
            while e + 1 < m and back[e + 1] >= min(D, e + 1 - s):
                e += 1
            if e - s + 1 >= min_sites:
                total = 0.0
                for j in range(s, e):
                    total += float(r2[rows[j], 0])
                found.append((int(rows[s]), int(sites["pos"][rows[e]]), e - s + 1, total / (e - s)))
            s = e + 1
    found.sort()
    first = np.asarray([f[0] for f in found], np.int64)
    return {"rname": sites["rname"][first], "strand": sites["strand"][first], "start": sites["pos"][first],
            "end": np.asarray([f[1] for f in found], np.int32), "nsites": np.asarray([f[2] for f in found], np.int32),
            "mean_r2": np.asarray([f[3] for f in found], np.float64)}


def letters(ctx):
    c = H.CONTEXT_TO_BASES[ctx]
    return c["ctx_meth"] + c["ctx_unmeth"]


def gpu_report(ea, bam, ctx, D, max_oo=0.1, min_reads=1, max_distance=0):
    return ea.rcpp_linkage_report(bam, letters(ctx), D, max_distance, max_oo, min_reads)


def gpu_blocks(ea, bam, ctx, D, min_r2, min_sites, max_oo=0.1, min_reads=1, max_distance=0):
    return ea.rcpp_linkage_blocks(bam, letters(ctx), D, max_distance, max_oo, min_reads, min_r2, min_sites)


def assert_table(got, want, int_cols, float_cols, what=""):
    assert list(got.keys()) == list(int_cols + float_cols)
    for q in int_cols:
        assert got[q].dtype == np.int32 and np.array_equal(got[q], want[q]), (what, q)
    for q in float_cols:
        assert got[q].dtype == np.float64 and got[q].shape == want[q].shape, (what, q)
        assert np.array_equal(np.isnan(got[q]), np.isnan(want[q])), (what, q, "NaN places")
        ok = ~np.isnan(want[q])
        err = float(np.max(np.abs(got[q][ok] - want[q][ok]))) if ok.any() else 0.0
        print(what, q, "max abs error", err)
        assert err <= ATOL, (what, q, err)


def assert_same(got, want, what=""):
    assert_table(got, want, INT_COLS, FLOAT_COLS, what)


def exercises(want, D, r2_defined=True):
    """(two empty tables would compare equal)"""
    assert want["pos"].size > 0, "the case exercises nothing"
    assert D == 1 or np.any(want["neighbour"] > 1), "no pair beyond the adjacent ones"
    assert not r2_defined or np.any(~np.isnan(want["r2"])), "no defined r2"


def check(ea, t, ctx, D, r2_defined=True, **kw):
    want = restate(t, ctx, D, **kw)
    exercises(want, D, r2_defined)
    got = gpu_report(ea, HT.as_bam(ea, t), ctx, D, **kw)
    assert_same(got, want, (ctx, D, kw))
    return got, want


def check_blocks(ea, t, ctx, D, min_r2, min_sites, nonempty=True, **kw):
    pairs = restate(t, ctx, D, **kw)
    want = restate_blocks(pairs, min_r2, min_sites)
    if nonempty:
        exercises(pairs, D)
        assert want["start"].size > 0, "the case has no block"
    got = gpu_blocks(ea, HT.as_bam(ea, t), ctx, D, min_r2, min_sites, **kw)
    assert_table(got, want, BLOCK_INT_COLS, BLOCK_FLOAT_COLS, (ctx, D, min_r2, min_sites, kw))
    return got, want


# ---- the reference's fixtures ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def fixture_want(name, ctx, D, min_reads=1):
    return restate(H.bam(name), ctx, D, min_reads=min_reads)


# reported pairs and pairs with a defined r2, as the restatement gives them on the CPU: (D = 1, 4, 16)
FIXTURE_PAIRS = {"capture.bam": ((13622, 125), (45905, 323), (104495, 494)),
                 "amplicon010meth.bam": ((406, 63), (1305, 228), (2596, 525))}
# blocks for D = 4, min_r2 = 0.5, min_sites = 3: (min_reads = 1, min_reads = 10)
FIXTURE_BLOCKS = {"capture.bam": (16, None), "amplicon010meth.bam": (6, 4)}


@pytest.mark.parametrize("D", [1, 4, 16])
@pytest.mark.parametrize("name", ["capture.bam", "amplicon010meth.bam"])
def test_fixtures_cg(ea, name, D):
    t = H.bam(name)
    want = fixture_want(name, "CG", D)
    exercises(want, D)
    assert (want["pos"].size, int(np.count_nonzero(~np.isnan(want["r2"])))) == FIXTURE_PAIRS[name][(1, 4, 16).index(D)]
    assert_same(gpu_report(ea, HT.as_bam(ea, t), "CG", D), want, (name, D))


def test_fixture_three_contexts(ea):
    t = H.bam("capture.bam")
    want = fixture_want("capture.bam", "CX", 3)
    exercises(want, 3)
    assert set(np.unique(want["sites"]["context"])) == {2, 6, 7}
    assert_same(gpu_report(ea, HT.as_bam(ea, t), "CX", 3), want)


@pytest.mark.parametrize("name", ["capture.bam", "amplicon010meth.bam"])
def test_fixture_blocks(ea, name):
    t = H.bam(name)
    for min_reads, count in zip((1, 10), FIXTURE_BLOCKS[name]):
        if count is None:
            continue
        pairs = fixture_want(name, "CG", 4, min_reads)
        exercises(pairs, 4)
        want = restate_blocks(pairs, 0.5, 3)
        assert want["start"].size == count
        got = gpu_blocks(ea, HT.as_bam(ea, t), "CG", 4, 0.5, 3, min_reads=min_reads)
        assert_table(got, want, BLOCK_INT_COLS, BLOCK_FLOAT_COLS, (name, min_reads))
        assert np.all(got["nsites"] >= 3) and np.all(got["end"] > got["start"]) and np.all(got["mean_r2"] >= 0.5)


# ---- D = 1 against the heterogeneity report of windows of two sites ---------------------------------------------------------

def fuzz_batch(seed, nrows=3000):
    """3000 rows of 30 to 400 bytes on two sequences, contexts fixed per position, 5 % of the bytes replaced
    (test_gpu_heterogeneity.test_fuzz's batch)."""
    rng = np.random.default_rng(900 + seed)
    glen = 6000
    alphabet = np.asarray(list(".zxh"))
    track = [alphabet[rng.choice(4, glen, p=[0.7, 0.15, 0.08, 0.07])] for _ in range(2)]
    noise = np.asarray(list(".-zZxXhHuU"))
    xms, starts, strands, rnames = [], [], [], []
    for _ in range(nrows):
        r, s = int(rng.integers(0, 2)), int(rng.integers(1, 3))
        ln = int(rng.integers(30, 401))
        st = int(rng.integers(1, glen - ln))
        row = track[r][st - 1:st - 1 + ln].copy()
        if s == 2:                                       # the '-' strand has its own sites: the track shifted by one
            row = np.roll(row, 1)
        up = rng.random(ln) < np.where(row == "z", 0.2 + 0.6 * rng.random(), rng.choice([0.0, 0.05, 0.15, 0.4]))
        row = np.where(up, np.char.upper(row), row)
        bad = rng.random(ln) < 0.05
        row[bad] = noise[rng.integers(0, noise.size, int(bad.sum()))]
        xms.append("".join(row))
        starts.append(st)
        strands.append(s)
        rnames.append(r + 1)
    return H.templates_from_xm(xms, starts, strands, rnames)


@pytest.mark.parametrize("which", ["capture.bam", "fuzz"])
def test_one_neighbour_is_the_window_of_two(ea, which):
    t = H.bam(which) if which != "fuzz" else fuzz_batch(7)
    bam = HT.as_bam(ea, t)
    link = gpu_report(ea, bam, "CG", 1)
    het = ea.rcpp_heterogeneity_report(bam, "Zz", 2, 0.1, with_counts=True)
    assert link.nrow == het.nrow > 0 and np.any(het["npatterns"] > 1)
    if which == "capture.bam":
        assert link.nrow == HT.FIXTURE_WINDOWS[which][0]
    for a, b in (("rname", "rname"), ("strand", "strand"), ("pos", "pos"), ("pos2", "end"), ("context", "context"), ("nreads", "nreads")):
        assert np.array_equal(link[a], het[b]), a
    assert np.array_equal(np.stack([link[q] for q in ("n_uu", "n_mu", "n_um", "n_mm")], axis=1), het.counts)
    assert np.all(link["neighbour"] == 1)


# ---- hand-made batches ----------------------------------------------------------------------------------------------------

def calls_row(rng, nsites, step, every=1, p_meth=0.5):
    """A row over nsites sites `step` positions apart, with a CG call at every `every`-th of them ('.' elsewhere)."""
    out = []
    for i in range(nsites):
        ch = ("Z" if rng.random() < p_meth else "z") if i % every == 0 else "."
        out.append(ch + "." * (step - 1))
    return "".join(out)


def round_batch(seed, step, nsites_row):
    """A strand of at least 130 sites `step` positions apart.  Three rows in four call every site, one in four every other
    one (so every site keeps its majority); rows start at the site ordinals 0, 15, 16, 17 and at others drawn at random,
    every row holds nsites_row sites: more than three rounds of 16 sites, pairs that straddle one and (by the carried
    bits) none that reaches over two."""
    rng = np.random.default_rng(seed)
    first = [0, 15, 16, 17] * 3 + [int(v) for v in rng.integers(0, 140 - nsites_row // 2, 28)]
    xms, starts = [], []
    for i, o in enumerate(first):
        for rep in range(4):
            # half of the rows are concordant (all of one state), so that r2 is far from 0 somewhere
            p = (0.0 if rng.random() < 0.5 else 1.0) if rep < 2 else 0.5
            xms.append(calls_row(rng, nsites_row, step, 2 if rep == 3 else 1, p))
            starts.append(1 + step * o)
    return H.templates_from_xm(xms, starts, [1] * len(xms))


@pytest.mark.parametrize("D", [1, 5, 16])
def test_round_boundaries(ea, D):
    t = round_batch(21, 2, 70)
    assert np.mean(np.diff(t["off"])) < 512
    got, want = check(ea, t, "CG", D)
    sites = want["sites"]["pos"]
    assert sites.size >= 130 and np.array_equal(sites, 1 + 2 * np.arange(sites.size))
    if D == 16:
        # the row that starts at ordinal o pairs its 16th site (the last of its first round) with its 17th to 32nd, and its
        # first with its 17th: every such pair is there, with at least the rows that start at o
        for o in (0, 15, 16, 17):
            for j, d in ((o + 15, 1), (o + 15, 16), (o, 16), (o + 31, 1), (o + 31, 16), (o + 47, 16)):
                sel = (want["pos"] == 1 + 2 * j) & (want["neighbour"] == d)
                assert np.count_nonzero(sel) == 1 and want["nreads"][sel][0] >= 3, (o, j, d)


@pytest.mark.parametrize("D", [3, 16])
def test_round_boundaries_long_rows(ea, D):
    """The same with rows of 1500 bytes (sites ten positions apart): a whole wave takes a row, 64 sites a round."""
    t = round_batch(22, 10, 150)
    assert np.mean(np.diff(t["off"])) > 512
    got, want = check(ea, t, "CG", D)
    assert want["sites"]["pos"].size >= 130
    if D == 16:
        for o in (0, 15, 16, 17):
            for j, d in ((o + 63, 1), (o + 63, 16), (o + 48, 16), (o + 127, 16)):
                sel = (want["pos"] == 1 + 10 * j) & (want["neighbour"] == d)
                assert np.count_nonzero(sel) == 1 and want["nreads"][sel][0] >= 3, (o, j, d)


def test_one_long_row_among_short_ones(ea):
    rng = np.random.default_rng(23)
    long_row = "".join(rng.choice(list("Zz....."), 10000, p=[0.1, 0.05, 0.17, 0.17, 0.17, 0.17, 0.17]))
    xms, starts = [long_row], [1]
    for _ in range(200):
        s = int(rng.integers(1, 9900))
        ln = int(rng.integers(40, 120))
        xms.append("".join((("Z" if rng.random() < 0.5 else "z") if ch in "Zz" else ".") for ch in long_row[s - 1:s - 1 + ln]))
        starts.append(s)
    t = H.templates_from_xm(xms, starts, [1] * 201)
    check(ea, t, "CG", 6)


def test_gaps(ea):
    xms = ["Z.z.Z.z.Z.z",       # six sites at 1, 3, ..., 11
           "Z.z.Z.z.Z.z",
           "z.Z.z.Z.z.Z",
           "Z.-.Z.z.Z.z",       # '-' on the second site
           "Z.z...z.Z.z",       # '.' on the third
           "Z.z.h.z.Z.z",       # another context where the majority is z
           "Z.zzZ.z.Z.z",       # a z at position 4, where most rows have '.': not a site
           "z.Z.z",             # starts at position 5
           "Z.z.Z.z",
           "Z"]
    starts = [1, 1, 1, 1, 1, 1, 1, 5, 1, 11]
    t = H.templates_from_xm(xms, starts, [1] * len(xms))
    for D in (1, 3, 16):
        got, want = check(ea, t, "CG", D, max_oo=1.0)
        assert np.array_equal(want["sites"]["pos"], [1, 3, 5, 7, 9, 11])
    n = lambda p, q: int(want["nreads"][(want["pos"] == p) & (want["pos2"] == q)][0])
    # 1-5: the row with '-' at 3 counts (what lies between is no gap); those with '.' or h AT 5 do not
    assert n(1, 5) == 6 and n(1, 3) == 7 and n(3, 7) == 7 and n(5, 7) == 7 and n(1, 11) == 7


def test_strands_interleaved_and_sequence_ends(ea):
    """'+' sites at even, '-' sites at odd positions on two sequences; the last sites of sequence 1 and the first of
    sequence 2 are neighbours in each strand's site table: no pair joins them."""
    rng = np.random.default_rng(24)
    xms, starts, strands, rnames = [], [], [], []
    for r in (1, 2):
        for s in (1, 2):
            for _ in range(30):
                xms.append(HT.every_other(rng, int(rng.integers(3, 12))))
                starts.append(2 * int(rng.integers(1, 20)) + (s - 1))
                strands.append(s)
                rnames.append(r)
    t = H.templates_from_xm(xms, starts, strands, rnames)
    for D in (2, 16):
        got, want = check(ea, t, "CG", D)
        assert np.all(got["pos2"] > got["pos"]) and np.array_equal(got["pos"] % 2, (got["strand"] - 1) % 2)
        assert np.array_equal(got["pos2"] % 2, got["pos"] % 2)
        sites = want["sites"]
        for r in (1, 2):
            for s in (1, 2):
                m = np.count_nonzero((sites["rname"] == r) & (sites["strand"] == s))
                assert m >= 3
                for d in range(1, D + 1):
                    sel = (got["rname"] == r) & (got["strand"] == s) & (got["neighbour"] == d)
                    assert np.count_nonzero(sel) <= max(m - d, 0)


def test_short_strand_beside_a_long_one(ea):
    """two sites on '-', five on '+': '-' has its one adjacent pair and nothing for d >= 2"""
    t = H.templates_from_xm(["Z.z.Z.z.Z", "z.Z.z.Z.z", "Z.Z.z.z.Z", ".Z.z", ".z.Z"], [1, 1, 1, 1, 1], [1, 1, 1, 2, 2])
    got, want = check(ea, t, "CG", 4)
    minus = got["strand"] == 2
    assert got["pos"][minus].tolist() == [2] and got["pos2"][minus].tolist() == [4] and got["neighbour"][minus].tolist() == [1]
    assert np.count_nonzero(~minus) == 4 + 3 + 2 + 1


def test_row_filter(ea):
    """Out-of-context methylation just below, at and above max_outofcontext_beta; a row without out-of-context calls."""
    oo = HT.oo_row
    rows = [oo(0, 0), oo(1, 10), oo(2, 10), oo(0, 10), oo(3, 30), oo(4, 30), oo(2, 30),
            oo(1, 10, "z.Z.z.Z.z"), oo(2, 10, "z.Z.z.Z.z"), oo(10, 10, "z.z.z.z.z")]
    t = H.templates_from_xm(rows, [1] * len(rows), [1] * len(rows))
    keep = H.mhl_keep_np(t["xm"], t["off"], "Zz", 0, 0.1)
    assert keep.tolist() == [True, True, False, True, True, False, True, True, False, False]      # (0 / 0 is kept)
    got, want = check(ea, t, "CG", 2, max_oo=0.1)
    assert set(want["nreads"].tolist()) == {6}
    got1, want1 = check(ea, t, "CG", 2, max_oo=1.0)
    assert set(want1["nreads"].tolist()) == {10} and np.array_equal(got["pos"], got1["pos"])
    got0, want0 = check(ea, t, "CG", 2, max_oo=0.0, r2_defined=False)
    assert set(want0["nreads"].tolist()) == {2}


@pytest.mark.parametrize("D", [4, 16])
def test_contention(ea, D):
    """Thousands of identical rows on 25 sites: the rows of a wave hold the same counters (added once per set of lanes);
    a few rows that start one and two sites later sit in the same waves with other sites in their lanes."""
    a, b = "Z.z." * 12 + "Z", "z.Z." * 12 + "z"
    xms = [a] * 3000 + [b] * 2000 + [a[2:]] * 5 + [b[4:]] * 3
    starts = [100] * 5000 + [102] * 5 + [104] * 3
    t = H.templates_from_xm(xms, starts, [1] * len(xms))
    got, want = check(ea, t, "CG", D)
    assert want["sites"]["pos"].size == 25
    first = (got["pos"] == 100) & (got["neighbour"] == 1)
    assert got["n_mu"][first].tolist() == [3000] and got["n_um"][first].tolist() == [2000]
    assert int(got["nreads"].max()) == 5008


def test_min_reads_and_distance(ea):
    rng = np.random.default_rng(25)
    xms, starts = [], []
    track = "".join(rng.choice(list("C..."), 600))      # where the CpGs are: spacing varies, so distances do
    for _ in range(300):
        s = int(rng.integers(1, 500))
        xms.append("".join((("Z" if rng.random() < 0.5 else "z") if ch == "C" else ".") for ch in track[s - 1:s - 1 + int(rng.integers(30, 100))]))
        starts.append(s)
    t = H.templates_from_xm(xms, starts, [1] * 300)
    full, wfull = check(ea, t, "CG", 5)
    dist = full["pos2"] - full["pos"]
    cut = int(np.median(dist))
    sel = (full["nreads"] >= 3) & (dist <= cut)
    assert 0 < np.count_nonzero(sel) < sel.size and np.any(full["nreads"] < 3) and np.any(dist > cut) and np.any(dist == cut)
    got, want = check(ea, t, "CG", 5, min_reads=3, max_distance=cut)
    for q in INT_COLS + FLOAT_COLS:
        assert np.array_equal(got[q], full[q][sel], equal_nan=q in FLOAT_COLS), q
    got0 = gpu_report(ea, HT.as_bam(ea, t), "CG", 5, min_reads=0)       # below 1: as 1
    assert np.array_equal(got0["pos"], full["pos"]) and np.array_equal(got0["neighbour"], full["neighbour"])


def test_bad_arguments_at_the_c_level(ea):
    from epialleler_amd import _lib
    t = H.templates_from_xm(["Z.z.Z", "z.Z.z"], [1, 1], [1, 1])
    bam = HT.as_bam(ea, t)
    lib, nrow = _lib.load(), C.c_int64(0)
    for D, dist in ((0, 0), (17, 0), (2, -1)):
        assert lib.epi_batch_linkage_report_dev(bam.batch(), b"Zz", D, dist, 0.1, 1, None, C.byref(nrow)) == _lib.EPI_ERR_ARG
    assert lib.epi_batch_linkage_report_dev(bam.batch(), b"Zz", 2, 0, 0.1, 1, None, C.byref(nrow)) == _lib.EPI_OK and nrow.value == 3
    for r2, ms in ((-0.5, 2), (1.5, 2), (float("nan"), 2), (0.5, 1)):
        assert lib.epi_batch_linkage_blocks_dev(bam.batch(), r2, ms, None, C.byref(nrow)) == _lib.EPI_ERR_ARG
    # the counter cap is a function of the site count and D alone (test_linkage_host.test_counter_cap has its edges)
    out = C.c_int64(0)
    assert lib.epi_linkage_counter_bytes((4 << 30) // 256 + 1, 16, C.byref(out)) == _lib.EPI_ERR_ARG


@pytest.mark.parametrize("case", ["empty", "no_site", "one_site", "all_nan"])
def test_degenerate(ea, case):
    D = 4
    if case == "empty":
        t = H.templates_from_xm([], [], [])
    elif case == "no_site":
        t = H.templates_from_xm(["....", "..x..h"], [1, 3], [1, 2])
    elif case == "one_site":
        t = H.templates_from_xm(["..Z..", "..z.."], [1, 1], [1, 1])
    else:
        t = H.templates_from_xm(["Z.Z.Z.Z.Z.Z"] * 5 + ["Z.Z.Z"], [1] * 6, [1] * 6)     # fully methylated: every margin a = b = 0
    want = restate(t, "CG", D)
    got = gpu_report(ea, HT.as_bam(ea, t), "CG", D)
    assert_same(got, want, case)
    blocks = gpu_blocks(ea, HT.as_bam(ea, t), "CG", D, 0.0, 2)
    assert_table(blocks, restate_blocks(want, 0.0, 2), BLOCK_INT_COLS, BLOCK_FLOAT_COLS, case)
    assert blocks.nrow == 0
    if case == "all_nan":
        assert got.nrow == 5 + 4 + 3 + 2 and np.all(np.isnan(got["r2"])) and np.all(np.isnan(got["dprime"])) and np.all(got["cov"] == 0)
    else:
        assert got.nrow == 0


# ---- blocks ------------------------------------------------------------------------------------------------------------------

def concordant(nsites, reps=12):
    """rows that are methylated or unmethylated at all of nsites sites (every other position): r2 = 1 for every pair"""
    return ["Z." * (nsites - 1) + "Z"] * reps + ["z." * (nsites - 1) + "z"] * reps


def test_blocks_break_where_a_second_neighbour_is_not_linked(ea):
    """Six sites at 1, 3, ..., 11.  All adjacent pairs are linked; rows that call only the sites at 3 and 7, discordantly,
    take the pair (3, 7) to r2 = (144 - 25)^2 / 17^4 = 0.17: the site at 7 is linked to 5 but not to 3, the first block ends at 5 and the next
    starts at 7 and runs to the strand's end."""
    xms = concordant(6) + ["Z...z"] * 5 + ["z...Z"] * 5
    starts = [1] * 24 + [3] * 10
    t = H.templates_from_xm(xms, starts, [1] * len(xms))
    pairs = restate(t, "CG", 2)
    r2 = {(int(p), int(q)): v for p, q, v in zip(pairs["pos"], pairs["pos2"], pairs["r2"])}
    assert abs(r2[(3, 7)] - 119.0 ** 2 / 17.0 ** 4) < 1e-15 and all(v == 1.0 for k, v in r2.items() if k != (3, 7)) and len(r2) == 5 + 4
    got, want = check_blocks(ea, t, "CG", 2, 0.5, 3)
    assert got["start"].tolist() == [1, 7] and got["end"].tolist() == [5, 11] and got["nsites"].tolist() == [3, 3]
    assert got["mean_r2"].tolist() == [1.0, 1.0]
    # min_sites at its edge: three sites pass 3, not 4
    got4, _ = check_blocks(ea, t, "CG", 2, 0.5, 4, nonempty=False)
    assert got4.nrow == 0
    # with one neighbour only the pair (3, 7) is not looked at: one block of six
    got1, _ = check_blocks(ea, t, "CG", 1, 0.5, 6)
    assert got1["start"].tolist() == [1] and got1["end"].tolist() == [11] and got1["nsites"].tolist() == [6]


def test_blocks_nan_and_run_heads(ea):
    """Nine sites on '+': the fifth is methylated in every row (every pair with it has r2 = NaN: not linked, back = 0 at it
    and at its successor), so that the strand falls into the runs (1 .. 7), (9) and (11 .. 17); on '-' a discordant pair
    in the middle of six sites.  min_r2 = 1 keeps the exactly concordant pairs only."""
    plus = ["Z.Z.Z.Z.Z.Z.Z.Z.Z"] * 10 + ["z.z.z.z.Z.z.z.z.z"] * 10
    minus = ["Z.Z.Z.z.z.z"] * 6 + ["z.z.z.Z.Z.Z"] * 6 + ["Z.Z.Z.Z.Z.Z"] * 6 + ["z.z.z.z.z.z"] * 6
    t = H.templates_from_xm(plus + minus, [1] * 20 + [2] * 24, [1] * 20 + [2] * 24)
    got, want = check_blocks(ea, t, "CG", 3, 1.0, 2)
    assert got["strand"].tolist() == [1, 2, 2, 1] and got["start"].tolist() == [1, 2, 8, 11] and got["end"].tolist() == [7, 6, 12, 17]
    got3, _ = check_blocks(ea, t, "CG", 3, 1.0, 4)
    assert got3["strand"].tolist() == [1, 1] and got3["nsites"].tolist() == [4, 4]
    # a lower bar joins the two halves of '-' (r2 of its discordant pairs is 0 there: still two blocks at 0.01)
    got0, _ = check_blocks(ea, t, "CG", 3, 0.0, 2)
    assert got0["strand"].tolist() == [1, 2, 1] and got0["nsites"].tolist() == [4, 6, 4]


def test_blocks_do_not_touch_the_pair_table(ea):
    from epialleler_amd import _lib, api
    import torch
    t = H.bam("amplicon010meth.bam")
    bam = HT.as_bam(ea, t)
    want = fixture_want("amplicon010meth.bam", "CG", 4)
    lib, n = _lib.load(), C.c_int64(0)
    _lib.check(lib.epi_batch_linkage_report_dev(bam.batch(), b"Zz", 4, 0, 0.1, 1, None, C.byref(n)))
    assert n.value == want["pos"].size

    def fetch(fn, nrow, nint, nfloat):
        ic = list(torch.empty((nint, nrow), dtype=torch.int32, device="cuda").unbind(0))
        dc = list(torch.empty((nfloat, nrow), dtype=torch.float64, device="cuda").unbind(0))
        rc = fn(bam.batch(), api._ptr_array(ic), api._ptr_array(dc), None)
        torch.cuda.synchronize()
        return rc, [c.cpu().numpy() for c in ic + dc]

    assert fetch(lib.epi_batch_linkage_blocks_fetch_dev, 8, 5, 1)[0] == _lib.EPI_ERR_STATE          # no blocks_dev yet
    for min_r2, min_sites in ((0.5, 3), (0.9, 2), (0.5, 3)):
        nb = C.c_int64(0)
        _lib.check(lib.epi_batch_linkage_blocks_dev(bam.batch(), min_r2, min_sites, None, C.byref(nb)))
        wb = restate_blocks(want, min_r2, min_sites)
        assert nb.value == wb["start"].size > 0
        rc, cols = fetch(lib.epi_batch_linkage_blocks_fetch_dev, nb.value, 5, 1)
        assert rc == _lib.EPI_OK
        assert_table(dict(zip(BLOCK_INT_COLS + BLOCK_FLOAT_COLS, cols)), wb, BLOCK_INT_COLS, BLOCK_FLOAT_COLS, (min_r2, min_sites))
        rc, cols = fetch(lib.epi_batch_linkage_fetch_dev, n.value, 11, 3)
        assert rc == _lib.EPI_OK
        assert_same(dict(zip(INT_COLS + FLOAT_COLS, cols)), want, "pairs after blocks")


# ---- fuzz ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed,D", [(1, 2), (2, 5), (3, 16)])
def test_fuzz(ea, seed, D):
    t = fuzz_batch(seed)
    check(ea, t, "CG", D)
    check(ea, t, "CxG" if seed & 1 else "CX", D, max_oo=0.3)
    check_blocks(ea, t, "CG", D, 0.1, 2, min_reads=4)


# ---- call sequences ----------------------------------------------------------------------------------------------------------

def test_sequence_leaves_the_batch_fit(ea):
    import torch
    from epialleler_amd import _lib, api
    t = H.bam("capture.bam")
    bam = HT.as_bam(ea, t)
    lib = _lib.load()
    want = fixture_want("capture.bam", "CG", 4)
    cx0 = ea.generateCytosineReport(bam)                                  # pool, then direct on the repeats
    link = gpu_report(ea, bam, "CG", 4)
    assert_same(link, want)
    H.assert_reports_equal(cx0, ea.generateCytosineReport(bam))
    H.assert_reports_equal(cx0, ea.generateCytosineReport(bam))
    cxu0 = ea.generateCytosineReport(bam, threshold_reads=False, report_context="CX")
    gpu_report(ea, bam, "CHG", 2)
    H.assert_reports_equal(cxu0, ea.generateCytosineReport(bam, threshold_reads=False, report_context="CX"))
    het0 = ea.rcpp_heterogeneity_report(bam, "Zz", 3, 0.1, with_counts=True)
    m0 = ea.generateMhlReport(bam)
    assert_same(gpu_report(ea, bam, "CG", 4), want)
    het1 = ea.rcpp_heterogeneity_report(bam, "Zz", 3, 0.1, with_counts=True)
    for q in het0:
        assert np.array_equal(het0[q], het1[q]), q
    assert np.array_equal(het0.counts, het1.counts)
    blocks = gpu_blocks(ea, bam, "CG", 4, 0.5, 3)
    H.assert_reports_equal(m0, ea.generateMhlReport(bam), float_cols=("length", "lmhl"))
    assert_table(blocks, restate_blocks(want, 0.5, 3), BLOCK_INT_COLS, BLOCK_FLOAT_COLS)
    assert_same(gpu_report(ea, bam, "CG", 4), want)

    # fetches in the wrong order: a call sequence error
    ic = list(torch.empty((11, 8), dtype=torch.int32, device="cuda").unbind(0))
    dc = list(torch.empty((4, 8), dtype=torch.float64, device="cuda").unbind(0))
    b = bam.batch()
    assert lib.epi_batch_mhl_fetch_dev(b, api._ptr_array(ic[:5]), api._ptr_array(dc[:2]), None) == _lib.EPI_ERR_STATE
    assert lib.epi_batch_cx_fetch_dev(b, api._ptr_array(ic[:6]), None) == _lib.EPI_ERR_STATE
    assert lib.epi_batch_heterogeneity_fetch_dev(b, api._ptr_array(ic[:7]), api._ptr_array(dc), None, None) == _lib.EPI_ERR_STATE
    nrow = C.c_int64(0)
    for other in (lambda: ea.rcpp_heterogeneity_report(bam, "Zz", 2, 0.1), lambda: ea.generateMhlReport(bam),
                  lambda: ea.generateCytosineReport(bam, threshold_reads=False)):
        other()
        assert lib.epi_batch_linkage_fetch_dev(b, api._ptr_array(ic), api._ptr_array(dc[:3]), None) == _lib.EPI_ERR_STATE
        assert lib.epi_batch_linkage_blocks_dev(b, 0.5, 3, None, C.byref(nrow)) == _lib.EPI_ERR_STATE
        assert lib.epi_batch_linkage_blocks_fetch_dev(b, api._ptr_array(ic[:5]), api._ptr_array(dc[:1]), None) == _lib.EPI_ERR_STATE
    assert_same(gpu_report(ea, bam, "CG", 4), want)


def test_shared_tiles_are_refused(ea):
    import torch
    from epialleler_amd import _lib
    t = H.bam("amplicon010meth.bam")
    bam = HT.as_bam(ea, t)
    lib, b = _lib.load(), bam.batch()
    T = lib.epi_cx_tile_positions(b"Z")
    k0, k1 = C.c_int64(0), C.c_int64(-1)
    _lib.check(lib.epi_batch_tile_key_range_for(b, T, None, C.byref(k0), C.byref(k1)))
    keys, owned = np.asarray([k0.value], np.int64), np.asarray([1], np.int32)
    slab = torch.zeros(16 * T, dtype=torch.int32, device="cuda")
    _lib.check(lib.epi_batch_cx_set_shared(b, C.c_void_p(keys.ctypes.data), C.c_void_p(owned.ctypes.data), 1, C.c_void_p(slab.data_ptr())))
    try:
        with pytest.raises(ea.EpihipError) as ei:
            gpu_report(ea, bam, "CG", 4)
        assert ei.value.code == _lib.EPI_ERR_STATE and "sharded" in str(ei.value)
    finally:
        _lib.check(lib.epi_batch_cx_set_shared(b, None, None, 0, None))
    assert_same(gpu_report(ea, bam, "CG", 4), fixture_want("amplicon010meth.bam", "CG", 4))


# ---- files -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gz", [False, True])
def test_file_output(ea, tmp_path, gz):
    t = H.bam("amplicon010meth.bam")
    levels = t.get("levels") or ["chr%d" % i for i in range(1, 100)]
    bam = HT.as_bam(ea, t, levels)
    want = fixture_want("amplicon010meth.bam", "CG", 4)
    rep = ea.generateLinkageReport(bam, linkage_context="CG")
    assert_same(rep, want)
    read = lambda p: (gzip.open(p, "rt") if gz else open(p)).read()
    p = tmp_path / ("pairs.tsv.gz" if gz else "pairs.tsv")
    assert ea.generateLinkageReport(bam, report_file=str(p), linkage_context="CG", gzip=gz) is None
    lines = read(p).split("\n")
    assert lines[0] == "\t".join(INT_COLS + FLOAT_COLS) and len(lines) == rep.nrow + 2 and lines[-1] == ""
    cells = [ln.split("\t") for ln in lines[1:-1]]
    assert all(c[1] in "+-" and c[4] == "CG" for c in cells)
    for j, q in enumerate(INT_COLS):
        if q not in ("rname", "strand", "context"):
            assert [int(c[j]) for c in cells] == rep[q].tolist(), q
    r2 = np.asarray([float(c[12]) if c[12] else np.nan for c in cells])          # NaN is an empty field
    assert np.array_equal(np.isnan(r2), np.isnan(rep["r2"])) and np.isnan(r2).any() and np.allclose(r2, rep["r2"], atol=1e-12, equal_nan=True)

    blocks = ea.generateHaplotypeBlocks(bam, linkage_context="CG")                # min_reads = 10, min_r2 = 0.5, min_sites = 3
    wb = restate_blocks(fixture_want("amplicon010meth.bam", "CG", 4, 10), 0.5, 3)
    assert_table(blocks, wb, BLOCK_INT_COLS, BLOCK_FLOAT_COLS)
    assert blocks.nrow == FIXTURE_BLOCKS["amplicon010meth.bam"][1]
    q = tmp_path / ("blocks.tsv.gz" if gz else "blocks.tsv")
    assert ea.generateHaplotypeBlocks(bam, report_file=str(q), linkage_context="CG", gzip=gz) is None
    lines = read(q).split("\n")
    assert lines[0] == "\t".join(BLOCK_INT_COLS + BLOCK_FLOAT_COLS) and len(lines) == blocks.nrow + 2
    cells = [ln.split("\t") for ln in lines[1:-1]]
    assert [int(c[2]) for c in cells] == blocks["start"].tolist() and [int(c[3]) for c in cells] == blocks["end"].tolist()
    assert [int(c[4]) for c in cells] == blocks["nsites"].tolist() and all(c[1] in "+-" for c in cells)
    assert np.allclose([float(c[5]) for c in cells], blocks["mean_r2"], atol=1e-12)
    dev = ea.generateLinkageReport(bam, linkage_context="CG", as_device=True)
    assert dev["r2"].is_cuda and np.array_equal(dev["r2"].cpu().numpy(), rep["r2"], equal_nan=True)
