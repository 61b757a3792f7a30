"""generateFdrpReport where the pieces of its site -> rows index change behaviour (csrc/fdrp.hip): the number of table
sites N at the changeovers of the sort's pass count (the passes are the bytes that N - 1 occupies: none for N = 1, two from
257, three from 65537), the number of rows at the 4096-row blocks of k_fdrp_sum_calls and of the u32 scan, the number of
(site, row) pairs at the sort's 4096-key tile, a site whose run of equal keys spans several sorting tiles, and keys at the
ends of int32.  Every case compares all ten columns bit for bit (test_gpu_fdrp.assert_same) with the loop restatement of
the same templates: fdrp_np.restate, or, where a segment is too long for its scan of all rows per site,
fdrp_np.restate_indexed (test_fdrp_host.py shows the two equal).  The batches and the restatements need no GPU
(test_fdrp_host.py checks the builders' counts there, too).

The second half holds properties that do not come from the restatement -- both were written from the same header text --
and compare GPU results with GPU results."""
import functools

import numpy as np
import pytest

import fdrp_np
import helpers as H
import test_gpu_fdrp as TF

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ea():
    import epialleler_amd
    return epialleler_amd


TOP = 2 ** 31 - 1
SCAN_LIMIT = 4_000_000                                      # sites x rows above which restate's scan per site gives way to the index


def want_of(t, ctx="CG", **kw):
    names = {"W": "flank_sites", "m": "max_reads"}
    kw = {names.get(k, k): v for k, v in kw.items()}
    nsite = int(fdrp_np.site_table(t, ctx)["pos"].size)
    f = fdrp_np.restate if nsite * (t["off"].size - 1) <= SCAN_LIMIT else fdrp_np.restate_indexed
    return f(t, ctx, **kw)


def check(ea, t, want, **kw):
    got = TF.gpu_report(ea, TF.as_bam(ea, t), "CG", **kw)
    TF.assert_same(got, want, str(kw))
    assert got.nrow > 0, "two empty tables would compare equal"
    return got


def calls(rng, L):
    """L bytes, a CpG call at every one"""
    return "".join("Z" if x else "z" for x in rng.random(L) < 0.5)


def all_sites_coverage(want):
    s = want["sites"]
    return s["meth"].astype(np.int64) + s["unmeth"]


def ordinals(s):
    """the CX rows of a site table in the order of the per-strand table: '+' sites, then '-' sites, each by (rname, pos)"""
    return np.lexsort((s["pos"], s["rname"], s["strand"]))


# ---- table sizes -----------------------------------------------------------------------------------------------------------------

# (rname, strand) of the segments: '+' on sequences 4 to 8, '-' on sequences 1 to 4.  The table lists the '+' sites, then the
# '-' sites, each by (rname, pos): its first ordinal is the first '+' site of sequence 4, its last ordinal the last '-' site of
# sequence 4, and rows of ONE sequence hold both.
SEGMENTS = ((4, 1), (4, 2), (5, 1), (3, 2), (6, 1), (2, 2), (7, 1), (1, 2), (8, 1))


@functools.lru_cache(maxsize=None)
def table_batch(N, seed=71):
    """Exactly N CG sites over the first min(N, 9) of SEGMENTS, of random sizes.  A segment of n sites is the positions
    p0 .. p0 + n - 1; three gap-free backbones of rows of 40 to 130 sites (cut at the segment's end) tile it from p0 on, so
    that the site count is the span and every site is covered three times; a few more rows lie inside.
    The pairs of the index are written in batch order, and a stable sort that dropped its last pass would still leave
    the rows of ordinals 0 and N - 1 (equal in the lower key bytes for N = 257 and 65537) as two runs if every row of the
    one came in front of every row of the other.  So the '+' segment of sequence 4 starts 20 positions in front of the last
    site of its '-' segment, and two more '-' rows that end at that site start 10 positions in front of the first '+' rows
    and 5 behind them: in batch order the rows of the two ordinals interleave (table_want asserts it)."""
    rng = np.random.default_rng([seed, N])
    nseg = min(N, len(SEGMENTS))
    w = rng.random(nseg) + 0.25
    w[:2] += 2.0
    sizes = 1 + np.floor(w / w.sum() * (N - nseg)).astype(np.int64)
    sizes[int(np.argmax(w))] += N - int(sizes.sum())
    xms, starts, strs, rns = [], [], [], []

    def add(L, st, strand, rn):
        xms.append(calls(rng, L)); starts.append(st); strs.append(strand); rns.append(rn)
    for k, n in enumerate(sizes.tolist()):
        rn, strand = SEGMENTS[k]
        p0 = int(rng.integers(1000, 5000)) + (int(sizes[1]) if k == 0 and nseg > 1 else 0)
        if k == 1:                                          # the '-' segment of sequence 4 ends 20 positions into its '+' segment
            p0 = first_plus + 20 - (n - 1)
            if n > 40:
                add(31, first_plus - 10, 2, 4)
                add(16, first_plus + 5, 2, 4)
        first_plus = p0 if k == 0 else first_plus
        for _ in range(3):
            at = 0
            while at < n:
                L = min(int(rng.integers(40, 131)), n - at)
                add(L, p0 + at, strand, rn)
                at += L
        for _ in range(n // 150):
            L = min(int(rng.integers(40, 131)), n)
            add(L, p0 + int(rng.integers(0, n - L + 1)), strand, rn)
    t = H.templates_from_xm(xms, starts, strs, rns)
    assert t["start"].min() > 0
    return t


TABLE_CASES = [(N, 8, 40) for N in (1, 2, 256, 257, 65536, 65537)] + [(65537, 31, 64), (65537, 0, 2)]


def covering(t, rname, strand, pos):
    """the batch rows with a byte at pos (every byte of these batches is a call)"""
    return np.flatnonzero((t["rname"] == rname) & (t["strand"] == strand) & (t["start"] <= pos) & (pos < t["start"] + np.diff(t["off"])))


def table_want(N, W, m):
    t = table_batch(N)
    want = want_of(t, W=W, m=m)
    s = want["sites"]
    assert s["pos"].size == N
    assert all_sites_coverage(want).min() >= 2
    if N >= 16:
        assert np.unique(s["rname"]).size == 8 and set(s["strand"].tolist()) == {1, 2}
    # the first and the last ordinal of the table are reported: with N = 257 only ordinal 256 has a second key byte
    code = lambda q, i: (int(q["rname"][i]), int(q["strand"][i]), int(q["pos"][i]))
    order = ordinals(s)
    reported = {code(want, i) for i in range(want["pos"].size)}
    assert code(s, order[0]) in reported and code(s, order[-1]) in reported
    if N >= 256:                                            # their rows interleave in batch order (table_batch has the reason)
        first, last = covering(t, *code(s, order[0])), covering(t, *code(s, order[-1]))
        assert first.size >= 3 and last.min() < first.min() and first.max() < last.max()
    return t, want


@pytest.mark.parametrize("N,W,m", TABLE_CASES)
def test_table_sizes(ea, N, W, m):
    t, want = table_want(N, W, m)
    got = check(ea, t, want, W=W, m=m)
    assert got.nrow == N                                    # every site has two rows or more, and each pair shares the site


# ---- row counts ------------------------------------------------------------------------------------------------------------------

ROW_CASES = [(4095, False, 8, 40), (4096, False, 8, 40), (4097, False, 8, 40), (65537, False, 4, 6), (5, True, 8, 40), (4097, True, 8, 12)]


@functools.lru_cache(maxsize=None)
def rows_batch(n, wide, seed=73):
    """n rows in batch order over up to 8 sequences, strands drawn per row.  narrow: 4 to 12 bytes, a call at every byte;
    wide: 80 to 100 sites nine bytes apart (mean row above 512 bytes: a wave per row).  One row in 60 is dropped by the read
    rule (an HHHHHH tail) or of length 0, and so are the fourth and the third last row in front of every multiple of 4096
    and of the end of the batch (the tail of every block of 4096 rows holds both kinds) -- the last two rows of a block
    and of the batch are kept rows with calls, so that a block that is left out shows."""
    rng = np.random.default_rng([seed, n, int(wide)])
    step = 9 if wide else 1
    special = {int(x): int(x) % 2 for x in np.flatnonzero(rng.random(n) < 1 / 60)}          # row -> 0: dropped, 1: length 0
    edges = list(range(4096, n + 1, 4096)) + [n]
    tails = [e for e in edges if e % 4096 == 0 or n % 4096 >= 6 or n < 4096]      # (4097: the end's tail is the block's)
    for edge in edges:
        for x in range(max(edge - 6, 0), min(edge + 2, n)):
            special.pop(x, None)
    for edge in tails:
        special[edge - 4], special[edge - 3] = 0, 1
    xms, starts, strs, rns = [], [], [], []
    per_seq = max(-(-n // 8), 64)
    site = 0
    for x in range(n):
        if x % per_seq == 0:
            site = int(rng.integers(1, 100))
        site += int(rng.integers(0, 9 if wide else 3 if n < 10000 else 2))      # (65537 rows: fewer, deeper sites)
        ns = int(rng.integers(80, 101)) if wide else int(rng.integers(4, 13))
        xm = ("." * (step - 1)).join(calls(rng, ns))
        if x in special:
            xm = "" if special[x] else xm[:-6] + "HHHHHH"
        xms.append(xm); starts.append(1 + site * step); strs.append(int(rng.integers(1, 3)) if n > 64 else 1); rns.append(1 + x // per_seq)
    t = H.templates_from_xm(xms, starts, strs, rns)
    L = np.diff(t["off"])
    kept = H.mhl_keep_np(t["xm"], t["off"], "Zz", 0, 0.1) & (L > 0)
    assert t["start"].size == n
    assert all(kept[edge - 2] and kept[edge - 1] for edge in edges)
    assert all(L[edge - 4] > 0 and not kept[edge - 4] and L[edge - 3] == 0 for edge in tails)
    assert (int(t["off"][-1]) > 512 * n) == wide
    return t


def rows_want(n, wide, W, m):
    t = rows_batch(n, wide)
    want = want_of(t, W=W, m=m)
    assert want["pos"].size > 0
    assert any(n - 1 in u for u in want["used"]), "the last row of the batch is compared"
    return t, want


@pytest.mark.parametrize("n,wide,W,m", ROW_CASES)
def test_row_counts(ea, n, wide, W, m):
    t, want = rows_want(n, wide, W, m)
    check(ea, t, want, W=W, m=m)


# ---- pair counts -----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def pairs_batch(nc, seed=79):
    """Rows of 10 to 50 bytes without '.' or '-', all kept: the (site, row) pairs are the bytes.  The last row is cut so that
    there are exactly nc."""
    rng = np.random.default_rng([seed, nc])
    xms, starts, strs = [], [], []
    left, st = nc, 1
    while left:
        L = min(int(rng.integers(10, 51)), left)
        xms.append(calls(rng, L)); starts.append(st); strs.append(int(rng.integers(1, 3)))
        st += int(rng.integers(0, 6))
        left -= L
    return H.templates_from_xm(xms, starts, strs)


def pairs_want(nc):
    t = pairs_batch(nc)
    want = want_of(t, W=8, m=40)
    assert int(t["off"][-1]) == nc and int(all_sites_coverage(want).sum()) == nc
    return t, want


@pytest.mark.parametrize("nc", [4095, 4096, 4097, 8193])
def test_pair_counts(ea, nc):
    t, want = pairs_want(nc)
    check(ea, t, want, W=8, m=40)


# ---- deep sites ------------------------------------------------------------------------------------------------------------------

DEEP_POS = 500


@functools.lru_cache(maxsize=None)
def deep_batch(c, seed=83):
    """Position 500 of sequence 2, '+', is covered by exactly c kept rows with a call: 20 to 60 sites each (a call at every
    byte), ragged starts within 30 positions in front of it.  In batch order they are interleaved with rows of the other
    strand, rows without a call at the site, rows that end in front of it, rows the read rule drops and the rows of a
    second sequence, as test_gpu_fdrp.selection_batch does: the run of c equal keys spans the sort's 4096-key tiles and
    has to come out in ascending row index."""
    rng = np.random.default_rng([seed, c])
    xms, starts, strs, rns = [], [], [], []

    def add(xm, st, strand, rn=2):
        xms.append(xm); starts.append(st); strs.append(strand); rns.append(rn)

    def over(L, call=None):
        st = DEEP_POS - int(rng.integers(0, min(L, 30)))
        x = list(calls(rng, L))
        if call is not None:
            x[DEEP_POS - st] = call
        return "".join(x), st
    for _ in range(c):
        add(*over(int(rng.integers(20, 61))), 1)
    for _ in range(c // 8):
        add(*over(int(rng.integers(20, 61))), 2)                                # the other strand
    for _ in range(c // 40):
        add(*over(int(rng.integers(20, 61)), "."), 1)                           # no call at the site
        st = DEEP_POS - int(rng.integers(10, 30))
        add(calls(rng, DEEP_POS - st), st, 1)                                   # ends in front of it
        x, st = over(40)
        add(x[:-6] + "HHHHHH", st, 1)                                           # dropped by the read rule
    for _ in range(c // 8):
        add(calls(rng, int(rng.integers(20, 61))), DEEP_POS - int(rng.integers(0, 30)), int(rng.integers(1, 3)), 3)
    return H.templates_from_xm(xms, starts, strs, rns)


def deep_want(c, m):
    t = deep_batch(c)
    want = want_of(t, W=8, m=m)
    i = np.flatnonzero((want["rname"] == 2) & (want["strand"] == 1) & (want["pos"] == DEEP_POS))
    assert i.size == 1 and want["coverage"][i[0]] == c and want["nreads"][i[0]] == m
    used = want["used"][i[0]]
    assert used == sorted(used) and np.any(np.diff(used) > 1), "the covering rows are not a run of the batch"
    # two of the selected rows differ inside the window: another selection would not give the same numbers
    assert want["ndiscordant"][i[0]] > 0 and fdrp_np.selected_ranks(c, m) != list(range(m))
    return t, want, int(i[0])


@pytest.mark.parametrize("c", [4095, 4097, 9000])
@pytest.mark.parametrize("m", [2, 40, 64])
def test_deep_sites(ea, c, m):
    t, want, i = deep_want(c, m)
    got = check(ea, t, want, W=8, m=m)
    assert got["pos"][i] == DEEP_POS and got["coverage"][i] == c


# ---- keys at the ends of int32 ---------------------------------------------------------------------------------------------------

# The engine sets no limit on rname below int32 (epi_batch_upload takes any int32 column; the site table's key holds the
# rname in its upper 32 bits, site_table.hpp): the largest rname is 2^31 - 1.
MAX_RNAME = 2 ** 31 - 1


@functools.lru_cache(maxsize=None)
def end_batch(which):
    t = {k: v.copy() for k, v in table_batch(257).items()}
    if which == "pos":                                      # the last row ends at 2^31 - 1, as test_gpu_fuzz_reports.near_top
        end = int((t["start"].astype(np.int64) + np.diff(t["off"])).max())
        t["start"] = (t["start"].astype(np.int64) + (TOP - end)).astype(np.int32)
        assert int((t["start"].astype(np.int64) + np.diff(t["off"])).max()) == TOP and t["start"].min() > 0
    else:
        t["rname"] = (t["rname"].astype(np.int64) + (MAX_RNAME - int(t["rname"].max()))).astype(np.int32)
        assert int(t["rname"].max()) == MAX_RNAME and t["rname"].min() > 0 and np.all(np.diff(t["rname"]) >= 0)
    return t


def end_want(which, max_distance):
    t = end_batch(which)
    want = want_of(t, W=8, m=40, max_distance=max_distance)
    assert want["sites"]["pos"].size == 257 and want["pos"].size == 257
    assert (want["pos"].max() == TOP - 1) if which == "pos" else (want["rname"].max() == MAX_RNAME)
    return t, want


@pytest.mark.parametrize("max_distance", [0, 3])
@pytest.mark.parametrize("which", ["pos", "rname"])
def test_keys_at_the_ends_of_int32(ea, which, max_distance):
    t, want = end_want(which, max_distance)
    check(ea, t, want, W=8, m=40, max_distance=max_distance)
    if max_distance:
        assert not np.array_equal(want["qfdrp"], end_want(which, 0)[1]["qfdrp"])


# ---- properties that do not come from the restatement ------------------------------------------------------------------------------

def prop_batch(seed):
    rng = np.random.default_rng([89, seed])
    return TF.ragged(rng, 180, span=70, lmin=6, lmax=60, rnames=(1, 2, 3), p_site=0.9, p_gap=0.15, other="xhXH-", p_other=0.1)


def rows_of(rep, keep=None):
    keep = np.ones(rep["pos"].size, bool) if keep is None else keep
    return {q: np.asarray(rep[q])[keep] for q in fdrp_np.INT_COLS + fdrp_np.FLOAT_COLS}


def same_but(a, b, but=(), label=""):
    for q in fdrp_np.INT_COLS + fdrp_np.FLOAT_COLS:
        if q not in but:
            assert np.array_equal(a[q], b[q]), (label, q)


@pytest.mark.parametrize("W", [0, 4, 31])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_properties(ea, seed, W):
    t = prop_batch(seed)
    L = np.diff(t["off"])
    for min_overlap in (1, 2) if W else (1,):
        kw = dict(W=W, m=40, min_overlap=min_overlap)
        base = rows_of(TF.gpu_report(ea, TF.as_bam(ea, t), "CG", **kw))
        assert base["pos"].size > 50 and base["ndiscordant"].max() > 0 and set(base["strand"].tolist()) == {1, 2}

        # the scores' ranges, and the pairs of nreads rows
        assert np.all(0.0 <= base["qfdrp"]) and np.all(base["qfdrp"] <= base["fdrp"] + 1e-12) and np.all(base["fdrp"] <= 1.0)
        nr = base["nreads"].astype(np.int64)
        assert np.all(base["ndiscordant"] <= base["npairs"]) and np.all(base["nreads"] <= base["coverage"])
        if min_overlap == 1:
            assert np.array_equal(base["npairs"], nr * (nr - 1) // 2)
        else:
            assert np.all(base["npairs"] <= nr * (nr - 1) // 2) and np.any(base["npairs"] < nr * (nr - 1) // 2)

        # Z <-> z in every row
        swapped = dict(t, xm=np.where((t["xm"] & 7) == 7, t["xm"] ^ 8, t["xm"]).astype(np.uint8))
        assert np.count_nonzero(swapped["xm"] != t["xm"]) > 1000
        same_but(rows_of(TF.gpu_report(ea, TF.as_bam(ea, swapped), "CG", **kw)), base, label="Z <-> z")

        # a constant added to every start
        shifted = rows_of(TF.gpu_report(ea, TF.as_bam(ea, dict(t, start=t["start"] + 12345)), "CG", **kw))
        same_but(shifted, base, but=("pos",), label="shift")
        assert np.array_equal(shifted["pos"], base["pos"] + 12345)

        # every row on the other strand: the table's rows in the order of (rname, pos, strand) on both sides
        other = rows_of(TF.gpu_report(ea, TF.as_bam(ea, dict(t, strand=(3 - t["strand"]).astype(np.int32))), "CG", **kw))
        oa = np.lexsort((base["strand"], base["pos"], base["rname"]))
        ob = np.lexsort((3 - other["strand"], other["pos"], other["rname"]))
        same_but({q: v[ob] for q, v in other.items()}, {q: v[oa] for q, v in base.items()}, but=("strand",), label="strand")
        assert np.array_equal(3 - other["strand"][ob], base["strand"][oa])

        # rows of a further sequence behind the batch
        more = prop_batch(seed + 10)
        both = {"xm": np.concatenate((t["xm"], more["xm"])), "off": np.concatenate((t["off"], t["off"][-1] + more["off"][1:])),
                "rname": np.concatenate((t["rname"], more["rname"] + 3)), "strand": np.concatenate((t["strand"], more["strand"])),
                "start": np.concatenate((t["start"], more["start"]))}
        longer = TF.gpu_report(ea, TF.as_bam(ea, both), "CG", **kw)
        assert longer.nrow > base["pos"].size and L.size < both["start"].size
        same_but(rows_of(longer, np.asarray(longer["rname"]) <= 3), base, label="appended")
