"""Plain restatements (loops and numpy) of the cytosine report comparison and its regions as include/epihip.h defines them
(epi_cx_compare_dev, epi_cx_compare_regions_dev), the hand-written tables and the Fisher tables the tests of both share.
The p-values of the restatement are the host epi_fisher_exact's, which test_vcf_host.py pins against scipy (cells below
30 000) and test_cx_compare_host.py against exact_fisher, the same rule in exact fractions or 60-digit arithmetic (cells up
to 2^31 - 1); pooled cells of a region that pass int32 take exact_fisher's p.  Test infrastructure only; treat what the
functions return as read-only."""
import fractions
import functools

import numpy as np

CX = ("rname", "strand", "pos", "context", "meth", "unmeth")
CMP_INT = ("rname", "strand", "pos", "context", "meth_a", "unmeth_a", "meth_b", "unmeth_b")
CMP_FLOAT = ("beta_a", "beta_b", "delta_beta", "p")
DMR_INT = ("rname", "start", "end", "nsites", "direction")
DMR_FLOAT = ("beta_a", "beta_b", "delta_beta", "mean_delta_beta", "p")


def host_fisher(a, b, c, d):
    """The host epi_fisher_exact (one thread) over four integer array-likes."""
    import epialleler_amd as ea
    cells = {k: np.asarray(v, np.int64) for k, v in zip("abcd", (a, b, c, d))}
    for v in cells.values():
        assert v.size == 0 or (v.min() >= -2 ** 31 and v.max() < 2 ** 31)
    return ea.rcpp_fep({k: v.astype(np.int32) for k, v in cells.items()}, tuple("abcd"), nthreads=1)


def cx_table(rows):
    """rows of (rname, strand, pos, context, meth, unmeth) -> the six int32 columns"""
    m = np.asarray(rows, np.int64).reshape(-1, 6)
    return {k: np.ascontiguousarray(m[:, i]).astype(np.int32) for i, k in enumerate(CX)}


def is_sorted(t):
    key = list(zip(t["rname"].tolist(), t["pos"].tolist(), t["strand"].tolist()))
    return all(x < y for x, y in zip(key, key[1:]))


def join_np(a, b, min_coverage=1):
    """The comparison table of the CX tables a and b (dict of the twelve columns, `ncommon`)."""
    in_b = {(r, s, p): j for j, (r, s, p) in enumerate(zip(b["rname"].tolist(), b["strand"].tolist(), b["pos"].tolist()))}
    lo = max(int(min_coverage), 1)
    ncommon = 0
    rows = []
    for i, key in enumerate(zip(a["rname"].tolist(), a["strand"].tolist(), a["pos"].tolist())):
        j = in_b.get(key)
        if j is None or int(b["context"][j]) != int(a["context"][i]):
            continue
        ncommon += 1
        ma, ua, mb, ub = int(a["meth"][i]), int(a["unmeth"][i]), int(b["meth"][j]), int(b["unmeth"][j])
        if ma + ua >= lo and mb + ub >= lo:
            rows.append(key[:1] + (key[1], key[2], int(a["context"][i]), ma, ua, mb, ub))
    m = np.asarray(rows, np.int64).reshape(-1, 8)
    out = {k: m[:, i].astype(np.int32) for i, k in enumerate(CMP_INT)}
    with np.errstate(invalid="ignore", divide="ignore"):
        out["beta_a"] = m[:, 4].astype(np.float64) / (m[:, 4] + m[:, 5]).astype(np.float64)
        out["beta_b"] = m[:, 6].astype(np.float64) / (m[:, 6] + m[:, 7]).astype(np.float64)
    out["delta_beta"] = out["beta_b"] - out["beta_a"]
    out["p"] = host_fisher(m[:, 4], m[:, 5], m[:, 6], m[:, 7])
    out["ncommon"] = ncommon
    return out


def pack_key(t):
    """(rname, pos, strand) of a CX table as one uint64 that sorts as the triple does: 31 + 31 + 2 bits."""
    r, p, s = (np.asarray(t[k], np.int64) for k in ("rname", "pos", "strand"))
    assert r.size == 0 or (min(r.min(), p.min(), s.min()) >= 0 and s.max() < 4)
    return (r.astype(np.uint64) << np.uint64(33)) | (p.astype(np.uint64) << np.uint64(2)) | s.astype(np.uint64)


def join_vec(a, b, min_coverage=1):
    """join_np without the loop (np.searchsorted on pack_key), for tables of a million rows; both tables sorted.  Equal
    tables have equal p: the host Fisher test runs once per distinct table."""
    ka, kb = pack_key(a), pack_key(b)
    j = np.minimum(np.searchsorted(kb, ka), max(kb.size - 1, 0))
    if kb.size:
        common = (kb[j] == ka) & (np.asarray(b["context"])[j] == np.asarray(a["context"]))
    else:
        common = np.zeros(ka.size, bool)
    lo = max(int(min_coverage), 1)
    i = np.flatnonzero(common)
    j = j[i]
    cells = np.stack([np.asarray(t[k], np.int64)[x] for t, x in ((a, i), (b, j)) for k in ("meth", "unmeth")], 1).reshape(-1, 4)
    keep = (cells[:, 0] + cells[:, 1] >= lo) & (cells[:, 2] + cells[:, 3] >= lo)
    i, cells = i[keep], cells[keep]
    out = {k: np.asarray(a[k])[i].astype(np.int32) for k in CX[:4]}
    out.update({k: cells[:, c].astype(np.int32) for c, k in enumerate(CMP_INT[4:])})
    with np.errstate(invalid="ignore", divide="ignore"):
        out["beta_a"] = cells[:, 0].astype(np.float64) / (cells[:, 0] + cells[:, 1]).astype(np.float64)
        out["beta_b"] = cells[:, 2].astype(np.float64) / (cells[:, 2] + cells[:, 3]).astype(np.float64)
    out["delta_beta"] = out["beta_b"] - out["beta_a"]
    distinct, inverse = np.unique(cells, axis=0, return_inverse=True)
    out["p"] = host_fisher(*distinct.T)[inverse.reshape(-1)] if cells.size else np.zeros(0, np.float64)
    out["ncommon"] = int(common.sum())
    return out


def regions_np(t, max_p, min_delta_beta, max_gap, min_sites):
    """The regions of the comparison table t (dict of the ten columns, `cells`: the pooled tables); one sequential pass.
    p is the host epi_fisher_exact's where the pooled cells fit int32 and exact_fisher's, rounded to a double, elsewhere."""
    n = t["pos"].size
    delta, p = np.asarray(t["delta_beta"], np.float64), np.asarray(t["p"], np.float64)

    def direction(i):
        d = float(delta[i])
        if not (p[i] <= max_p) or not (abs(d) >= min_delta_beta) or d == 0.0 or d != d:
            return 0
        return 1 if d > 0 else -1

    runs = []
    i = 0
    while i < n:
        d = direction(i)
        if d == 0:
            i += 1
            continue
        j = i + 1
        while j < n and direction(j) == d and int(t["rname"][j]) == int(t["rname"][i]) and int(t["pos"][j]) - int(t["pos"][j - 1]) <= max_gap:
            j += 1
        if j - i >= min_sites:
            runs.append((i, j, d))
        i = j
    ints = np.zeros((len(runs), 5), np.int64)
    flt = np.zeros((len(runs), 5), np.float64)
    cells = np.zeros((len(runs), 4), np.int64)
    for r, (i, j, d) in enumerate(runs):
        ma, ua, mb, ub = (int(np.asarray(t[k][i:j], np.int64).sum()) for k in ("meth_a", "unmeth_a", "meth_b", "unmeth_b"))
        ints[r] = (t["rname"][i], t["pos"][i], t["pos"][j - 1], j - i, d)
        total = 0.0
        for v in delta[i:j].tolist():                     # ascending rows, one accumulator
            total += v
        beta_a, beta_b = np.float64(ma) / np.float64(ma + ua), np.float64(mb) / np.float64(mb + ub)
        flt[r, :4] = (beta_a, beta_b, beta_b - beta_a, np.float64(total) / np.float64(j - i))
        cells[r] = (ma, ua, mb, ub)
    wide = (cells >= 2 ** 31).any(axis=1)                  # a pooled cell beyond int32: the host entry point cannot take it
    flt[~wide, 4] = host_fisher(*cells[~wide].T) if np.any(~wide) else 0.0
    flt[wide, 4] = [float(exact_fisher(*row)) for row in cells[wide].tolist()]
    out = {k: ints[:, i].astype(np.int32) for i, k in enumerate(DMR_INT)}
    out.update({k: flt[:, i].copy() for i, k in enumerate(DMR_FLOAT)})
    out["cells"] = cells                                   # the pooled tables (not a column of the report)
    return out


# ---- the hand-written known answer ------------------------------------------------------------------------------------
# U: b far above a, D: b far below a, N: (3 1 / 1 3), not significant.  context 6 = CG, 5 = CHG.
KAT_A = cx_table([
    (1, 1, 10, 6, 0, 20), (1, 2, 11, 6, 2, 8), (1, 1, 50, 6, 1, 29),       # a run of three ...
    (1, 1, 300, 6, 0, 20), (1, 2, 301, 6, 0, 20),                          # ... broken by max_gap (250 > 100)
    (1, 1, 320, 6, 20, 0), (1, 2, 321, 6, 20, 0),                          # ... by a direction flip
    (1, 1, 330, 6, 0, 20), (1, 2, 331, 6, 0, 20),                          # ... and back
    (1, 1, 340, 6, 3, 1),                                                  # ... by an insignificant row
    (1, 1, 350, 6, 0, 20), (1, 2, 351, 6, 0, 20),
    (2, 1, 352, 6, 0, 20), (2, 2, 353, 6, 0, 20),                          # ... by an rname change (one base on)
    (2, 1, 400, 6, 0, 20),                                                 # b has CHG here: not common
    (2, 1, 500, 6, 0, 20),                                                 # a only
    (2, 1, 600, 6, 0, 20),                                                 # a run of one: below min_sites
    (2, 1, 700, 6, 1, 0),                                                  # common, covered once: below min_coverage
])
KAT_B = cx_table([
    (1, 1, 5, 6, 9, 9),                                                    # b only
    (1, 1, 10, 6, 20, 0), (1, 2, 11, 6, 9, 1), (1, 1, 50, 6, 25, 5),
    (1, 1, 300, 6, 20, 0), (1, 2, 301, 6, 20, 0),
    (1, 1, 320, 6, 0, 20), (1, 2, 321, 6, 0, 20),
    (1, 1, 330, 6, 20, 0), (1, 2, 331, 6, 20, 0),
    (1, 1, 340, 6, 1, 3),
    (1, 1, 350, 6, 20, 0), (1, 2, 351, 6, 20, 0),
    (2, 1, 352, 6, 20, 0), (2, 2, 353, 6, 20, 0),
    (2, 1, 400, 5, 20, 0),
    (2, 1, 600, 6, 20, 0),
    (2, 1, 700, 6, 0, 1),
])
KAT_ARGS = dict(min_coverage=2, max_p=0.05, min_delta_beta=0.1, max_gap=100, min_sites=2)
KAT_NCOMMON = 16
KAT_POS = [10, 11, 50, 300, 301, 320, 321, 330, 331, 340, 350, 351, 352, 353, 600]
KAT_REGIONS = [(1, 10, 50, 3, 1), (1, 300, 301, 2, 1), (1, 320, 321, 2, -1), (1, 330, 331, 2, 1), (1, 350, 351, 2, 1), (2, 352, 353, 2, 1)]
KAT_P_3113 = 0.4857142857142857          # fisher.test(matrix(c(3, 1, 1, 3), 2))


def check_kat(table, regions):
    """A comparison table and its regions (dicts of numpy columns) against the hand-written expectation."""
    assert table["pos"].tolist() == KAT_POS
    assert table["rname"].tolist() == [1] * 12 + [2] * 3 and table["strand"].tolist() == [1, 2, 1, 1, 2, 1, 2, 1, 2, 1, 1, 2, 1, 2, 1]
    assert table["meth_a"].tolist() == [0, 2, 1, 0, 0, 20, 20, 0, 0, 3, 0, 0, 0, 0, 0]
    assert table["unmeth_b"].tolist() == [0, 1, 5, 0, 0, 20, 20, 0, 0, 3, 0, 0, 0, 0, 0]
    assert table["beta_a"][1] == 0.2 and table["beta_b"][1] == 0.9 and table["delta_beta"][1] == 0.9 - 0.2
    assert abs(table["p"][9] / KAT_P_3113 - 1) < 1e-12
    assert [tuple(int(regions[k][r]) for k in DMR_INT) for r in range(regions["rname"].size)] == KAT_REGIONS
    assert regions["beta_a"][0] == 3 / 60 and regions["beta_b"][0] == 54 / 60 and regions["delta_beta"][0] == 54 / 60 - 3 / 60
    assert regions["mean_delta_beta"][0] == ((1.0 + (0.9 - 0.2)) + (25 / 30 - 1 / 30)) / 3
    assert regions["delta_beta"][2] == -1.0 and regions["mean_delta_beta"][2] == -1.0
    assert np.all(regions["p"] < 1e-6)


# ---- Fisher tables ------------------------------------------------------------------------------------------------------

def small_tables():
    """All 2401 tables with cells 0 .. 6: ties, degenerate margins, the mode as the observed table."""
    g = np.arange(7)
    return np.stack(np.meshgrid(g, g, g, g, indexing="ij"), -1).reshape(-1, 4).astype(np.int32)


# Larger tables.  stirlerr sees the margins, k and margin - k: the rows below put its argument into (0, 15], (15, 35],
# (35, 80], (80, 500] and above 500; a cell next to its expectation takes bd0 through its series, one far from it through
# the logarithm.
LARGE_TABLES = np.asarray([
    (8, 3, 2, 9), (12, 1, 3, 11), (7, 7, 6, 8),                               # everything at most 15
    (20, 10, 9, 22), (16, 17, 30, 5), (33, 2, 1, 34),                         # (15, 35]
    (50, 30, 28, 60), (40, 39, 70, 12), (79, 1, 36, 44),                      # (35, 80]
    (200, 100, 90, 250), (480, 20, 100, 300), (81, 300, 499, 90),             # (80, 500]
    (600, 700, 800, 500), (5000, 4000, 4100, 5100), (30000, 200, 29000, 900), # above 500
    (3, 14000, 25, 19000), (0, 700, 9, 650), (1, 2, 20000, 30000),            # skewed: small next to large
    (100, 100, 100, 100), (1000, 1000, 1000, 1001), (251, 250, 249, 250),     # at the expectation: bd0's series
    (37, 37, 37, 37), (15, 16, 16, 15), (500, 501, 501, 500),                 # mirrored tables: exact ties
    (2000, 0, 0, 2000), (0, 5000, 5000, 0), (900, 0, 1, 900),                 # p underflows to 0, or nearly
    (300, 10, 12, 310), (400, 2, 3, 380),                                     # tiny but normal
    (1000000, 1000000, 1000000, 1000000), (1000000, 999000, 998500, 1000000), # cells of 10^6
    (1000000, 3, 5, 1000000), (1000000, 1000, 1000500, 900), (1002000, 1000000, 1000000, 1003000),
    (2 ** 31 - 1, 3, 5, 4), (4, 6, 2, 2 ** 31 - 1),                           # a cell at 2^31 - 1
    (0, 0, 5, 9), (0, 4, 0, 8), (7, 0, 11, 0), (0, 0, 0, 0),                  # degenerate margins
], np.int64).astype(np.int32)
NEGATIVE_TABLES = np.asarray([(-1, 2, 3, 4), (1, -2 ** 31, 3, 4), (5, 5, -7, 5), (1, 2, 3, -1)], np.int64).astype(np.int32)


def degenerate(t):
    """One table only has these margins: the p-value is exactly 1."""
    t = np.asarray(t, np.int64)
    n1, n2, m = t[:, 0] + t[:, 1], t[:, 2] + t[:, 3], t[:, 0] + t[:, 2]
    return np.maximum(0, m - n2) == np.minimum(m, n1)


def _ratios_exact(n1, n2, m, lo, hi, a):
    """P(k) / P(a) of the hypergeometric distribution for k = lo .. hi as exact fractions (the ratio recurrence)."""
    out = {a: fractions.Fraction(1)}
    for x in range(a, hi):
        out[x + 1] = out[x] * fractions.Fraction((n1 - x) * (m - x), (x + 1) * (n2 - m + x + 1))
    for x in range(a, lo, -1):
        out[x - 1] = out[x] * fractions.Fraction(x * (n2 - m + x), (n1 - x + 1) * (m - x + 1))
    return out


def tie_band_distance(table, exact_below=400):
    """min over the tables k with these margins of |P(k) / P(a) - (1 + 1e-7)|: how far the nearest table is from
    changing sides when P is a few ulp off.  Exact fractions for a short range; else 60-digit log-gamma, at the tables
    around the two places where the ratio crosses the band (P is unimodal)."""
    import mpmath
    a, b, c, d = (int(v) for v in table)
    n1, n2, m = a + b, c + d, a + c
    lo, hi = max(0, m - n2), min(m, n1)
    band = fractions.Fraction(10 ** 7 + 1, 10 ** 7)
    if hi - lo <= exact_below:
        return float(min(abs(r - band) for r in _ratios_exact(n1, n2, m, lo, hi, a).values()))
    mp = mpmath.mp.clone()
    mp.dps = 60

    def logc(n, k):
        return mp.loggamma(n + 1) - mp.loggamma(k + 1) - mp.loggamma(n - k + 1)

    def ratio(k):
        return mp.exp(logc(n1, k) + logc(n2, m - k) - logc(n1, a) - logc(n2, m - a))

    mode = min(max((m + 1) * (n1 + 1) // (n1 + n2 + 2), lo), hi)
    mpband = mp.mpf(band.numerator) / band.denominator
    near = {a, lo, hi, mode}
    x0, x1 = lo, mode                                       # non-decreasing: the first k above the band
    while x0 < x1:
        k = (x0 + x1) // 2
        if ratio(k) > mpband:
            x1 = k
        else:
            x0 = k + 1
    near.update((x0 - 1, x0, x0 + 1))
    x0, x1 = mode, hi                                       # non-increasing: the last k above the band
    while x0 < x1:
        k = (x0 + x1 + 1) // 2
        if ratio(k) > mpband:
            x0 = k
        else:
            x1 = k - 1
    near.update((x0 - 1, x0, x0 + 1))
    return float(min(abs(ratio(k) - mpband) for k in near if lo <= k <= hi))


# Tables with cells near 2^31 on both sides: x / n of dbinom_raw is within 1e-9 of 1 there.  Kept out of LARGE_TABLES
# (the `fisher_cases` of the device-against-host tests stay as they are).
NEAR_INT32_TABLES = np.asarray([(2 ** 31 - 1, 3, 5, 4), (2 ** 31 - 1, 7, 2147483548, 19), (2000000000, 1000, 1999990000, 1300)], np.int64)


def exact_fisher(a, b, c, d, exact_below=400):
    """The two-sided Fisher p of (a b / c d) by the rule of csrc/fisher_math.hpp, sum of P(k) over P(k) <= P(a) (1 + 1e-7),
    as a 60-digit mpmath number; cells of any size.  A range hi - lo of at most exact_below: exact fractions throughout.
    Else P(a) from loggamma and the ratio recurrence outwards from a in both directions, past the mode, until a term is
    below 1e-45 of P(a) (what is left out is below 1e-45 of p per term, P being log-concave).  When even
    (hi - lo + 1) P(a) (1 + 1e-7), which bounds p from above, is below 1e-400 the result is 0: no double holds it, and
    walking from a to the mode could take 2^32 steps."""
    import mpmath
    mp = mpmath.mp.clone()
    mp.dps = 60
    a, b, c, d = int(a), int(b), int(c), int(d)
    assert min(a, b, c, d) >= 0
    n1, n2, m = a + b, c + d, a + c
    lo, hi = max(0, m - n2), min(m, n1)
    if lo == hi:
        return mp.mpf(1)
    band = fractions.Fraction(10 ** 7 + 1, 10 ** 7)
    if hi - lo <= exact_below:
        r = _ratios_exact(n1, n2, m, lo, hi, a)
        p = sum(v for v in r.values() if v <= band) / sum(r.values())
        return mp.mpf(p.numerator) / mp.mpf(p.denominator)

    def logc(n, k):
        return mp.loggamma(n + 1) - mp.loggamma(k + 1) - mp.loggamma(n - k + 1)

    log_pa = logc(n1, a) + logc(n2, m - a) - logc(n1 + n2, m)
    mpband = mp.mpf(band.numerator) / band.denominator
    if log_pa + mp.log((hi - lo + 1) * mpband) < mp.log(mp.mpf(10)) * -400:
        return mp.mpf(0)
    stop = mp.mpf(10) ** -45
    total = mp.mpf(1)                                        # k = a itself
    r, x = mp.mpf(1), a
    while x < hi and r >= stop:
        r = r * ((n1 - x) * (m - x)) / ((x + 1) * (n2 - m + x + 1))
        x += 1
        if r <= mpband:
            total += r
    r, x = mp.mpf(1), a
    while x > lo and r >= stop:
        r = r * (x * (n2 - m + x)) / ((n1 - x + 1) * (m - x + 1))
        x -= 1
        if r <= mpband:
            total += r
    return total * mp.exp(log_pa)


def exact_rel_error(got, exact):
    """|got - exact| / exact of a double against an exact_fisher value, as a float."""
    return float(abs(type(exact)(float(got)) - exact) / exact)


def exact_cases():
    """The tables compared with exact arithmetic: LARGE_TABLES, NEAR_INT32_TABLES and every 7th of small_tables()."""
    return np.concatenate([LARGE_TABLES.astype(np.int64), NEAR_INT32_TABLES, small_tables()[::7].astype(np.int64)])


EXACT_EXCLUDED = [(2000, 0, 0, 2000), (0, 5000, 5000, 0), (900, 0, 1, 900), (1000000, 3, 5, 1000000)]   # exact p below 1e-280


@functools.lru_cache(maxsize=None)
def exact_values():
    """(tables, exact_fisher of each, compared: exact p at least 1e-280) of exact_cases(); computed once, about a second."""
    t = exact_cases()
    exact = [exact_fisher(*row) for row in t.tolist()]
    return t, exact, np.asarray([e >= 1e-280 for e in exact])


def worst_exact_error(p, what):
    """The largest relative error of the doubles p against exact_values() over the compared tables, printed, with its
    table; exactly 1.0 is required on degenerate margins."""
    t, exact, compared = exact_values()
    assert [tuple(row) for row in t[~compared].tolist()] == EXACT_EXCLUDED
    p = np.asarray(p, np.float64)
    assert p.shape == (len(t),) and np.all(p[degenerate(t)] == 1.0) and np.all(p[~compared] < 1e-279)
    rel = np.asarray([exact_rel_error(v, e) if c else 0.0 for v, e, c in zip(p, exact, compared)])
    worst = int(rel.argmax())
    print("largest relative error of the %s p against exact arithmetic over %d tables: %.3e at %s" %
          (what, int(compared.sum()), rel[worst], tuple(t[worst].tolist())))
    return rel, t


# The largest relative error of the host epi_fisher_exact against exact_fisher over exact_cases(), as
# test_cx_compare_host.py::test_fisher_host_against_exact_arithmetic prints it: at (480, 20, 100, 300), p = 9e-122.  The
# bound is 8 times that, the margin of the device-against-host RTOL.
EXACT_MEASURED_REL = 1.003e-13
EXACT_RTOL = 8 * EXACT_MEASURED_REL


def compare_p(got, want, tables, rtol):
    """Device p-values against the host's: NaN where the host has NaN, exactly 1.0 on degenerate margins, exactly equal
    where the host has 0.0, within 1e-300 absolute in the denormal range and within rtol relative elsewhere.  Returns
    the largest relative difference over the normal range."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    deg = degenerate(tables) & ~nan
    assert np.all(got[deg] == 1.0) and np.all(want[deg] == 1.0)
    zero = want == 0.0
    assert np.all(got[zero] == 0.0)
    tiny = ~nan & ~zero & (want < np.finfo(np.float64).tiny)
    assert np.all(np.abs(got[tiny] - want[tiny]) <= 1e-300)
    rest = ~nan & ~zero & ~tiny
    rel = np.abs(got[rest] - want[rest]) / want[rest]
    worst = float(rel.max()) if rel.size else 0.0
    print("largest relative difference of p over %d tables: %.3e (tolerance %.3e)" % (int(rest.sum()), worst, rtol))
    assert worst <= rtol, (worst, tables[rest][int(rel.argmax())].tolist())
    return worst


@functools.lru_cache(maxsize=None)
def fisher_cases():
    """(tables, host p-values) of the kernel test: the small tables, the larger ones, the negative ones."""
    t = np.concatenate([small_tables(), LARGE_TABLES, NEGATIVE_TABLES])
    return t, host_fisher(*t.T)


# ---- random tables ------------------------------------------------------------------------------------------------------

def random_cx(rng, n, npos, nrname=3, depth=40):
    """A sorted CX table of n rows drawn from npos positions per rname, both strands, contexts CG with a few CHG."""
    keys = set()
    while len(keys) < n:
        keys.add((int(rng.integers(1, nrname + 1)), int(rng.integers(1, npos + 1)), int(rng.integers(1, 3))))
    keys = sorted(keys)
    rows = [(r, s, p, 5 if rng.random() < 0.05 else 6, int(rng.integers(0, depth)), int(rng.integers(0, depth))) for r, p, s in keys]
    return cx_table(rows)


def random_comparison(rng, n, run_mean=6):
    """A comparison table of n rows whose significance and direction change in stretches of 1 .. 20 rows: p-values,
    deltas and counts as a region pass reads them (the p column is drawn, not computed, NaN here and there)."""
    rname = np.sort(rng.integers(1, 4, n)).astype(np.int32)
    pos = np.zeros(n, np.int64)
    state = np.zeros(n, np.int64)
    i = 0
    while i < n:
        ln = int(min(rng.integers(1, 21), n - i))
        state[i:i + ln] = rng.integers(-1, 2)
        i += ln
    step = np.where(rng.random(n) < 0.03, rng.integers(400, 900, n), rng.integers(0, 60, n))
    for r in np.unique(rname):
        sel = rname == r
        pos[sel] = 100 + np.cumsum(step[sel])
    cells = rng.integers(0, 50, (n, 4)) + 1
    beta_a = cells[:, 0] / (cells[:, 0] + cells[:, 1])
    delta = np.where(state == 0, rng.choice([0.0, 0.05, -0.05], n), state * rng.uniform(0.2, 0.9, n))
    p = np.where(state == 0, rng.uniform(0.0, 1.0, n), rng.uniform(0.0, 0.05, n))
    p[rng.random(n) < 0.01] = np.nan
    delta[rng.random(n) < 0.01] = np.nan
    out = {"rname": rname, "strand": rng.integers(1, 3, n).astype(np.int32), "pos": pos.astype(np.int32),
           "context": np.full(n, 6, np.int32)}
    for i, k in enumerate(("meth_a", "unmeth_a", "meth_b", "unmeth_b")):
        out[k] = cells[:, i].astype(np.int32)
    out.update(beta_a=beta_a, beta_b=beta_a + delta, delta_beta=delta, p=p)
    return out


def random_cx_vec(rng, n, npos, nrname=3, depth=40):
    """random_cx without the loop: n distinct keys of nrname x npos positions x 2 strands, drawn at once."""
    code = np.sort(rng.choice(nrname * npos * 2, n, replace=False))
    out = {"rname": 1 + code // (2 * npos), "strand": 1 + code % 2, "pos": 1 + code // 2 % npos,
           "context": np.where(rng.random(n) < 0.05, 5, 6), "meth": rng.integers(0, depth, n), "unmeth": rng.integers(0, depth, n)}
    return {k: np.ascontiguousarray(out[k]).astype(np.int32) for k in CX}


def stretches_comparison(rng, stretches):
    """A comparison table on one rname made of (length, state) stretches: state +1 / -1 rows are significant in that
    direction (p = 0.01), state 0 rows are not (p = 0.5, delta_beta 0); neighbours 1 .. 29 bases apart."""
    n = sum(ln for ln, _ in stretches)
    state = np.concatenate([np.full(ln, st, np.int64) for ln, st in stretches]) if stretches else np.zeros(0, np.int64)
    cells = rng.integers(0, 50, (n, 4)) + 1
    out = {"rname": np.ones(n, np.int32), "strand": rng.integers(1, 3, n).astype(np.int32),
           "pos": (100 + np.cumsum(rng.integers(1, 30, n))).astype(np.int32), "context": np.full(n, 6, np.int32)}
    for i, k in enumerate(CMP_INT[4:]):
        out[k] = cells[:, i].astype(np.int32)
    beta_a = cells[:, 0] / (cells[:, 0] + cells[:, 1])
    delta = state * rng.uniform(0.2, 0.9, n)
    out.update(beta_a=beta_a, beta_b=beta_a + delta, delta_beta=delta, p=np.where(state == 0, 0.5, 0.01))
    return out


# Stretches around min_sites = 300 and 5000, longer than a workgroup (256 rows) and than a scan block (4096): the flag
# walk of a run's first row crosses both.  Directions alternate, so no two stretches merge.
LONG_STRETCHES = [(ln, (1, -1, 0)[i % 3]) for i, ln in enumerate(
    (250, 5000, 40, 299, 300, 7, 4999, 301, 1, 6000, 256, 3, 4097, 5001, 9, 700, 298, 2))]
LONG_MIN_SITES = (300, 5000)


def long_stretches_table():
    return stretches_comparison(np.random.default_rng(23), LONG_STRETCHES)


# ---- pooled cells beyond int32 -------------------------------------------------------------------------------------------

M31 = 2 ** 31 - 1


def wide_tables():
    """Hand-made comparison tables whose runs pool 2 to 4 rows with meth_a / meth_b near 2^31 - 1: pooled sums of about
    4.3e9 and 6.4e9 (and 8.6e9), unmeth_* small, so that hi - lo of the pooled table stays below 40 and exact_fisher is
    exact fractions.  Each table ends with a run whose pooled table is degenerate (unmeth_* all 0: p is exactly 1) and a
    run that is (3 M31, 0 / 0, 3 M31): p = 1 / C(6 M31, 3 M31) underflows to exactly 0.  name -> (table, regions_np
    arguments).  delta_beta and p of the rows are set by hand, as a region pass reads them."""
    def table(runs):
        # runs of (delta_beta, [(meth_a, unmeth_a, meth_b, unmeth_b), ...]); one insignificant row between two runs
        rows = []
        for delta, cells in runs:
            rows += [(delta, 0.01) + c for c in cells] + [(0.0, 0.5, 5, 5, 5, 5)]
        n = len(rows)
        m = np.asarray([r[2:] for r in rows], np.int64)
        t = {"rname": np.ones(n, np.int32), "strand": np.asarray([1 + i % 2 for i in range(n)], np.int32),
             "pos": np.arange(10, 10 + 7 * n, 7, dtype=np.int32), "context": np.full(n, 6, np.int32)}
        t.update({k: m[:, i].astype(np.int32) for i, k in enumerate(CMP_INT[4:])})
        with np.errstate(invalid="ignore", divide="ignore"):
            t.update(beta_a=m[:, 0] / (m[:, 0] + m[:, 1]), beta_b=m[:, 2] / (m[:, 2] + m[:, 3]))
        t.update(delta_beta=np.asarray([r[0] for r in rows], np.float64), p=np.asarray([r[1] for r in rows], np.float64))
        return t

    tail = [(0.3, [(M31, 0, M31 - 5, 0), (M31 - 1, 0, M31, 0), (M31, 0, M31, 0)]),     # degenerate: exactly 1
            (-0.9, [(M31, 0, 0, M31)] * 3)]                                            # underflow: exactly 0
    return {
        "two_and_three_rows": (table([(0.3, [(M31, 3, M31 - 100, 11), (M31 - 7, 2, M31, 9)]),
                                      (-0.4, [(M31, 9, M31, 1), (M31 - 1, 12, M31 - 2, 0), (M31, 8, M31 - 3, 2)])] + tail), (0.05, 0.1, 50, 2)),
        "four_rows_and_a_one_sided_run": (table([(0.2, [(M31, 1, M31, 6), (M31, 0, M31, 9), (M31, 2, M31, 5), (M31 - 9, 3, M31, 7)]),
                                                 (-0.2, [(M31, 5, 17, 0), (M31, 7, 4, 1), (M31, 6, 9, 0)]),      # meth_a alone is wide
                                                 (0.5, [(9, 1, M31, 2), (11, 0, M31, 0), (5, 1, M31, 1)])] + tail), (0.05, 0.1, 50, 3)),
    }
