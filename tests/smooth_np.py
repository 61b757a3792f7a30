"""Plain restatements (loops and numpy, no GPU result read) of CpG strand merging and of the local-regression smoother as
include/epihip.h defines them (epi_cx_merge_strands_dev, epi_cx_smooth_dev), the exact-arithmetic form of the fit, and
the tables the tests of both share.  The smoother's sums run in the header's order: the per-site terms are elementwise IEEE
operations, and every sum is sequential (np.add.accumulate(...)[-1]; np.sum is pairwise and would not do).  D_i is taken
from its definition (the k-th smallest distance in the cluster), not from the kernel's binary search.  Test
infrastructure only; treat what the functions return as read-only."""
import fractions

import numpy as np

CX = ("rname", "strand", "pos", "context", "meth", "unmeth")
SMOOTH_INT = CX + ("nsites", "halfwidth", "degree")
SMOOTH_FLOAT = ("beta", "smoothed", "weight")
SMOOTH_COLUMNS = SMOOTH_INT + SMOOTH_FLOAT
CG, CHG, CHH = 7, 6, 2
K_PIVOT = 1e-4
MAX_WINDOW = 65536


def cx_table(rows):
    """rows of (rname, strand, pos, context, meth, unmeth) -> the six int32 columns"""
    m = np.asarray(rows, np.int64).reshape(-1, 6)
    return {k: np.ascontiguousarray(m[:, i]).astype(np.int32) for i, k in enumerate(CX)}


def rows_of(t):
    return list(zip(*[np.asarray(t[k]).tolist() for k in CX]))


def is_sorted(t):
    key = list(zip(np.asarray(t["rname"]).tolist(), np.asarray(t["pos"]).tolist(), np.asarray(t["strand"]).tolist()))
    return all(x < y for x, y in zip(key, key[1:]))


# ---- merge ---------------------------------------------------------------------------------------------------------------

def merge_np(t):
    """The merged table of the CX table t and (nmerged, nmoved, nkept); ValueError where the call gives EPI_ERR_ARG."""
    rows = rows_of(t)
    if not is_sorted(t) or any(s not in (1, 2) or m < 0 or u < 0 for _, s, _, _, m, u in rows):
        raise ValueError("bad table")
    out, nmerged, nmoved, nkept = [], 0, 0, 0
    for i, (rname, strand, q, ctx, m, u) in enumerate(rows):
        if not (strand == 2 and ctx == CG):
            out.append((rname, strand, q, ctx, m, u))
            continue
        prev = rows[i - 1] if i > 0 else None
        if prev is not None and prev[:4] == (rname, 1, q - 1, CG):
            if m + prev[4] > 2 ** 31 - 1 or u + prev[5] > 2 ** 31 - 1:
                raise ValueError("overflow")
            assert out[-1] == prev                                       # (a '+' row is copied)
            out[-1] = (rname, 1, q - 1, CG, m + prev[4], u + prev[5])
            nmerged += 1
        elif q >= 2 and (prev is None or (prev[0], prev[2], prev[1]) < (rname, q - 1, 1)):
            out.append((rname, 1, q - 1, ctx, m, u))
            nmoved += 1
        else:
            out.append((rname, strand, q, ctx, m, u))
            nkept += 1
    res = cx_table(out)
    res.update(nmerged=nmerged, nmoved=nmoved, nkept=nkept)
    return res


# ---- smooth --------------------------------------------------------------------------------------------------------------

def window_sums(pos, meth, cov, i, H):
    """(S0 .. S4, T0 .. T2, first site, end) of the window of site i of one cluster (int64 arrays) with half-width H"""
    d_all = pos - pos[i]
    inside = np.flatnonzero(np.abs(d_all) < H)
    jlo, jhi = int(inside[0]), int(inside[-1]) + 1
    assert np.array_equal(inside, np.arange(jlo, jhi))
    d = d_all[jlo:jhi]
    u = d.astype(np.float64) / np.float64(H)
    a = np.abs(u)
    c = 1.0 - (a * a) * a
    t = (c * c) * c
    u2 = u * u
    w = t * cov[jlo:jhi].astype(np.float64)
    v = t * meth[jlo:jhi].astype(np.float64)
    wu2, vu2 = w * u2, v * u2
    terms = np.stack([w, w * u, wu2, wu2 * u, wu2 * u2, v, v * u, vu2], 1)
    sums = np.add.accumulate(np.concatenate([np.zeros((1, 8)), terms]), axis=0)[-1]    # sequential, from 0.0
    return [float(x) for x in sums], jlo, jhi


def solve(S, degree):
    """(smoothed, degree_used) from the eight sums"""
    S0, S1, S2, S3, S4, T0, T1, T2 = S
    if not S0 > 0.0:
        return float("nan"), -1
    d0 = S0
    l10 = S1 / d0
    d1 = S2 - l10 * S1
    used = 0
    if degree >= 1 and d1 > K_PIVOT * S2:
        used = 1
        if degree == 2:
            l20 = S2 / d0
            l21 = (S3 - l20 * S1) / d1
            d2 = (S4 - l20 * S2) - l21 * (l21 * d1)
            if d2 > K_PIVOT * S4:
                used = 2
    if used == 0:
        a0 = T0 / d0
    else:
        z1 = T1 - l10 * T0
        if used == 1:
            a1 = z1 / d1
            a0 = T0 / d0 - l10 * a1
        else:
            z2 = (T2 - l20 * T0) - l21 * z1
            a2 = z2 / d2
            a1 = z1 / d1 - l21 * a2
            a0 = (T0 / d0 - l10 * a1) - l20 * a2
    return min(1.0, max(0.0, a0)), used


def knn_distance(pos, i, k):
    """the smallest distance within which k sites of the cluster lie, site i included"""
    return int(np.sort(np.abs(pos - pos[i]))[k - 1])


def smooth_series(pos, meth, unmeth, bandwidth=1000, min_sites=70, max_gap=10 ** 8, degree=2):
    """One series (pos ascending): per site nsites, halfwidth, degree, smoothed, weight, and the number of clusters"""
    pos, meth, unmeth = (np.asarray(x, np.int64) for x in (pos, meth, unmeth))
    n = pos.size
    out = dict(nsites=np.zeros(n, np.int32), halfwidth=np.zeros(n, np.int32), degree=np.zeros(n, np.int32),
               smoothed=np.zeros(n, np.float64), weight=np.zeros(n, np.float64))
    cuts = [0] + [j for j in range(1, n) if pos[j] - pos[j - 1] > max_gap] + [n]
    for lo, hi in zip(cuts, cuts[1:]):
        cp, cm, cc = pos[lo:hi], meth[lo:hi], meth[lo:hi] + unmeth[lo:hi]
        k = min(min_sites, hi - lo)
        for i in range(hi - lo):
            H = max(bandwidth, knn_distance(cp, i, k))
            S, jlo, jhi = window_sums(cp, cm, cc, i, H)
            if jhi - jlo > MAX_WINDOW:
                raise ValueError("window")
            sm, used = solve(S, degree)
            out["nsites"][lo + i] = jhi - jlo; out["halfwidth"][lo + i] = H; out["degree"][lo + i] = used
            out["smoothed"][lo + i] = sm; out["weight"][lo + i] = S[0]
    out["ncluster"] = len(cuts) - 1
    return out


def smooth_np(t, bandwidth=1000, min_sites=70, max_gap=10 ** 8, degree=2):
    """The smoothed table of the CX table t (the twelve columns, `ncluster`, `max_window`); ValueError where the call gives
    EPI_ERR_ARG."""
    cols = {k: np.asarray(t[k], np.int64) for k in CX}
    n = cols["pos"].size
    if not is_sorted(t) or (n and (not np.isin(cols["strand"], (1, 2)).all() or cols["context"].min() < 0 or cols["context"].max() > 7 or
                                   min(cols["pos"].min(), cols["meth"].min(), cols["unmeth"].min()) < 0)):
        raise ValueError("bad table")
    out = {k: np.asarray(t[k], np.int32).copy() for k in CX}
    for k in ("nsites", "halfwidth", "degree"):
        out[k] = np.zeros(n, np.int32)
    with np.errstate(invalid="ignore", divide="ignore"):
        out["beta"] = cols["meth"].astype(np.float64) / (cols["meth"] + cols["unmeth"]).astype(np.float64)
    out["smoothed"], out["weight"] = np.zeros(n, np.float64), np.zeros(n, np.float64)
    series = {}
    for i, key in enumerate(zip(cols["rname"].tolist(), cols["strand"].tolist(), cols["context"].tolist())):
        series.setdefault(key, []).append(i)
    ncluster = 0
    for idx in series.values():
        idx = np.asarray(idx)
        r = smooth_series(cols["pos"][idx], cols["meth"][idx], cols["unmeth"][idx], bandwidth, min_sites, max_gap, degree)
        for k in ("nsites", "halfwidth", "degree", "smoothed", "weight"):
            out[k][idx] = r[k]
        ncluster += r["ncluster"]
    out["ncluster"] = ncluster
    out["max_window"] = int(out["nsites"].max()) if n else 0
    return out


def smooth_exact(pos, meth, unmeth, i, H, used):
    """The fit of degree `used` (0 .. 2) at site i over the window |pos_j - pos_i| < H in exact rational arithmetic, clamped
    to [0, 1].  The common factor H^-9 of the tricube weights cancels and a polynomial in d = pos_j - pos_i has the
    intercept of the one in u = d / H, so the moments are integers."""
    s, t = [0] * 5, [0] * 3
    for p, m, u in zip(pos, meth, unmeth):
        d = int(p) - int(pos[i])
        if abs(d) >= H:
            continue
        w = (H ** 3 - abs(d) ** 3) ** 3
        for k in range(5):
            s[k] += w * (int(m) + int(u)) * d ** k
        for k in range(3):
            t[k] += w * int(m) * d ** k
    F = fractions.Fraction
    if used == 0:
        a0 = F(t[0], s[0])
    elif used == 1:
        a0 = F(t[0] * s[2] - t[1] * s[1], s[0] * s[2] - s[1] * s[1])
    else:
        det = lambda m: (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
                         m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))
        A = [[s[0], s[1], s[2]], [s[1], s[2], s[3]], [s[2], s[3], s[4]]]
        B = [[t[0], s[1], s[2]], [t[1], s[2], s[3]], [t[2], s[3], s[4]]]
        a0 = F(det(B), det(A))
    return min(F(1), max(F(0), a0))


# ---- tables --------------------------------------------------------------------------------------------------------------

GAP_KINDS = ("uniform", "geometric", "bursty", "ones")


def random_series(rng, n, kind, depth=8, zero_frac=0.3, start=None):
    """(pos, meth, unmeth) of n sites: gaps of `kind`, Poisson(depth) coverage, zero_frac of the sites without coverage"""
    if kind == "uniform":
        gaps = rng.integers(1, 400, n)
    elif kind == "geometric":
        gaps = rng.geometric(0.01, n)
    elif kind == "bursty":
        gaps = np.where(rng.random(n) < 0.85, rng.integers(1, 6, n), rng.integers(500, 5000, n))
    else:
        gaps = np.ones(n, np.int64)
    pos = np.cumsum(gaps) + (int(rng.integers(0, 10 ** 6)) if start is None else start)
    cov = rng.poisson(depth, n) * (rng.random(n) >= zero_frac)
    meth = rng.binomial(cov, rng.random(n) if n else 0.5)
    return pos.astype(np.int64), meth.astype(np.int64), (cov - meth).astype(np.int64)


def series_table(series):
    """A CX table from [(rname, strand, context, pos, meth, unmeth)] series, in table order"""
    rows = [(r, s, int(p), c, int(m), int(u)) for r, s, c, pos, meth, unmeth in series for p, m, u in zip(pos, meth, unmeth)]
    rows.sort(key=lambda x: (x[0], x[2], x[1]))
    t = cx_table(rows)
    assert is_sorted(t)
    return t


def random_cx(rng, n, n_rname=2, cpg_frac=0.6):
    """A CX table of about n rows as a cytosine report has them: CpGs with a '+' row at pos and a '-' row at pos + 1 (either
    may be missing), CHG and CHH rows on either strand in between, now and then a non-CG '+' row right before a '-' CpG."""
    sites = {}
    per = max(n // n_rname, 1)
    for rname in range(1, n_rname + 1):
        pos = np.cumsum(rng.choice([1, 1, 2, 3, 7, 40, 300], per)) + int(rng.integers(1, 50))
        for p in pos.tolist():
            x = rng.random()
            if x < cpg_frac:
                which = rng.random()
                if which < 0.7 or which >= 0.85:
                    sites.setdefault((rname, p, 1), CG)
                if which < 0.85 and (rname, p + 1, 2) not in sites:
                    sites[(rname, p + 1, 2)] = CG
            else:
                sites.setdefault((rname, p, int(rng.integers(1, 3))), CHG if x < 0.8 else CHH)
    keys = sorted(sites)[:n]
    cov = rng.poisson(6, len(keys)) * (rng.random(len(keys)) >= 0.2)
    meth = rng.binomial(cov, rng.random(len(keys)))
    t = cx_table([(r, s, p, sites[(r, p, s)], int(m), int(c - m)) for (r, p, s), m, c in zip(keys, meth, cov)])
    assert is_sorted(t)
    return t


# hand-written merge table: (rows, merged rows, nmerged, nmoved, nkept)
MERGE_KAT = cx_table([
    (1, 2, 1, CG, 1, 1),        # '-' CpG at q = 1: nowhere to go, stays
    (1, 1, 10, CG, 3, 1), (1, 2, 11, CG, 2, 4),        # a pair
    (1, 2, 21, CG, 5, 0),       # lone '-' CpG: moves to (20, '+')
    (1, 1, 30, CHH, 1, 2), (1, 2, 31, CG, 2, 2),       # blocked by (30, '+', CHH): stays
    (1, 2, 40, CHG, 0, 3), (1, 2, 41, CG, 1, 1),       # blocked by (40, '-'): stays
    (1, 1, 50, CHG, 4, 4), (1, 2, 50, CHH, 0, 1), (1, 2, 52, CG, 7, 7),   # non-CG rows copied; (52, '-') moves behind (50, '-')
    (1, 1, 60, CG, 9, 1),       # '+' CpG without a '-' row: copied
    (2, 2, 5, CG, 0, 0),        # first row of an rname: moves to (4, '+')
    (2, 1, 9, CG, 1, 0), (2, 2, 10, CG, 0, 1), (2, 2, 11, CG, 2, 2),      # a pair, then a '-' CpG right behind its '-' row: blocked, stays
])
MERGE_KAT_WANT = cx_table([
    (1, 2, 1, CG, 1, 1), (1, 1, 10, CG, 5, 5), (1, 1, 20, CG, 5, 0), (1, 1, 30, CHH, 1, 2), (1, 2, 31, CG, 2, 2), (1, 2, 40, CHG, 0, 3),
    (1, 2, 41, CG, 1, 1), (1, 1, 50, CHG, 4, 4), (1, 2, 50, CHH, 0, 1), (1, 1, 51, CG, 7, 7), (1, 1, 60, CG, 9, 1), (2, 1, 4, CG, 0, 0),
    (2, 1, 9, CG, 1, 1), (2, 2, 11, CG, 2, 2)])
MERGE_KAT_COUNTS = dict(nmerged=2, nmoved=3, nkept=4)
MERGE_OVERFLOW = cx_table([(1, 1, 10, CG, 2 ** 31 - 1, 0), (1, 2, 11, CG, 1, 0)])


def same(got, want, what=""):
    """Integer columns equal, float columns bit for bit (NaN where want has NaN)"""
    for k in want:
        if k not in SMOOTH_COLUMNS:
            continue
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        if w.dtype.kind == "f":
            assert g.dtype == np.float64 and np.array_equal(g.view(np.uint64) | (np.isnan(g) * np.uint64(2 ** 63 - 1)),
                                                            w.view(np.uint64) | (np.isnan(w) * np.uint64(2 ** 63 - 1))), (what, k)
        else:
            assert np.array_equal(g, w), (what, k, np.flatnonzero(g != w)[:5])
