"""What the group comparison and the distribution tails are tested against.

groups_np restates include/epihip.h's epi_cx_groups_dev as a plain loop over the sites in float64, in the header's order
of operations: integer columns, betas, means, variances, phi and Welch's stat and df are what a sequential IEEE evaluation
gives, bit for bit; G goes through a Python restatement of fisher_math.hpp's bd0 and the p-values through the host's
epi_fisher_exact and epi_dist_tail, which test_dist_host.py holds against 50-digit arithmetic (dist_exact).  The grid
and the random points of that comparison are dist_points(), shared with the GPU test."""
import ctypes as C
import functools
import math

import numpy as np

import cx_compare_np as X

CX = X.CX
GROUP_INT = ("rname", "strand", "pos", "context", "meth_a", "unmeth_a", "meth_b", "unmeth_b", "nsamples_a", "nsamples_b")
GROUP_FLOAT = ("beta_a", "beta_b", "delta_beta", "mean_beta_a", "mean_beta_b", "var_a", "var_b", "stat", "df", "phi", "p")
GROUP_COLUMNS = GROUP_INT + GROUP_FLOAT
TESTS = {"fisher": 0, "lrt": 1, "lrt_mn": 2, "welch": 3}
CHISQ, T2, F1 = 0, 1, 2
MAX_RNAME = 2 ** 21 - 1
M31 = 2 ** 31 - 1

# The host epi_dist_tail against dist_exact on dist_points(), measured on the CPU (test_dist_host.py prints the figure
# of a run): the largest relative error where the exact value is at least 1e-300.  The tests allow 8 times it.
DIST_HOST_MEASURED = 6.4e-13
DIST_HOST_RTOL = 8 * DIST_HOST_MEASURED
# The device against the host, measured on an MI355X: the largest relative difference of epi_dist_tail_dev from
# epi_dist_tail over dist_points() (5.69e-14, the F(1, df) tail; Student 5.67e-14, chi-square 4.4e-16) and of G (5.1e-15) and
# p (5.66e-14) over the tables of test_gpu_cx_groups.py and test_gpu_cx_groups_seams.py (the tests print the figures of a
# run; DESIGN 4.18 records them).  The GPU tests allow 8 times it.
DEV_HOST_MEASURED = 5.7e-14
DEV_HOST_RTOL = 8 * DEV_HOST_MEASURED


def host_dist_tail(kind, x, df):
    """The host epi_dist_tail over two array-likes (df may be one value)."""
    from epialleler_amd import _lib
    x = np.ascontiguousarray(np.asarray(x, np.float64).reshape(-1))
    df = np.ascontiguousarray(np.broadcast_to(np.asarray(df, np.float64).reshape(-1), x.shape))
    p = np.empty(x.size, np.float64)
    _lib.check(_lib.load().epi_dist_tail(int(kind), C.c_void_p(x.ctypes.data), C.c_void_p(df.ctypes.data), x.size, C.c_void_p(p.ctypes.data)))
    return p


GRID_X = (0.0, 1e-8, 0.1, 1.0, 2.0, 3.84, 5.0, 10.0, 37.0, 100.0, 1e3, 1400.0)
GRID_DF = (1.0, 1.5, 2.0, 3.7, 10.0, 30.0, 63.0, 100.0, 1e3, 1e4)


def dist_points(nrandom=200, seed=20):
    """(kind, x, df): the grid for each of the three kinds, then nrandom seeded random points per kind -- x log-uniform in
    [1e-6, 2e3] (the square root of that for a t statistic, with a random sign), df log-uniform in [0.5, 1e4]."""
    rng = np.random.default_rng(seed)
    kind, x, df = [], [], []
    for k in (CHISQ, T2, F1):
        for d in GRID_DF:
            for v in GRID_X:
                kind.append(k); x.append(v); df.append(d)
        rx = np.exp(rng.uniform(math.log(1e-6), math.log(2e3), nrandom))
        if k == T2:
            rx = np.sqrt(rx) * rng.choice([-1.0, 1.0], nrandom)
        kind += [k] * nrandom
        x += rx.tolist()
        df += np.exp(rng.uniform(math.log(0.5), math.log(1e4), nrandom)).tolist()
    return np.asarray(kind, np.int32), np.asarray(x, np.float64), np.asarray(df, np.float64)


@functools.lru_cache(maxsize=None)
def _exact_one(kind, x, df):
    import mpmath
    with mpmath.workdps(50):
        x, df = mpmath.mpf(x), mpmath.mpf(df)
        if kind == CHISQ:
            return mpmath.gammainc(df / 2, x / 2, mpmath.inf, regularized=True)
        s = x * x if kind == T2 else x
        if s == 0:
            return mpmath.mpf(1)
        # I_x(df / 2, 1 / 2) with x = df / (df + s) directly where x is the smaller argument; else as 1 - I_y(1 / 2, df / 2),
        # y = s / (df + s), at 450 digits: the difference cancels as many digits as the tail is small (300 at most here)
        if df < s:
            return mpmath.betainc(df / 2, mpmath.mpf(1) / 2, 0, df / (df + s), regularized=True)
    with mpmath.workdps(450):
        x, df = mpmath.mpf(x), mpmath.mpf(df)
        s = x * x if kind == T2 else x
        return +(1 - mpmath.betainc(mpmath.mpf(1) / 2, df / 2, 0, s / (df + s), regularized=True))


def dist_exact(kind, x, df):
    """The tails at 50 digits (mpmath): a list of mpf."""
    return [_exact_one(int(k), float(a), float(d)) for k, a, d in zip(kind, x, df)]


def dist_errors(got, exact):
    """Relative errors of doubles against dist_exact values where the exact value is at least 1e-300 (NaN elsewhere), and
    whether every value below that lies in [0, 1e-300]."""
    import mpmath
    rel = np.full(len(exact), np.nan)
    tiny_ok = True
    for i, (g, e) in enumerate(zip(got, exact)):
        if e >= mpmath.mpf("1e-300"):
            rel[i] = float(abs(mpmath.mpf(float(g)) - e) / e)
        else:
            tiny_ok = tiny_ok and 0.0 <= float(g) <= 1e-300
    return rel, tiny_ok


def rel_diff(got, want):
    """Largest |got - want| / |want| of device values against host values.  NaN sits where the host has NaN, an exact 0 or 1
    of the host (G = 0, p = 1 of a site without a difference; an underflown tail) is the device's too, and below 1e-300
    both are: asserted."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
    exact = (want == 0.0) | (want == 1.0)
    assert np.array_equal(got[exact], want[exact])
    tiny = ~np.isnan(want) & ~exact & (np.abs(want) < 1e-300)
    assert np.all(np.abs(got[tiny]) < 1e-300)
    ok = ~np.isnan(want) & ~exact & ~tiny
    return float(np.max(np.abs(got[ok] - want[ok]) / np.abs(want[ok]))) if ok.any() else 0.0


def bd0(x, e):
    """csrc/fisher_math.hpp's bd0 in Python floats."""
    if abs(x - e) < 0.1 * (x + e):
        v = (x - e) / (x + e)
        s = (x - e) * v
        ej = 2 * x * v
        v *= v
        for j in range(1, 1000):
            ej *= v
            s1 = s + ej / (2 * j + 1)
            if s1 == s:
                return s1
            s = s1
        return s
    return x * math.log(x / e) + e - x


def dev_term(x, e):
    return e if x == 0 else bd0(float(x), e)


def g_statistic(ma, ua, mb, ub):
    na, nb = float(ma + ua), float(mb + ub)
    n = float(ma + ua + mb + ub)
    p0, q0 = float(ma + mb) / n, float(ua + ub) / n
    return 2.0 * (((dev_term(ma, na * p0) + dev_term(ua, na * q0)) + dev_term(mb, nb * p0)) + dev_term(ub, nb * q0))


def site_key(t, i):
    return (int(t["rname"][i]), int(t["pos"][i]), int(t["strand"][i]), int(t["context"][i]))


def groups_np(tabs_a, tabs_b, min_coverage=1, min_samples_a=None, min_samples_b=None, test="lrt"):
    """The group comparison of two lists of CX tables: dict of the 21 columns and `nsites`."""
    lo = max(int(min_coverage), 1)
    min_a = len(tabs_a) if min_samples_a is None else min_samples_a
    min_b = len(tabs_b) if min_samples_b is None else min_samples_b
    sites = {}
    for k, t in enumerate(list(tabs_a) + list(tabs_b)):
        for i in range(t["pos"].size):
            sites.setdefault(site_key(t, i), []).append((k, int(t["meth"][i]), int(t["unmeth"][i])))
    nan = float("nan")
    rows, nsites = [], 0
    for key in sorted(sites):
        counting = [(k, m, u) for k, m, u in sites[key] if m + u >= lo]       # in sample order
        nsites += 1 if counting else 0
        grp = [[(m, u) for k, m, u in counting if k < len(tabs_a)], [(m, u) for k, m, u in counting if k >= len(tabs_a)]]
        if len(grp[0]) < min_a or len(grp[1]) < min_b:
            continue
        M = [sum(m for m, u in g) for g in grp]
        U = [sum(u for m, u in g) for g in grp]
        assert max(M[0] + U[0], M[1] + U[1]) <= M31, "pooled coverage beyond int32: the device refuses the call"
        cnt = [len(g) for g in grp]
        beta = [np.float64(M[g]) / np.float64(M[g] + U[g]) for g in (0, 1)]
        mean, var = [], []
        X2 = np.float64(0.0)
        for g in (0, 1):
            s = np.float64(0.0)
            for m, u in grp[g]:
                s = s + np.float64(m) / np.float64(m + u)
            mean.append(s / np.float64(cnt[g]))
        for g in (0, 1):
            ss = np.float64(0.0)
            for m, u in grp[g]:
                dev = np.float64(m) / np.float64(m + u) - mean[g]
                ss = ss + dev * dev
                ex = np.float64(m + u) * beta[g]
                den = ex * (np.float64(1.0) - beta[g])
                res = np.float64(m) - ex
                if den != 0.0:
                    X2 = X2 + res * res / den
            var.append(ss / np.float64(cnt[g] - 1) if cnt[g] >= 2 else np.float64(nan))
        stat = df = phi = p = nan
        if test == "fisher":
            p = float(X.host_fisher([M[0]], [U[0]], [M[1]], [U[1]])[0])
        elif test == "welch":
            if cnt[0] >= 2 and cnt[1] >= 2:
                va, vb = var[0] / np.float64(cnt[0]), var[1] / np.float64(cnt[1])
                s2 = va + vb
                if s2 != 0.0:
                    with np.errstate(all="ignore"):
                        stat = float((mean[1] - mean[0]) / np.sqrt(s2))
                        df = float(s2 * s2 / (va * va / np.float64(cnt[0] - 1) + vb * vb / np.float64(cnt[1] - 1)))
                    p = float(host_dist_tail(T2, [stat], [df])[0])
        else:
            G = g_statistic(M[0], U[0], M[1], U[1])
            if test == "lrt":
                stat, df = G, 1.0
                p = float(host_dist_tail(CHISQ, [G], [1.0])[0])
            else:
                n = cnt[0] + cnt[1]
                df = float(n - 2)
                if n > 2:
                    over = float(X2) / df
                    phi = over if over > 1.0 else 1.0
                    stat = G / phi
                    p = float(host_dist_tail(F1, [stat], [df])[0])
        rows.append((key[0], key[2], key[1], key[3], M[0], U[0], M[1], U[1], cnt[0], cnt[1],
                     float(beta[0]), float(beta[1]), float(beta[1] - beta[0]), float(mean[0]), float(mean[1]), float(var[0]), float(var[1]),
                     stat, df, phi, p))
    out = {k: np.asarray([r[i] for r in rows], np.int32 if i < 10 else np.float64) for i, k in enumerate(GROUP_COLUMNS)}
    out["nsites"] = nsites
    return out


def random_groups(rng, n_a, n_b, nrows, npos, depth=30, disjoint=False, rname_max=3):
    """n_a + n_b sorted CX tables of about nrows rows each drawn from npos positions: a shared per-site methylation level
    with a group shift and sample noise, so that every test has signal, ties and nothing.  disjoint: every sample draws from
    a position set of its own (no site is shared)."""
    K = n_a + n_b
    base = rng.random(npos)
    tabs = []
    for k in range(K):
        n = min(int(nrows), npos)
        idx = np.sort(rng.choice(npos, n, replace=False)) if n else np.zeros(0, np.int64)
        pos = idx * (K if disjoint else 1) + (k if disjoint else 0)
        lvl = np.clip(base[idx] + (0.25 if k >= n_a else 0.0) * (idx % 3 == 0) + rng.normal(0, 0.08, n), 0, 1)
        lvl[idx % 11 == 0] = 1.0                                   # all-methylated sites: G = 0, zero variance
        lvl[idx % 13 == 0] = 0.0
        cov = rng.integers(0, depth + 1, n)
        meth = rng.binomial(cov, lvl)
        rname = 1 + idx * rname_max // max(npos, 1)
        strand = 1 + (idx & 1)
        ctx = np.where(idx % 5 == 0, 6, 7)
        if not disjoint and n:                                     # a few rows whose context differs from the other samples'
            ctx = np.where((idx % 97 == 3) & (k % 2 == 1), 2, ctx)
        tabs.append(X.cx_table(np.stack([rname, strand, pos, ctx, meth, cov - meth], 1)))
    for t in tabs:
        assert X.is_sorted(t)
    return tabs[:n_a], tabs[n_a:]


# A table written by hand: 2 + 3 samples.  Site 100 is in every sample; 200 is missing from a's second sample; at 300 b's
# third sample is below min_coverage = 4; at 400 a's first sample has another context (two sites); 500 is all-methylated;
# 600 has zero variance in both groups (and differs between them).
KAT_A = [X.cx_table([(1, 1, 100, 7, 8, 2), (1, 2, 200, 7, 3, 7), (1, 1, 300, 7, 5, 5), (1, 1, 400, 6, 6, 4), (1, 1, 500, 7, 10, 0), (2, 1, 600, 7, 2, 6)]),
         X.cx_table([(1, 1, 100, 7, 6, 4), (1, 1, 300, 7, 4, 6), (1, 1, 400, 7, 5, 5), (1, 1, 500, 7, 8, 0), (2, 1, 600, 7, 3, 9)])]
KAT_B = [X.cx_table([(1, 1, 100, 7, 2, 8), (1, 2, 200, 7, 9, 1), (1, 1, 300, 7, 9, 1), (1, 1, 400, 7, 1, 9), (1, 1, 500, 7, 7, 0), (2, 1, 600, 7, 6, 2)]),
         X.cx_table([(1, 1, 100, 7, 1, 9), (1, 2, 200, 7, 8, 2), (1, 1, 300, 7, 8, 2), (1, 1, 400, 7, 2, 8), (1, 1, 500, 7, 9, 0), (2, 1, 600, 7, 9, 3)]),
         X.cx_table([(1, 1, 100, 7, 3, 7), (1, 2, 200, 7, 7, 3), (1, 1, 300, 7, 2, 1), (1, 1, 400, 7, 3, 7), (1, 1, 500, 7, 4, 0), (2, 1, 600, 7, 3, 1)])]
KAT_MIN_COVERAGE = 4
