"""rcpp_cx_compare_groups timed on 4 + 4 device cytosine tables of about a million rows each, next to the path a user has
without it: every table fetched to the host, joined in numpy, the test per cytosine on the host with scipy -- the driver of
profiles/cx_groups.txt.
    python scratch/cx_groups_profile.py [rows per sample]
The tables are made on the device: every sample draws its rows from one grid of positions (rows / 0.85 of them, four
sequences, both strands), coverage 5 .. 40, a per-site methylation level with a group shift at every fifth site and sample
noise.  Whole calls: median [min, max] of 9 repeats after one untimed call, stream synchronised, as_device (nothing copied
to the host); kernels from the epi_prof labels "cxg_key" (order and range checks, keys), "cxg_sort" (the seven radix
passes), "cxg_flag" (sites, flags, scan) and "cxg_emit" (the rows and their test); the host steps by the wall clock, 3 repeats
(Welch's test on the host over the first 100 000 sites only: scipy's masked t-test takes minutes on a million)."""
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.argv, argv = [sys.argv[0], "none"], sys.argv
sys.path[:0] = [HERE]
from heterogeneity_profile import ea, kernel_ms, np, timed, torch  # noqa: E402

sys.argv = argv
CX = ("rname", "strand", "pos", "context", "meth", "unmeth")
LEVELS = ("chrS1", "chrS2", "chrS3", "chrS4")


def host_timed(fn, reps=3):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return r, "%.1f ms [%.1f, %.1f]" % (statistics.median(ts), min(ts), max(ts))


def sample(rows, grid, k, in_b, gen):
    idx = torch.sort(torch.randperm(grid, device="cuda", generator=gen)[:rows]).values
    level = ((idx * 2654435761) % 1000).double() / 1000.0                       # the site's level: a function of the site
    level = (level + (0.25 if in_b else 0.0) * (idx % 5 == 0) + 0.08 * torch.randn(rows, device="cuda", generator=gen, dtype=torch.float64)).clamp(0, 1)
    cov = torch.randint(5, 41, (rows,), device="cuda", generator=gen)
    meth = torch.binomial(cov.double(), level, generator=gen).to(torch.int32)
    per = (grid + 3) // 4
    cols = dict(rname=(1 + idx // per), strand=(1 + (idx & 1)), pos=(1 + idx % per), context=torch.full_like(idx, 7), meth=meth, unmeth=cov.to(torch.int32) - meth)
    return ea.Report({c: cols[c].to(torch.int32).contiguous() for c in CX}, LEVELS)


def host_join(tabs, n_a, min_coverage):
    """K host CX tables -> per site and sample (meth, unmeth) with 0 where the sample does not count; sites every sample
    of both groups counts at."""
    key = [(t["rname"].astype(np.int64) << 35) | (t["pos"].astype(np.int64) << 4) | ((t["strand"].astype(np.int64) - 1) << 3) | t["context"] for t in tabs]
    sites = np.unique(np.concatenate(key))
    m = np.zeros((len(tabs), sites.size), np.int64)
    u = np.zeros_like(m)
    for k, t in enumerate(tabs):
        at = np.searchsorted(sites, key[k])
        ok = t["meth"].astype(np.int64) + t["unmeth"] >= min_coverage
        m[k, at[ok]], u[k, at[ok]] = t["meth"][ok], t["unmeth"][ok]
    keep = ((m + u) > 0).all(axis=0)
    return m[:, keep], u[:, keep]


def host_lrt(m, u, n_a):
    from scipy import stats, special
    M = np.stack([m[:n_a].sum(0), m[n_a:].sum(0)]).astype(np.float64)
    U = np.stack([u[:n_a].sum(0), u[n_a:].sum(0)]).astype(np.float64)
    N = M + U
    p0 = M.sum(0) / N.sum(0)
    G = 2 * (special.xlogy(M, M / (N * p0)) + special.xlogy(U, U / (N * (1 - p0)))).sum(0)
    return stats.chi2.sf(np.maximum(G, 0), 1)


def host_welch(m, u, n_a):
    from scipy import stats
    beta = m / (m + u)
    return stats.ttest_ind(beta[n_a:], beta[:n_a], axis=0, equal_var=False).pvalue


if __name__ == "__main__":
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    n_a = n_b = 4
    gen = torch.Generator(device="cuda")
    gen.manual_seed(18)
    grid = int(rows / 0.85)
    reps = [sample(rows, grid, k, k >= n_a, gen) for k in range(n_a + n_b)]
    print("%d + %d device CX tables of %d rows each on one grid of %d sites, coverage 5 .. 40" % (n_a, n_b, rows, grid))
    for test in ("lrt", "lrt_mn", "welch", "fisher"):
        call = lambda: ea.rcpp_cx_compare_groups(reps[:n_a], reps[n_a:], 5, None, None, test, as_device=True)
        rep, t_call = timed(call, 9)
        print("  rcpp_cx_compare_groups test=%-7s %s   %d sites, %d rows" % (test, t_call, rep.nsites, rep.nrow))
        for label in ("cxg_key", "cxg_sort", "cxg_flag", "cxg_emit"):
            print("  ... %-30s%s" % (label, kernel_ms(call, label, 9)))
        sys.stdout.flush()
    some = lambda: ea.rcpp_cx_compare_groups(reps[:n_a], reps[n_a:], 5, 2, 2, "lrt_mn", as_device=True)
    rep2, t_some = timed(some, 9)
    print("  ... min_samples 2 + 2, lrt_mn         %s   %d rows" % (t_some, rep2.nrow))
    # the path without the call
    tabs, t_fetch = host_timed(lambda: [{k: r[k].cpu().numpy() for k in CX} for r in reps])
    (m, u), t_join = host_timed(lambda: host_join(tabs, n_a, 5))
    p_lrt, t_lrt = host_timed(lambda: host_lrt(m, u, n_a))
    sub = min(100_000, m.shape[1])
    p_w, t_w = host_timed(lambda: host_welch(m[:, :sub], u[:, :sub], n_a))
    print("  all %d tables to the host                %s" % (len(reps), t_fetch))
    print("  numpy join (unique + searchsorted)      %s   %d sites with every sample" % (t_join, m.shape[1]))
    print("  numpy G + scipy chi2.sf                 %s" % t_lrt)
    print("  scipy ttest_ind(equal_var=False), first %d sites  %s" % (sub, t_w))
    dev = ea.rcpp_cx_compare_groups(reps[:n_a], reps[n_a:], 5, None, None, "lrt")
    assert dev["p"].size == p_lrt.size
    ok = p_lrt > 1e-290
    print("  device p against the host's (lrt): largest relative difference %.3e over %d sites" %
          (float(np.max(np.abs(dev["p"][ok] - p_lrt[ok]) / p_lrt[ok])), int(ok.sum())))
