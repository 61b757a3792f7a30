"""compareCytosineReports timed on a cfg2-like pair of batches, next to the path a user has without it: both cytosine
reports fetched to the host, joined in numpy, the host epi_fisher_exact with 16 threads -- the driver of
profiles/cx_compare.txt.
    python scratch/cx_compare_profile.py [rows]     two batches like bench.py's cfg2 on one site grid (the pair of
                                                    heterogeneity_compare_profile.py), un-thresholded CG reports
Whole calls: median [min, max] of 9 repeats after one untimed call, stream synchronised, as_device (nothing copied to the
host); kernels from the epi_prof labels "cxcmp_match" (order checks, match, scan), "cxcmp_emit", "fisher_exact",
"cxcmp_region_flag" (flags + scan), "cxcmp_region_emit"; the host steps by the wall clock, 3 repeats."""
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.argv, argv = [sys.argv[0], "none"], sys.argv
sys.path[:0] = [HERE]
from heterogeneity_compare_profile import cfg2_like, ea, kernel_ms, np, timed, torch  # noqa: E402

sys.argv = argv
CX = ("rname", "strand", "pos", "context", "meth", "unmeth")


def host_timed(fn, reps=3):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return r, "%.1f ms [%.1f, %.1f]" % (statistics.median(ts), min(ts), max(ts))


def host_join(ta, tb):
    """The common rows of two host CX tables (same rname, strand, pos and context): their cells."""
    key = lambda t: (t["rname"].astype(np.int64) << 34) | (t["pos"].astype(np.int64) << 2) | t["strand"].astype(np.int64)
    _, ia, ib = np.intersect1d(key(ta), key(tb), assume_unique=True, return_indices=True)
    same = ta["context"][ia] == tb["context"][ib]
    ia, ib = ia[same], ib[same]
    return {"a": ta["meth"][ia], "b": ta["unmeth"][ia], "c": tb["meth"][ib], "d": tb["unmeth"][ib]}


if __name__ == "__main__":
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    a, b = cfg2_like(rows, 5), cfg2_like(rows, 6)
    a.batch(); b.batch()
    print("cfg2-like pair: 2 x %d rows of 300 bytes, uniform starts, depth 30, one site grid; un-thresholded CG reports" % rows)
    cx = lambda x: ea.generateCytosineReport(x, threshold_reads=False, report_context="CG", as_device=True)
    ra, rb = cx(a), cx(b)
    join = lambda: ea.rcpp_cx_compare(ra, rb, 1, as_device=True)
    rep, t_join = timed(join, 9)
    print("  CX rows %d and %d, common sites %d, rows reported %d" % (ra.nrow, rb.nrow, rep.ncommon, rep.nrow))
    cov = (rep["meth_a"] + rep["unmeth_a"] + rep["meth_b"] + rep["unmeth_b"]).double()
    print("  cells per table: mean sum %.1f, largest %d" % (cov.mean().item(), int(cov.max().item())))
    _, t_two = timed(lambda: (cx(a), cx(b)), 9)
    _, t_whole = timed(lambda: ea.compareCytosineReports(a, b, threshold_reads=False, as_device=True), 9)
    print("  the two generateCytosineReport calls          %s" % t_two)
    print("  compareCytosineReports (reports + join)       %s" % t_whole)
    print("  rcpp_cx_compare (join + Fisher)               %s" % t_join)
    for label in ("cxcmp_match", "cxcmp_emit", "fisher_exact"):
        print("  ... %-42s%s" % (label, kernel_ms(join, label, 9)))
    regions = lambda: ea.rcpp_cx_compare_regions(rep, as_device=True)
    reg, t_reg = timed(regions, 9)
    print("  rcpp_cx_compare_regions (defaults)            %s   %d regions" % (t_reg, reg.nrow))
    for label in ("cxcmp_region_flag", "cxcmp_region_emit"):
        print("  ... %-42s%s" % (label, kernel_ms(regions, label, 9)))
    sys.stdout.flush()
    # the path without the comparison
    (ta, tb), t_fetch = host_timed(lambda: tuple({k: r[k].cpu().numpy() for k in CX} for r in (ra, rb)))
    cells, t_hjoin = host_timed(lambda: host_join(ta, tb))
    p_host, t_fisher = host_timed(lambda: ea.rcpp_fep(cells, tuple("abcd"), nthreads=16))
    print("  both tables to the host                       %s" % t_fetch)
    print("  numpy join (intersect1d on a 64-bit key)      %s" % t_hjoin)
    print("  host epi_fisher_exact, 16 threads, %8d tables  %s" % (p_host.size, t_fisher))
    p_dev = rep["p"].cpu().numpy()
    assert p_dev.size == p_host.size
    ok = p_host > 0
    print("  device p against host p: largest relative difference %.3e over %d tables" %
          (float(np.max(np.abs(p_dev[ok] - p_host[ok]) / p_host[ok])), int(ok.sum())))
