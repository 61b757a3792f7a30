"""adjustPValues timed on the p column of a cfg2-like comparison table, next to the path a user has without it (the column
fetched to the host, the numpy restatement of tests/padjust_np.py) and, as a yardstick for the sort alone, torch.sort(stable=True)
of the same device column -- the driver of profiles/p_adjust.txt.
    python scratch/p_adjust_profile.py [rows]     the pair of cx_compare_profile.py (2 x rows, 7.0 M table rows at the default)
The two device paths are timed against each other in rounds of alternating order, 9 rounds after one untimed round, then the
host path 9 times: median [min, max], stream synchronised.
Kernels from the epi_prof labels "padj_keys" (keys + plan), "rsort_hist", "rsort_table_scan", "rsort_scatter" (radix_sort.hip; each
summed over the digit passes), "padj_terms", "padj_dscan", "padj_scatter"; 9 calls."""
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.argv, argv = [sys.argv[0], "none"], sys.argv
sys.path[:0] = [HERE, os.path.join(HERE, "..", "tests")]
from heterogeneity_compare_profile import cfg2_like, ea, kernel_ms, np, torch  # noqa: E402
import padjust_np as P  # noqa: E402

sys.argv = argv
HBM = 4.8e12                            # bytes per second the streaming kernels of this library reach


def fmt(ts, digits=2):
    return "%.*f ms [%.*f, %.*f]" % (digits, statistics.median(ts), digits, min(ts), digits, max(ts))


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t0) * 1e3


if __name__ == "__main__":
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    method = sys.argv[2] if len(sys.argv) > 2 else "BH"
    a, b = cfg2_like(rows, 5), cfg2_like(rows, 6)
    cx = lambda x: ea.generateCytosineReport(x, threshold_reads=False, report_context="CG", as_device=True)
    rep = ea.rcpp_cx_compare(cx(a), cx(b), 1, as_device=True)
    p = rep["p"]
    n = int(p.numel())
    p_host = p.cpu().numpy()
    passes = P.digit_passes(p_host)
    print("cfg2-like pair: 2 x %d rows; comparison table of %d rows; method %s" % (rows, n, method))
    print("  p: %d distinct values, %.1f %% exact 1.0, smallest %.3g; key bytes that differ (digit passes run): %d of 8"
          % (np.unique(p_host).size, 100.0 * np.mean(p_host == 1.0), p_host.min(), passes))
    device = lambda: ea.adjustPValues(p, method, as_device=True)
    sort = lambda: torch.sort(p, stable=True)
    calls = [("adjustPValues (device column in, device column out)", device), ("torch.sort(stable=True) of the column, keys + indices", sort)]
    times = {k: [] for k, _ in calls}
    for rnd in range(10):                                                     # the two device paths against each other, nothing in between
        for k, fn in (calls if rnd % 2 == 0 else calls[::-1]):
            r, ms = once(fn)
            if rnd:
                times[k].append(ms)
            if fn is device:
                q_dev = r
    for k, _ in calls:
        print("  %-58s%s" % (k, fmt(times[k])))
    fetch, restate = [], []
    for rnd in range(10):                                                     # the path before: the device idles while numpy sorts
        h, ms = once(lambda: p.cpu().numpy())
        t0 = time.perf_counter()
        q_host = P.adjust_np(h, method)[0]
        if rnd:
            fetch.append(ms)
            restate.append((time.perf_counter() - t0) * 1e3)
    print("  %-58s%s" % ("the path before: fetch of p (%d MB)" % (n * 8 // 10 ** 6), fmt(fetch)))
    print("  %-58s%s" % ("... numpy restatement on the host", fmt(restate)))
    same = np.array_equal(q_dev.cpu().numpy().view(np.uint64), q_host.view(np.uint64))
    print("  device q against the restatement, bit for bit over %d rows: %s" % (n, "equal" if same else "DIFFERENT"))
    assert same
    labels = ("padj_keys", "rsort_hist", "rsort_table_scan", "rsort_scatter", "padj_terms", "padj_dscan", "padj_scatter")
    for label in labels:
        print("  ... %-54s%s" % (label, kernel_ms(device, label, 9)))
    sys.stdout.flush()
    model = passes * 24.0 * n
    print("  traffic model of the sort: %d passes x 24 B x %d rows = %.2f GB = %.3f ms at %.1f TB/s" % (passes, n, model / 1e9, model / HBM * 1e3, HBM / 1e12))
    print("  bytes the passes move as built: 8 (histogram) + 12 + 12 (scatter) = 32 B per row and pass = %.2f GB = %.3f ms" %
          (passes * 32.0 * n / 1e9, passes * 32.0 * n / HBM * 1e3))
    for m2 in ("holm", "BY"):
        f = lambda: ea.adjustPValues(p, m2, as_device=True)
        f()
        ts = [once(f)[1] for _ in range(9)]
        print("  adjustPValues, %-43s%s" % (m2, fmt(ts)))
    # a column without ties: uniform random of the same length
    u = torch.rand(n, dtype=torch.float64, device=p.device)
    fu, su = (lambda: ea.adjustPValues(u, method, as_device=True)), (lambda: torch.sort(u, stable=True))
    tu = {0: [], 1: []}
    for rnd in range(10):
        for i in ((0, 1) if rnd % 2 == 0 else (1, 0)):
            _, ms = once((fu, su)[i])
            if rnd:
                tu[i].append(ms)
    print("  uniform random column of %d rows (%d passes): adjustPValues %s; torch.sort(stable=True) %s" % (n, P.digit_passes(u.cpu().numpy()), fmt(tu[0]), fmt(tu[1])))
    for label in ("padj_keys", "rsort_hist", "rsort_scatter"):
        print("  ... %-54s%s" % (label, kernel_ms(fu, label, 9)))
