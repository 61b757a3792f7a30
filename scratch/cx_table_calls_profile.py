"""The stateless CX-table calls in one process, one library (EPIHIP_LIB picks it): wall clock of the whole Python call with the
device synchronised (as_device: nothing copied to the host) and kernel time from epi_prof (device events around each step), the
median of the repeats after a warm-up call of each: the driver of profiles/cx_table_calls.txt, which holds two libraries'
processes against each other.
    python scratch/cx_table_calls_profile.py [repeats] [out.json]      default 5 repeats
Tables, made on the device (seeded): 28 000 000 '+' CpGs over 24 rnames, geometric gaps of mean 100, Poisson(5) coverage
(scratch/smooth_profile.py's) for merge, smooth and segment (K = 3, one decode); its first 7 000 000 rows with two sets of
counts for the join and the regions, and the join's p column for the adjustment (BH); its first 1 000 000 rows with eight
sets of counts for the group comparison (4 + 4, lrt).  A checksum of every result is printed so that two libraries' runs can
be held against each other."""
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import segment_np as G  # noqa: E402
import smooth_np as S  # noqa: E402
import epialleler_amd as ea  # noqa: E402

lib = ea._lib.load()
N_RNAME = 24
LEVELS = ["chr%d" % (k + 1) for k in range(N_RNAME)]
POISSON5 = np.cumsum([math.exp(-5.0 + k * math.log(5.0) - math.lgamma(k + 1.0)) for k in range(60)])


def counts(n, g):
    cov = torch.searchsorted(torch.from_numpy(POISSON5).cuda(), torch.rand(n, generator=g, device="cuda", dtype=torch.float64)).to(torch.int32)
    beta = torch.rand(n, generator=g, device="cuda", dtype=torch.float64)
    meth = torch.minimum((beta * (cov + 1).double()).floor().to(torch.int32), cov)
    return meth, cov - meth


def make_keys(n, g):
    per = (n + N_RNAME - 1) // N_RNAME
    u = torch.rand(n, generator=g, device="cuda", dtype=torch.float64)
    gaps = (torch.log1p(-u) / np.log1p(-0.01)).floor().to(torch.int64) + 1
    rname = (torch.arange(n, device="cuda") // per).to(torch.int32) + 1
    pos = torch.cumsum(gaps, 0)
    first = torch.arange(n, device="cuda") // per * per
    pos = (pos - pos[first] + gaps[first]).to(torch.int32)
    return dict(rname=rname, strand=torch.ones(n, dtype=torch.int32, device="cuda"), pos=pos,
                context=torch.full((n,), S.CG, dtype=torch.int32, device="cuda"))


def table(keys, n, g):
    meth, unmeth = counts(n, g)
    return ea.Report(dict({k: v[:n].contiguous() for k, v in keys.items()}, meth=meth, unmeth=unmeth), LEVELS)


def checksum(cols):
    """the sum of the columns' bits (a Report, or one tensor)"""
    total = 0
    for v in ([cols] if isinstance(cols, torch.Tensor) else cols.values()):
        total += int((v.view(torch.int64) if v.dtype == torch.float64 else v.to(torch.int64)).sum())
    return total & (2 ** 64 - 1)


def prof_ms(fn, labels):
    lib.epi_prof_reset(); lib.epi_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        lib.epi_prof_enable(0)
    total = 0.0
    for label in labels:
        ms, k = C.c_double(0), C.c_int64(0)
        lib.epi_prof_get(label.encode(), C.byref(ms), C.byref(k))
        total += ms.value
    return total


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    del out
    return (t1 - t0) * 1e3


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    g = torch.Generator(device="cuda").manual_seed(42)
    n = 28_000_000
    keys = make_keys(n, g)
    big = table(keys, n, g)
    a, b = table(keys, 7_000_000, g), table(keys, 7_000_000, g)
    group = [table(keys, 1_000_000, g) for _ in range(8)]
    cmp_tab = ea.rcpp_cx_compare(a, b, as_device=True)
    model = G.start_model((0.1, 0.5, 0.9), 0.9)
    calls = [
        ("rcpp_cx_compare", lambda: ea.rcpp_cx_compare(a, b, as_device=True), ("cxcmp_match", "cxcmp_emit", "fisher_exact")),
        ("rcpp_cx_compare_regions", lambda: ea.rcpp_cx_compare_regions(cmp_tab, as_device=True), ("cxcmp_region_flag", "cxcmp_region_emit")),
        ("rcpp_cx_compare_groups", lambda: ea.rcpp_cx_compare_groups(group[:4], group[4:], as_device=True), ("cxg_key", "cxg_sort", "cxg_flag", "cxg_emit")),
        ("rcpp_cx_merge_strands", lambda: ea.rcpp_cx_merge_strands(big, as_device=True), ("cxmerge_flag", "cxmerge_emit")),
        ("rcpp_cx_smooth", lambda: ea.rcpp_cx_smooth(big, as_device=True), ("smooth_sort", "smooth_bounds", "smooth_fit")),
        ("rcpp_cx_segment", lambda: ea.rcpp_cx_segment(big, *model, max_iter=1, as_device=True),
         ("segment_sort", "segment_gather", "segment_fwd_agg", "segment_fwd_carry", "segment_fwd_walk", "segment_bwd_agg", "segment_bwd_carry",
          "segment_bwd_walk", "segment_runs", "segment_emit")),
        ("adjustPValues", lambda: ea.adjustPValues(cmp_tab["p"], as_device=True), ("padj_keys", "rsort_hist", "rsort_table_scan", "rsort_scatter",
                                                                                   "padj_terms", "padj_dscan", "padj_scatter")),
    ]
    result = {"library": ea._lib.LIB_PATH}
    for name, fn, labels in calls:
        out = fn()                                                      # warm-up
        torch.cuda.synchronize()
        sums = [checksum(out)]
        if hasattr(out, "segments"):
            sums.append(checksum(out.segments))
        del out
        wall = [wall_ms(fn) for _ in range(reps)]
        kern = [prof_ms(fn, labels) for _ in range(reps)]
        result[name] = {"wall_ms": statistics.median(wall), "kernel_ms": statistics.median(kern), "checksum": ["%016x" % s for s in sums]}
        print("%-26s wall %9.3f ms [%.3f, %.3f]   kernels %9.3f ms [%.3f, %.3f]   %s" % (
            name, statistics.median(wall), min(wall), max(wall), statistics.median(kern), min(kern), max(kern), result[name]["checksum"]))
    sys.stdout.flush()
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(result, f)


main()
