"""smoothCytosineReport's kernels on a destranded genome's worth of CpGs in one process -- kernel time of the sort, the bounds
and the fit from epi_prof (prof_begin / prof_end: device events around each step), median and range of the repeats after a
warm-up: the driver of profiles/smooth_report.txt.
    python scratch/smooth_profile.py [n_sites] [repeats]      default 28 000 000 sites, 7 repeats
The table: n_sites CpGs over 24 rnames, geometric gaps of mean 100, Poisson(5) coverage, strand '+' (seeded; made on the
device).  Timed at the defaults (bandwidth 1000, min_sites 70, degree 2) and at min_sites = 500.
With EPIHIP_LIB=epialleler_amd/csrc/libepihip_tsmooth.so (`make -C epialleler_amd/csrc timing-smooth`) the fit kernel reads
its windows from global memory only; everything else is the same in both libraries.  Before anything is timed the first and
the last 3000 rows of two rnames are compared with the restatement (tests/smooth_np.py) as tables of their own, and a
checksum of the whole result's bits is printed, so that the two libraries' runs can be held against each other.
Operations: the fit performs 23 fp64 operations per window visit as include/epihip.h writes them (1 division, 11
multiplications, 11 additions / subtractions); visits = the sum of the nsites column.  The share of peak is visits * 23
over the fit kernel's time over the fp64 vector peak of 78.6 TFLOP/s -- a division counted as one operation although the
hardware spends about ten instructions on it, so the share understates how busy the vector units are."""
import ctypes as C
import math
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import smooth_np as S  # noqa: E402
import epialleler_amd as ea  # noqa: E402

lib = ea._lib.load()
FP64_PEAK = 78.6e12
OPS_PER_VISIT = 23
N_RNAME = 24
LABELS = ("smooth_sort", "smooth_bounds", "smooth_fit")


def make_table(n, seed=42):
    g = torch.Generator(device="cuda").manual_seed(seed)
    per = (n + N_RNAME - 1) // N_RNAME
    u = torch.rand(n, generator=g, device="cuda", dtype=torch.float64)
    gaps = (torch.log1p(-u) / np.log1p(-0.01)).floor().to(torch.int64) + 1          # geometric, mean 100
    rname = (torch.arange(n, device="cuda") // per).to(torch.int32) + 1
    pos = torch.cumsum(gaps, 0)
    first = torch.arange(n, device="cuda") // per * per
    pos = (pos - pos[first] + gaps[first]).to(torch.int32)                           # restart per rname
    cdf = np.cumsum([math.exp(-5.0 + k * math.log(5.0) - math.lgamma(k + 1.0)) for k in range(60)])     # Poisson(5) by inversion
    cov = torch.searchsorted(torch.from_numpy(cdf).cuda(), torch.rand(n, generator=g, device="cuda", dtype=torch.float64)).to(torch.int32)
    beta = torch.rand(n, generator=g, device="cuda", dtype=torch.float64)
    meth = torch.minimum((beta * (cov + 1).double()).floor().to(torch.int32), cov)                       # uniform on 0 .. cov
    cols = dict(rname=rname, strand=torch.ones(n, dtype=torch.int32, device="cuda"), pos=pos,
                context=torch.full((n,), S.CG, dtype=torch.int32, device="cuda"), meth=meth, unmeth=cov - meth)
    return ea.Report(cols, ["chr%d" % (k + 1) for k in range(N_RNAME)])


def prof_run(fn):
    lib.epi_prof_reset(); lib.epi_prof_enable(1)
    try:
        fn()
    finally:
        lib.epi_prof_enable(0)
    out = {}
    for label in LABELS:
        ms, k = C.c_double(0), C.c_int64(0)
        lib.epi_prof_get(label.encode(), C.byref(ms), C.byref(k))
        out[label] = ms.value
    return out


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 28_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    rep = make_table(n)
    per = (n + N_RNAME - 1) // N_RNAME
    print("library %s; %d sites over %d rnames, mean gap %.1f, mean coverage %.2f, checksum of the table %016x" % (
        os.path.basename(ea._lib.LIB_PATH), n, N_RNAME, float(rep["pos"][per - 1]) / per, float((rep["meth"] + rep["unmeth"]).double().mean()),
        sum(int((v.to(torch.int64) * (k + 1)).sum()) for k, v in enumerate(rep.values())) & (2 ** 64 - 1)))
    # correctness first
    for a in (0, per - 3000, n - 3000):
        a = max(a, 0)
        sub = {k: v[a:a + 3000].cpu().numpy() for k, v in rep.items()}
        for kw in (dict(), dict(min_sites=500)):
            got = ea.rcpp_cx_smooth(ea.Report({k: torch.from_numpy(v).cuda() for k, v in sub.items()}, rep.levels["rname"]), **kw)
            S.same(got, S.smooth_np(sub, **kw), "rows %d.." % a)
    print("  equal to the restatement, bit for bit, on 3 windows of 3000 rows at min_sites 70 and 500")
    for min_sites in (70, 500):
        run = lambda: ea.rcpp_cx_smooth(rep, min_sites=min_sites, as_device=True)
        out = run()                                                      # warm-up
        visits = int(out["nsites"].sum(dtype=torch.int64))
        bits = int(out["smoothed"].view(torch.int64).sum()) & (2 ** 64 - 1)
        print("  min_sites %d: %d clusters, largest window %d, %d window visits (%.1f per site), degree used %s, checksum of smoothed %016x"
              % (min_sites, out.ncluster, out.max_window, visits, visits / n, torch.bincount(out["degree"] + 1, minlength=4).tolist(), bits))
        del out
        ts = [prof_run(run) for _ in range(reps)]
        for label in LABELS:
            v = [t[label] for t in ts]
            line = "    %-14s %9.3f ms [%.3f, %.3f]" % (label, statistics.median(v), min(v), max(v))
            if label == "smooth_fit":
                med = statistics.median(v) * 1e-3
                line += "   %.2f G visits/s, %.2f TFLOP/s fp64 as written = %.1f %% of the %.1f TFLOP/s vector peak" % (
                    visits / med / 1e9, visits * OPS_PER_VISIT / med / 1e12, 100 * visits * OPS_PER_VISIT / med / FP64_PEAK, FP64_PEAK / 1e12)
            print(line)
    sys.stdout.flush()


main()
