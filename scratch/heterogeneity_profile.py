"""generateHeterogeneityReport timed on two workloads, next to generateMhlReport on the same batch -- the driver of
profiles/heterogeneity_report.txt.
    python scratch/heterogeneity_profile.py cfg2 [rows]   the synthetic batch of bench.py's cfg2 (uniform starts, L = 300)
    python scratch/heterogeneity_profile.py deep          10^6 rows of 250 bytes on 25 sites (summarise_patterns_profile's)
Each: the whole call (median [min, max] of the repeats) and the counting kernel alone (epi_prof "het_count"), k = 4, CG.
With EPIHIP_LIB=epialleler_amd/csrc/libepihip_thet.so (`make -C epialleler_amd/csrc timing-het`) the build whose
counting kernel adds once per lane."""
import ctypes as C
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import epialleler_amd as ea  # noqa: E402
from epialleler_amd import synth  # noqa: E402

lib = ea._lib.load()


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return r, "%.2f ms [%.2f, %.2f]" % (statistics.median(ts), min(ts), max(ts))


def kernel_ms(fn, label, reps):
    out = []
    for _ in range(reps):
        lib.epi_prof_reset(); lib.epi_prof_enable(1)
        try:
            fn()
        finally:
            lib.epi_prof_enable(0)
        ms, n = C.c_double(0), C.c_int64(0)
        lib.epi_prof_get(label.encode(), C.byref(ms), C.byref(n))
        out.append(ms.value)
    return "%.3f ms [%.3f, %.3f]" % (statistics.median(out), min(out), max(out))


def deep_bam(n=10 ** 6, npat=200, L=250, seed=1):
    rng = np.random.default_rng(seed)
    sites = np.sort(rng.choice(L, 25, replace=False))
    pats = np.full((npat, L), ord("."), np.uint8)
    seen = set()
    k = 0
    while k < npat:
        m = rng.integers(0, 2, size=25)
        if m.tobytes() in seen:
            continue
        seen.add(m.tobytes())
        pats[k, sites] = np.where(m == 1, ord("Z"), ord("z"))
        k += 1
    body = np.concatenate([np.zeros(int(n * 0.55), np.int64), rng.integers(1, npat, size=n - int(n * 0.55))])
    rng.shuffle(body)
    xm = pats[body].reshape(-1).astype(np.int64)
    packed = ((1 << 4) | (((xm + 2) >> 2) & 15)).astype(np.uint8)
    off = np.arange(n + 1, dtype=np.int64) * L
    return ea.ProcessedBam.from_arrays(packed, off, np.ones(n, np.int32), np.ones(n, np.int32), np.full(n, 1000, np.int32), levels=("chrA",))


def run(name, bam, reps):
    het = lambda: ea.generateHeterogeneityReport(bam, window_context="CG", window_sites=4, as_device=True)
    rep, t_het = timed(het, reps)
    k_het = kernel_ms(het, "het_count", reps)
    _, t_cx = timed(lambda: ea.generateCytosineReport(bam, threshold_reads=False, report_context="CG", as_device=True), reps)
    _, t_mhl = timed(lambda: ea.generateMhlReport(bam, as_device=True), reps)
    print(name)
    print("  rows %d, windows reported %d, deepest %d reads" % (bam.n, rep.nrow, int(rep["nreads"].max()) if rep.nrow else 0))
    print("  generateHeterogeneityReport(k=4)          %s" % t_het)
    print("  ... its counting kernel (het_count)       %s" % k_het)
    print("  generateCytosineReport(unthresholded, CG) %s" % t_cx)
    print("  generateMhlReport                         %s" % t_mhl)
    sys.stdout.flush()


mode = sys.argv[1]
print("library", os.path.basename(ea._lib.LIB_PATH))
if mode == "cfg2":
    rows = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
    bam = synth.generate_device_uniform(n_total=rows, mean_len=300, n_chr=4, seed=5, n=rows, ragged=False, gap_every=0)
    bam.batch()
    run("cfg2-like: %d rows of 300 bytes, uniform starts, depth 30" % rows, bam, 9)
elif mode == "deep":
    bam = deep_bam()
    bam.batch()
    run("deep target: 10^6 rows of 250 bytes on 25 CpGs, 200 XM strings, one on 55 % of the rows", bam, 9)
