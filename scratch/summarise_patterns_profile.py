"""summarisePatterns against extractPatternsBed followed by the plain group-by of tests/test_gpu_summarise_patterns.py
(summary_np): wall clock, kernel time from epi_prof and result bytes -- the driver of profiles/summarise_patterns.txt.
    python scratch/summarise_patterns_profile.py fixture        capture.bam x capture.bed, 565 targets
    python scratch/summarise_patterns_profile.py deep           one target of 10^6 synthetic rows (deep_bam below)
    python scratch/summarise_patterns_profile.py deep-insert    the deep target's insert kernel, five calls; with
        EPIHIP_LIB=epialleler_amd/csrc/libepihip_tpats.so (`make -C epialleler_amd/csrc timing-pats`) the build whose
        insert kernel adds once per lane"""
import ctypes as C
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import helpers as H  # noqa: E402
import test_gpu_summarise_patterns as TS  # noqa: E402
import epialleler_amd as ea  # noqa: E402

lib = ea._lib.load()
BAM = os.path.join(H.GOLDEN, "bam")


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return r, "%.2f ms [%.2f, %.2f]" % (statistics.median(ts), min(ts), max(ts))


def prof(fn, labels):
    lib.epi_prof_reset(); lib.epi_prof_enable(1)
    try:
        fn()
    finally:
        lib.epi_prof_enable(0)
    out = {}
    for lb in labels:
        ms, n = C.c_double(0), C.c_int64(0)
        lib.epi_prof_get(lb.encode(), C.byref(ms), C.byref(n))
        out[lb] = (ms.value, n.value)
    return out


def ncols(rep):
    return len(TS.position_columns(rep))


def compare(name, bam, bed, reps_old, reps_new, **kw):
    new, t_new = timed(lambda: ea.summarisePatterns(bam, bed, **kw), reps_new)
    old, t_old = timed(lambda: ea.extractPatternsBed(bam, bed, **kw), reps_old)
    sums, t_np = timed(lambda: [TS.summary_np(r) for r in old], reps_old)
    both, t_both = timed(lambda: [TS.summary_np(r) for r in ea.extractPatternsBed(bam, bed, **kw)], reps_old)
    for g, w in zip(new, old):
        TS.same_summary(g, w)
    p_new = prof(lambda: ea.summarisePatterns(bam, bed, **kw), ["extract_patterns_multi", "summarise_patterns", "summarise_patterns_insert"])
    p_old = prof(lambda: ea.extractPatternsBed(bam, bed, **kw), ["extract_patterns_multi"])
    b_old = sum(r.nrow * (32 + 4 * ncols(r)) for r in old)
    b_new = sum(r.nrow * (12 + 4 * ncols(r)) for r in new) + 12 * len(new)
    print(name)
    print("  targets %d, patterns %d, unique %d, largest count %d" % (len(new), sum(r.nrow for r in old), sum(r.nrow for r in new),
                                                                      max([int(r["count"].max()) for r in new if r] or [0])))
    print("  extractPatternsBed            %s" % t_old)
    print("  summary_np of its Reports     %s" % t_np)
    print("  extractPatternsBed+summary_np %s" % t_both)
    print("  summarisePatterns             %s" % t_new)
    print("  kernels, old route: extract_patterns_multi %.3f ms in %d sequences" % p_old["extract_patterns_multi"])
    print("  kernels, new route: extract_patterns_multi %.3f ms in %d sequences, summarise_patterns %.3f ms in %d (insert %.3f ms)"
          % (p_new["extract_patterns_multi"] + p_new["summarise_patterns"] + (p_new["summarise_patterns_insert"][0],)))
    print("  result bytes fetched: old route >= %d (32 B + 4 B per column per pattern), new route %d" % (b_old, b_new))
    print("  stats (groups, pairs, fallback targets): %s" % (TS.stats(ea, bam),))
    sys.stdout.flush()


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


mode = sys.argv[1]
print("library", os.path.basename(ea._lib.LIB_PATH))
if mode == "fixture":
    pb = ea.preprocessBam(os.path.join(BAM, "capture.bam"))
    pb.batch()
    compare("capture.bam x capture.bed (565 targets)", pb, ea.readBed(os.path.join(BAM, "capture.bed")), 9, 9)
elif mode == "deep":
    bam = deep_bam()
    bam.batch()
    compare("deep target: 10^6 rows of 250 bytes on chrA:1000-1249, 200 XM strings, one on 55 % of the rows", bam,
            ea.Bed(["chrA"], [1000], [1249]), 5, 9)
elif mode == "deep-insert":
    bam = deep_bam()
    bam.batch()
    bed = ea.Bed(["chrA"], [1000], [1249])
    ea.summarisePatterns(bam, bed)
    for _ in range(5):
        p = prof(lambda: ea.summarisePatterns(bam, bed), ["summarise_patterns", "summarise_patterns_insert"])
        print("  summarise_patterns %.3f ms, insert kernel %.3f ms" % (p["summarise_patterns"][0], p["summarise_patterns_insert"][0]))
