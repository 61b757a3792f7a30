"""generateRegionReport against the route users had before it: summarisePatterns on the same batch and BED, then a Python loop
that derives the same columns from its unique patterns and counts -- wall clock, kernel time from epi_prof and launches:
the driver of profiles/region_report.txt.
    python scratch/region_profile.py fixture       capture.bam x capture.bed, 565 regions
    python scratch/region_profile.py deep          one region of 10^6 synthetic rows (the deep target of
                                                   scratch/summarise_patterns_profile.py, built the same way)
    python scratch/region_profile.py deep-count    the deep target's counting kernel, five calls; with
        EPIHIP_LIB=epialleler_amd/csrc/libepihip_trgn.so (`make -C epialleler_amd/csrc timing-rgn`) the build whose
        counting kernel adds to global memory once per row
The old route has no read rule, so both run with it off (max_outofcontext_beta = 1); every table is compared with the
restatement (tests/region_np.py) and with the old route's before anything is timed."""
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
import region_np as RN  # noqa: E402
import epialleler_amd as ea  # noqa: E402

lib = ea._lib.load()
BAM = os.path.join(H.GOLDEN, "bam")
KW = dict(min_sites=4, max_sites=64, uxm_thresholds=(0.25, 0.75))
LABELS = ["region_report", "region_count", "extract_patterns_multi", "summarise_patterns"]


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return r, "%.2f ms [%.2f, %.2f]" % (statistics.median(ts), min(ts), max(ts))


def prof(fn, labels=LABELS):
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


def derive(summaries, regions):
    """The region report's columns from summarisePatterns' Reports (clip_patterns=False, min_context_freq=0): per region the
    position columns inside it, per unique pattern its calls in position order, weighted by the pattern's count"""
    chrom, rs, re_ = regions
    out = {k: np.zeros(len(summaries), np.int32) for k in RN.INT_COLS}
    out.update({k: np.full(len(summaries), np.nan) for k in RN.FLOAT_COLS})
    for g, rep in enumerate(summaries):
        rows, counts = [], []
        if rep:
            pos = sorted(int(k) for k in rep if k.lstrip("-").isdigit() and rs[g] <= int(k) <= re_[g])
            if pos:
                cells = np.stack([np.asarray(rep[str(p)]) for p in pos], axis=1)
                rows = [[bool(c < 8) for c in row[row != H.NA_INT]] for row in cells]
                counts = np.asarray(rep["count"]).tolist()
        c, d, _ = RN.region_row(rows, KW["min_sites"], KW["max_sites"], *KW["uxm_thresholds"], weights=counts)
        out["rname"][g], out["start"][g], out["end"][g] = chrom[g], rs[g], re_[g]
        for k, v in list(c.items()) + list(d.items()):
            out[k][g] = v
    return out


def compare(name, bam, bed, t, reps_old):
    regions = RN.bed_regions(bam.levels, bed.chrom, bed.start, bed.end)
    new = lambda: ea.generateRegionReport(bam, bed, max_outofcontext_beta=1.0, **KW)
    old_gpu = lambda: ea.summarisePatterns(bam, bed, clip_patterns=False, min_context_freq=0, strand_offset=1)
    old = lambda: derive(old_gpu(), regions)
    got = new()
    t0 = time.perf_counter()
    RN.same(got, RN.restate(t, regions, "Zz", max_oo=1.0, min_sites=KW["min_sites"], max_sites=KW["max_sites"]), "restatement")
    t_restate = time.perf_counter() - t0
    # (a reverse-strand row that starts one base behind a region's end has a call inside it and is no pattern row of it)
    behind = np.asarray([np.any((t["rname"] == regions[0][g]) & (t["strand"] == 2) & (t["start"] == regions[2][g] + 1)) for g in range(len(bed))])
    theirs = old()
    sel = np.flatnonzero(~behind)
    RN.same({k: np.asarray(got[k])[sel] for k in RN.COLUMNS}, {k: theirs[k][sel] for k in RN.COLUMNS}, "old route")
    _, t_new = timed(new, 9)
    _, t_old_gpu = timed(old_gpu, reps_old)
    _, t_old = timed(old, reps_old)
    p_new, p_old = prof(new), prof(old_gpu)
    print(name)
    print("  regions %d (compared with the old route: %d), rows on them %d, k-reads %d, largest n %d; restatement %.1f s"
          % (len(bed), sel.size, int(got["nreads"].sum()), int(got["kreads"].sum()), int(got["maxsites"].max()), t_restate))
    print("  summarisePatterns                 %s" % t_old_gpu)
    print("  summarisePatterns + Python loop   %s" % t_old)
    print("  generateRegionReport              %s" % t_new)
    print("  kernels, old route: extract_patterns_multi %.3f ms in %d sequences, summarise_patterns %.3f ms in %d"
          % (p_old["extract_patterns_multi"] + p_old["summarise_patterns"]))
    print("  kernels, new route: region_report %.3f ms in %d sequences (its counting kernel %.3f ms in %d)" % (p_new["region_report"] + p_new["region_count"]))
    sys.stdout.flush()


def deep_bam(n=10 ** 6, npat=200, L=250, seed=1):
    """The deep target of scratch/summarise_patterns_profile.py -> (batch, templates)"""
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
    t = {"xm": packed, "off": off, "rname": np.ones(n, np.int32), "strand": np.ones(n, np.int32), "start": np.full(n, 1000, np.int32)}
    return ea.ProcessedBam.from_arrays(packed, off, t["rname"], t["strand"], t["start"], levels=("chrA",)), t


mode = sys.argv[1]
print("library", os.path.basename(ea._lib.LIB_PATH))
if mode == "fixture":
    pb = ea.preprocessBam(os.path.join(BAM, "capture.bam"))
    pb.batch()
    compare("capture.bam x capture.bed (2968 rows, 565 regions)", pb, ea.readBed(os.path.join(BAM, "capture.bed")), pb.host, 9)
elif mode == "deep":
    bam, t = deep_bam()
    bam.batch()
    compare("deep target: 10^6 rows of 250 bytes on chrA:1000-1249, 200 XM strings over 25 CpG sites, one on 55 % of the rows", bam,
            ea.Bed(["chrA"], [1000], [1249]), t, 9)
elif mode == "deep-count":
    bam, t = deep_bam()
    bam.batch()
    bed = ea.Bed(["chrA"], [1000], [1249])
    first = ea.generateRegionReport(bam, bed, max_outofcontext_beta=1.0, **KW)
    print("  " + ", ".join("%s %s" % (k, first[k][0]) for k in RN.COLUMNS[3:]))
    for _ in range(5):
        p = prof(lambda: ea.generateRegionReport(bam, bed, max_outofcontext_beta=1.0, **KW))
        print("  region_report %.3f ms, counting kernel %.3f ms" % (p["region_report"][0], p["region_count"][0]))
