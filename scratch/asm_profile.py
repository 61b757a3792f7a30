"""generateAsmReport's kernels on two shapes -- wall clock of rcpp_asm_report and kernel time from epi_prof: the driver of
profiles/asm_report.txt.
    python scratch/asm_profile.py capture   the capture fixture's SNVs (capture.vcf.gz inside capture.bed) under 10^6 synthetic
                                            rows of 150 bases, each laid over one of the SNVs, bases and calls at random
    python scratch/asm_profile.py pileup    10^5 rows of 150 bases on one SNV
Before anything is timed the tables are compared with the loop restatement (tests/asm_np.py): all of the pile-up, and for the
capture shape the first 3000 rows as a batch of their own; on the whole batch the SNV table must be the group-by of the pair
table."""
import ctypes as C
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import asm_np as A  # noqa: E402
import helpers as H  # noqa: E402
import epialleler_amd as ea  # noqa: E402

lib = ea._lib.load()
LABELS = ["asm_rows", "asm_count", "asm_emit", "asm_sort", "asm_reduce", "asm_snv", "asm_fetch"]
LETTERS = np.frombuffer(b"Zz.xh", np.uint8)
WEIGHTS = (0.04, 0.04, 0.86, 0.03, 0.03)


def rows_over(rng, n, length, chr_, pos):
    """n rows of `length` bases, each over one of the sites (its offset in the row uniform), sorted by (rname, start)"""
    k = rng.integers(0, len(pos), n)
    start = pos[k].astype(np.int64) - rng.integers(0, length, n)
    rname = chr_[k]
    order = np.lexsort((start, rname))
    xm = LETTERS[rng.choice(LETTERS.size, n * length, p=WEIGHTS)].astype(np.int64)
    nt16 = np.asarray([1, 2, 4, 8], np.int64)[rng.integers(0, 4, n * length)]
    packed = ((nt16 << 4) | (((xm + 2) >> 2) & 15)).astype(np.uint8)
    return {"xm": packed, "off": np.arange(n + 1, dtype=np.int64) * length, "rname": rname[order].astype(np.int32),
            "strand": rng.integers(1, 3, n).astype(np.int32), "start": start[order].astype(np.int32)}


def head(t, n):
    return {"xm": t["xm"][:t["off"][n]], "off": t["off"][:n + 1], "rname": t["rname"][:n], "strand": t["strand"][:n], "start": t["start"][:n]}


def bam_of(t):
    return ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"], levels=None)


def verify(t, sites, label):
    bam = bam_of(t)
    got = ea.rcpp_asm_report(bam, *sites, "Zz", 0, 1, 1.0)
    bam.close()
    t0 = time.perf_counter()
    want = A.restate(t, *sites, "Zz", max_oo=1.0)
    for g, w in zip(got, want):
        A.same(g, w, label)
    print("  %s: %d rows, %d pair rows equal to the restatement's (%.1f s on the host)" % (label, len(t["start"]), len(want[0]["snv"]), time.perf_counter() - t0))


def prof(fn):
    lib.epi_prof_reset(); lib.epi_prof_enable(1)
    try:
        fn()
    finally:
        lib.epi_prof_enable(0)
    out = {}
    for lb in LABELS:
        ms, n = C.c_double(0), C.c_int64(0)
        lib.epi_prof_get(lb.encode(), C.byref(ms), C.byref(n))
        out[lb] = (ms.value, n.value)
    return out


def measure(name, t, sites):
    bam = bam_of(t)
    bam.batch()
    call = lambda: ea.rcpp_asm_report(bam, *sites, "Zz", 0, 1, 1.0, as_device=True)
    pairs, snvs = ea.rcpp_asm_report(bam, *sites, "Zz", 0, 1, 1.0)
    for k in A.CELLS:
        assert np.array_equal(np.bincount(pairs["snv"], pairs[k], len(sites[0])), snvs[k]), k
    call()
    ts = []
    for _ in range(7):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    print(name)
    print("  rows %d, bytes %d, sites %d, pair rows %d, reads with an allele %d, without %d, events in reported rows %d"
          % (len(t["start"]), t["xm"].size, len(sites[0]), len(pairs["snv"]), int(snvs["reads_ref"].sum() + snvs["reads_alt"].sum()),
             int(snvs["reads_other"].sum()), int(sum(pairs[k].sum() for k in A.CELLS))))
    print("  rcpp_asm_report(as_device=True)   %.2f ms [%.2f, %.2f]  (median [min, max] of 7 after a warm-up call)" % (statistics.median(ts), min(ts), max(ts)))
    for rep in range(3):
        p = prof(call)
        print("  kernels, call %d: " % rep + ", ".join("%s %.3f ms (%d)" % (lb, p[lb][0], p[lb][1]) for lb in LABELS))
    bam.close()
    sys.stdout.flush()


mode = sys.argv[1]
print("library", os.path.basename(ea._lib.LIB_PATH))
rng = np.random.default_rng(1)
if mode == "capture":
    import test_asm_host as HOST
    _, sites, v = HOST.fixture_sites("capture")
    sites = tuple(np.ascontiguousarray(a, np.int32) for a in sites)
    t = rows_over(rng, 10 ** 6, 150, sites[0], sites[1])
    verify(head(t, 3000), sites, "the first 3000 rows")
    measure("capture SNVs: %d sites of capture.vcf.gz under 10^6 synthetic rows of 150 bases" % len(v), t, sites)
elif mode == "pileup":
    sites = (np.asarray([1], np.int32), np.asarray([5000], np.int32), np.asarray([A.mask_of("A", "G") | A.mask_of("A", "T")], np.int32))
    t = rows_over(rng, 10 ** 5, 150, sites[0], sites[1])
    verify(t, sites, "all rows")
    measure("pile-up: 10^5 rows of 150 bases on one SNV (REF A, ALT G or T)", t, sites)
