"""generateFdrpReport timed on the two workloads of heterogeneity_profile.py, next to generateHeterogeneityReport on the
same batch in the same process -- the driver of profiles/fdrp_report.txt.
    python scratch/fdrp_profile.py cfg2 [rows]   the synthetic batch of bench.py's cfg2 (uniform starts, L = 300)
    python scratch/fdrp_profile.py deep          10^6 rows of 250 bytes on 25 sites
Each: the whole call (median [min, max] of 9 repeats after one untimed call, stream synchronised, as_device) and every
kernel of the call from HIP events around its launches (epi_prof; the sort's three kernels carry radix_sort.hip's labels and
are summed over the passes), CG, the defaults (flank_sites 8, max_reads 40) and flank_sites 0 and 31, max_reads 64."""
import ctypes as C
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.argv, argv = [sys.argv[0], "none"], sys.argv           # (heterogeneity_profile runs a mode when imported with one; it prints the library's name)
sys.path[:0] = [HERE]
from heterogeneity_profile import deep_bam, ea, kernel_ms, lib, synth, timed  # noqa: E402

sys.argv = argv
LABELS = ("fdrp_mark", "fdrp_fill", "rsort_hist", "rsort_table_scan", "rsort_scatter", "fdrp_bounds", "fdrp_pairs", "fdrp_emit")


def kernels_ms(fn, reps):
    """median [min, max] per label, every label from the same `reps` profiled calls"""
    seen = {q: [] for q in LABELS}
    for _ in range(reps):
        lib.epi_prof_reset(); lib.epi_prof_enable(1)
        try:
            fn()
        finally:
            lib.epi_prof_enable(0)
        for q in LABELS:
            ms, n = C.c_double(0), C.c_int64(0)
            lib.epi_prof_get(q.encode(), C.byref(ms), C.byref(n))
            seen[q].append((ms.value, n.value))
    return {q: "%.3f ms [%.3f, %.3f] in %d launches" % (statistics.median(v[0] for v in seen[q]), min(v[0] for v in seen[q]),
                                                        max(v[0] for v in seen[q]), seen[q][0][1]) for q in LABELS}


def run(name, bam, reps=9):
    print(name)
    het = lambda: ea.generateHeterogeneityReport(bam, window_context="CG", window_sites=4, as_device=True)
    rep, t_het = timed(het, reps)
    print("  rows %d, windows of four sites reported %d" % (bam.n, rep.nrow))
    print("  generateHeterogeneityReport(k=4)            %s" % t_het)
    print("  ... its counting kernel (het_count)         %s" % kernel_ms(het, "het_count", reps))
    del rep
    _, t_cx = timed(lambda: ea.generateCytosineReport(bam, threshold_reads=False, report_context="CG", as_device=True), reps)
    print("  generateCytosineReport(unthresholded, CG)   %s" % t_cx)
    for W, m in ((8, 40), (0, 64), (31, 64)):
        fdrp = lambda: ea.generateFdrpReport(bam, fdrp_context="CG", flank_sites=W, max_reads=m, as_device=True)
        rep, t_fdrp = timed(fdrp, reps)
        print("  generateFdrpReport(flank_sites=%d, max_reads=%d)  %s   %d sites reported, deepest %d reads, %d pairs compared"
              % (W, m, t_fdrp, rep.nrow, int(rep["coverage"].max()) if rep.nrow else 0, int(rep["npairs"].sum()) if rep.nrow else 0))
        for q, v in kernels_ms(fdrp, reps).items():
            print("  ... %-18s %s" % (q, v))
        del rep
        sys.stdout.flush()


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "cfg2":
        rows = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
        bam = synth.generate_device_uniform(n_total=rows, mean_len=300, n_chr=4, seed=5, n=rows, ragged=False, gap_every=0)
        bam.batch()
        run("cfg2-like: %d rows of 300 bytes, uniform starts, depth 30" % rows, bam)
    else:
        bam = deep_bam()
        bam.batch()
        run("deep target: 10^6 rows of 250 bytes on 25 CpGs, 200 XM strings, one on 55 % of the rows", bam)
