"""generateLinkageReport timed on the two workloads of heterogeneity_profile.py, next to
generateHeterogeneityReport(window_sites=2) on the same batch -- the driver of profiles/linkage_report.txt.
    python scratch/linkage_profile.py cfg2 [rows]   the synthetic batch of bench.py's cfg2 (uniform starts, L = 300)
    python scratch/linkage_profile.py deep          10^6 rows of 250 bytes on 25 sites
Each: the whole call (median [min, max] of 9 repeats after one untimed call, stream synchronised, as_device) and the
counting kernel alone (epi_prof "link_count" / "het_count"), CG, max_neighbours 1, 4 and 16; and generateHaplotypeBlocks
(max_neighbours 4) for the blocks on top of the pair table."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.argv, argv = [sys.argv[0], "none"], sys.argv           # (heterogeneity_profile runs a mode when imported with one; it prints the library's name)
sys.path[:0] = [HERE]
from heterogeneity_profile import deep_bam, ea, kernel_ms, synth, timed  # noqa: E402

sys.argv = argv


def run(name, bam, reps=9):
    print(name)
    het = lambda: ea.generateHeterogeneityReport(bam, window_context="CG", window_sites=2, as_device=True)
    rep, t_het = timed(het, reps)
    print("  rows %d, windows of two sites reported %d" % (bam.n, rep.nrow))
    print("  generateHeterogeneityReport(k=2)            %s" % t_het)
    print("  ... its counting kernel (het_count)         %s" % kernel_ms(het, "het_count", reps))
    del rep
    for D in (1, 4, 16):
        link = lambda: ea.generateLinkageReport(bam, linkage_context="CG", max_neighbours=D, as_device=True)
        rep, t_link = timed(link, reps)
        print("  generateLinkageReport(max_neighbours=%-2d)    %s   %d pairs reported" % (D, t_link, rep.nrow))
        print("  ... its counting kernel (link_count)        %s" % kernel_ms(link, "link_count", reps))
        del rep
    blocks = lambda: ea.generateHaplotypeBlocks(bam, linkage_context="CG", max_neighbours=4, as_device=True)
    rep, t_blocks = timed(blocks, reps)
    print("  generateHaplotypeBlocks(max_neighbours=4)   %s   %d blocks" % (t_blocks, rep.nrow))
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
