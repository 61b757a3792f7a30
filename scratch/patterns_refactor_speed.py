"""Wall-clock times of pattern extraction for one library (EPIHIP_LIB selects it), batches resident, BED parsed once:
a Python loop of extractPatterns, extractPatternsBed and summarisePatterns over the 565 rows of capture.bed, and the same
three over 100 random 500-bp targets on a synthetic batch of 10^7 rows of 300 bytes (profiles/extract_patterns_bed.txt).

    [EPIHIP_LIB=/path/to/other/libepihip.so] python scratch/patterns_refactor_speed.py run out.json     # one process
    python scratch/patterns_refactor_speed.py table parent_*.json -- new_*.json                           # median [min, max]

Run the two libraries in alternating processes; `table` takes every process's median of 7 repeats and prints, per
measurement, the median, minimum and maximum over the processes of each side."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPEATS = 7


def timed(fn):
    import torch
    fn()                                                            # warm: code objects, allocator
    out = []
    for _ in range(REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()                                                        # every entry point synchronises its stream before it returns
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def run(path):
    import numpy as np
    import torch
    import epialleler_amd as ea
    from epialleler_amd import synth
    res = {}
    pb = ea.preprocessBam(os.path.join(ROOT, "tests", "golden", "bam", "capture.bam"))
    bed = ea.readBed(os.path.join(ROOT, "tests", "golden", "bam", "capture.bed"))
    pb.batch()
    res["fixture loop"] = timed(lambda: [ea.extractPatterns(pb, bed, bed_row=r) for r in range(1, 566)])
    res["fixture bed"] = timed(lambda: ea.extractPatternsBed(pb, bed))
    res["fixture summary"] = timed(lambda: ea.summarisePatterns(pb, bed))
    n = 10 ** 7
    bam = synth.generate_device(n, read_len=300, n_chr=4, depth=30, seed=5)
    try:
        bam.batch()
        rows = torch.as_tensor(np.sort(np.random.default_rng(23).integers(0, n, size=100)), device=bam.dev["start"].device)
        rn, st = bam.dev["rname"][rows].cpu().numpy(), bam.dev["start"][rows].cpu().numpy()
        targets = [(int(r), int(s), int(s) + 499) for r, s in zip(rn, st)]
        res["1e7 loop"] = timed(lambda: [ea.rcpp_extract_patterns(bam, *tg, 1, "Zz", 0.01, False, 1) for tg in targets])
        res["1e7 bed"] = timed(lambda: ea.rcpp_extract_patterns_multi(bam, targets, 1, "Zz", 0.01, False, 1))
        res["1e7 summary"] = timed(lambda: ea.rcpp_summarise_patterns_multi(bam, targets, 1, "Zz", 0.01, False, 1))
    finally:
        bam.close()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f)
    print(os.environ.get("EPIHIP_LIB", "(the tree's library)"), " ".join("%s %.2f" % kv for kv in res.items()))


def table(args):
    sides = [args[:args.index("--")], args[args.index("--") + 1:]]
    runs = [[json.load(open(p)) for p in side] for side in sides]
    for key in runs[0][0]:
        cells = []
        for side in runs:
            v = [r[key] for r in side]
            cells.append("%9.2f ms [%.2f, %.2f]" % (statistics.median(v), min(v), max(v)))
        print("  %-16s parent %s   new %s   (%d + %d processes)" % (key, cells[0], cells[1], len(runs[0]), len(runs[1])))


if __name__ == "__main__":
    run(sys.argv[2]) if sys.argv[1] == "run" else table(sys.argv[2:])
