"""preprocessBam(genome=) against the two-step route on call_profile.py's input (1 M PE150 bwa-meth records):

  (a) callMethylation(in.bam, called.bam, G) then preprocessBam(called.bam)
  (b) preprocessBam(in.bam, genome=G)

  python scratch/call_profile.py make DIR                        # writes DIR/genome.fa, DIR/in.bam
  EPIHIP_BAM_TIMING=1 python scratch/preprocess_genome_profile.py DIR NTHREADS [ROUNDS]

One warm-up of each, then ROUNDS alternations (a, b); prints one JSON line with the wall times and whether the
templates of (a) and (b) are byte-identical in every round.  The phase split goes to stderr (EPIHIP_BAM_TIMING=1).
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def same(a, b):
    return (a.n, a.nbytes, a.nrecs, a.paired, a.levels) == (b.n, b.nbytes, b.nrecs, b.paired, b.levels) and \
        all(np.array_equal(a.host[k], b.host[k]) for k in ("xm", "off", "rname", "strand", "start"))


def main(d, nthreads, rounds):
    import epialleler_amd as ea
    g = ea.preprocessGenome(os.path.join(d, "genome.fa"), nthreads=nthreads, verbose=False)
    src, called = os.path.join(d, "in.bam"), os.path.join(d, "called_%d.bam" % nthreads)

    def two_step():
        ea.callMethylation(src, called, g, nthreads=nthreads, verbose=False)
        return ea.preprocessBam(called, nthreads=nthreads)

    def direct():
        return ea.preprocessBam(src, genome=g, nthreads=nthreads)

    two_step(); direct()                                               # warm-up (genome upload, allocations)
    ta, tb, equal = [], [], []
    for _ in range(rounds):
        sys.stderr.write("-- (a) two-step, %d threads\n" % nthreads)
        t0 = time.perf_counter(); pa = two_step(); ta.append(time.perf_counter() - t0)
        sys.stderr.write("-- (b) direct, %d threads\n" % nthreads)
        t0 = time.perf_counter(); pb = direct(); tb.append(time.perf_counter() - t0)
        equal.append(bool(same(pa, pb)) and pb.ncalled == pa.nrecs)
        del pa, pb
    os.unlink(called)
    print(json.dumps({"nthreads": nthreads, "a_two_step_s": [round(t, 4) for t in ta],
                      "b_direct_s": [round(t, 4) for t in tb], "equal": equal}))
    return 0 if all(equal) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 3))
