"""Differential run of the BAM reader: one library per process (EPIHIP_LIB selects it), one JSON of case -> SHA-256
of the result (or the error text) per run; two libraries behave alike where their JSON files are identical.

    EPIHIP_LIB=/path/to/parent/libepihip.so python scratch/bam_refactor_diff.py parent.json [--gpu]
    python scratch/bam_refactor_diff.py new.json [--gpu]
    cmp parent.json new.json

Without --gpu: preprocessBam over every golden BAM and the long-read cases crossed with the options, and over seeded
crafted files whose records carry random, partly malformed aux fields, CIGARs and lengths (tests/bam_craft.py).  With
--gpu, only the cases that need the device: the goldens and the crafted files through genome= and mates="anywhere", and
callMethylation's inflated output for the three strand tags."""
import gzip
import hashlib
import itertools
import json
import os
import random
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import epialleler_amd as ea  # noqa: E402
from bam_craft import crafted_files  # noqa: E402
from test_long_read import CASES, case_bam  # noqa: E402

BAMS = os.path.join(ROOT, "tests", "golden", "bam")
GOLDENS = sorted(f for f in os.listdir(BAMS) if f.endswith(".bam"))
RESULTS = {}


def digest(b):
    h = hashlib.sha256()
    for k in ("xm", "off", "rname", "strand", "start"):
        h.update(np.ascontiguousarray(np.asarray(b.host[k])).tobytes())
    h.update(repr((list(b.levels), b.nrecs, b.npushed, bool(b.paired), getattr(b, "ncalled", 0))).encode())
    return h.hexdigest()


def case(name, fn):
    try:
        RESULTS[name] = fn()
    except Exception as e:                                          # the message is part of the behaviour
        RESULTS[name] = "%s: %s" % (type(e).__name__, e)


def grid():
    for trim, bq, mq, dup, nt, win in itertools.product((0, 3, (2, 5)), (0, 20), (0, 30), (False, True), (1, 3, 16), (0, 1, 7)):
        yield dict(trim=trim, min_baseq=bq, min_mapq=mq, skip_duplicates=dup, nthreads=nt, window_kib=win)


# ---- the runs ------------------------------------------------------------------------------------------------------------

def cpu_cases(d):
    for name in GOLDENS:
        path = os.path.join(BAMS, name)
        for kw in grid():
            case("golden %s %r" % (name, sorted(kw.items())), lambda: digest(ea.preprocessBam(path, **kw)))
    for k, c in enumerate(CASES):
        path = case_bam(c, os.path.join(d, "lr_%d.bam" % k))
        for kw in grid():
            for mp, hp in ((-1, True), (128, True), (128, False), (250, False)):
                case("longread %d %r %d %d" % (k, sorted(kw.items()), mp, hp),
                     lambda: digest(ea.preprocessBam(path, min_prob=mp, highest_prob=hp, **kw)))
    for k, path in enumerate(crafted_files(d)):
        for kw in ({}, dict(nthreads=3, window_kib=1), dict(trim=(1, 2), min_baseq=41)):
            case("crafted %d %r" % (k, sorted(kw.items())), lambda: digest(ea.preprocessBam(path, **kw)))


def inflated_sha(path):
    with gzip.open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def gpu_cases(d):
    fasta = os.path.join(BAMS, "reference.fasta.gz")
    g = ea.preprocessGenome(fasta, verbose=False)
    opts = [{}, dict(nthreads=3, window_kib=1), dict(trim=(2, 5), min_baseq=20, min_mapq=30, nthreads=16, window_kib=7, skip_duplicates=True)]
    for name in GOLDENS:
        path = os.path.join(BAMS, name)
        for kw in opts:
            case("genome %s %r" % (name, sorted(kw.items())), lambda: digest(ea.preprocessBam(path, genome=g, **kw)))
            case("anywhere %s %r" % (name, sorted(kw.items())), lambda: digest(ea.preprocessBam(path, mates="anywhere", **kw)))
    for name in ("dragen-pe-namesort-xg.bam", "bwameth-pe-namesort-yd.bam", "bsmap-pe-namesort-zs.bam", "dragen-se-unsort-xg.bam",
                 "bwameth-se-unsort-yd.bam", "bsmap-se-unsort-zs.bam"):
        for win in (0, 64):
            out = os.path.join(d, "called.bam")

            def run():
                res = ea.callMethylation(os.path.join(BAMS, name), out, g, nthreads=3, verbose=False, window_kib=win)
                return [inflated_sha(out), sorted(res.items())]
            case("call %s %d" % (name, win), run)
    # the crafted files over a genome of their own: aux_find / aux_clean see the malformed fields
    rng = random.Random(1)
    fa = os.path.join(d, "chrS.fa")
    with open(fa, "w") as f:
        f.write(">chrS\n" + "".join(rng.choice("ACGT") for _ in range(100000)) + "\n")
    gs = ea.preprocessGenome(fa, verbose=False)
    for k, path in enumerate(crafted_files(d, 300)):
        case("crafted genome %d" % k, lambda: digest(ea.preprocessBam(path, genome=gs, window_kib=k % 2)))
        case("crafted anywhere %d" % k, lambda: digest(ea.preprocessBam(path, mates="anywhere")))
        out = os.path.join(d, "crafted_called.bam")
        case("crafted call %d" % k, lambda: [str(ea.callMethylation(path, out, gs, nthreads=2, verbose=False)), inflated_sha(out)])


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as d:
        (gpu_cases if "--gpu" in sys.argv[2:] else cpu_cases)(d)
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(RESULTS, f, indent=0, sort_keys=True)
    errors = sum(1 for v in RESULTS.values() if isinstance(v, str) and ": " in v)
    print("%d cases (%d of them errors) -> %s" % (len(RESULTS), errors, sys.argv[1]))
