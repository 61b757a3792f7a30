"""Differential run of the BAM reader: one library per process (EPIHIP_LIB selects it), one JSON of case -> SHA-256
of the result (or the error text) per run; two libraries behave alike where their JSON files are identical.

    EPIHIP_LIB=/path/to/parent/libepihip.so python scratch/bam_refactor_diff.py parent.json [--gpu]
    python scratch/bam_refactor_diff.py new.json [--gpu]
    cmp parent.json new.json

Without --gpu: preprocessBam over every golden BAM and the long-read cases crossed with the options, and over seeded
crafted files whose records carry random, partly malformed aux fields, CIGARs and lengths.  With --gpu, only the cases
that need the device: the goldens and the crafted files through genome= and mates="anywhere", and callMethylation's
inflated output for the three strand tags."""
import gzip
import hashlib
import itertools
import json
import os
import random
import struct
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import epialleler_amd as ea  # noqa: E402
from test_preprocess_bam import _raw_bam  # noqa: E402
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


# ---- crafted records ---------------------------------------------------------------------------------------------------

def aux_field(rng, tag=None):
    tag = tag or bytes(rng.choice(b"ABNXYZM") for _ in range(2))
    ty = rng.choice("AcCsSiIfZHB")
    if ty in "AcC":
        return tag + ty.encode() + bytes([rng.randrange(256)])
    if ty in "sS":
        return tag + ty.encode() + os_bytes(rng, 2)
    if ty in "iIf":
        return tag + ty.encode() + os_bytes(rng, 4)
    if ty in "ZH":
        return tag + ty.encode() + bytes(rng.choice(b"zZxXhH.CTGA0123") for _ in range(rng.randrange(0, 12))) + b"\0"
    sub = rng.choice("cCsSiIf")
    n = rng.randrange(0, 6)
    return tag + b"B" + sub.encode() + struct.pack("<I", n) + os_bytes(rng, n * {"c": 1, "C": 1, "s": 2, "S": 2}.get(sub, 4))


def os_bytes(rng, n):
    return bytes(rng.randrange(256) for _ in range(n))


def malformed_field(rng, kind):
    tag = bytes(rng.choice(b"ABNXYZ") for _ in range(2))
    if kind == "z_open":                                             # a string without its terminator
        return tag + b"Z" + b"abc"
    if kind == "b_long":                                             # an array whose count runs past the record
        return tag + b"B" + rng.choice((b"c", b"S", b"i")) + struct.pack("<I", rng.choice((7, 1000, 0x7FFFFFFF, 0xFFFFFFFF))) + os_bytes(rng, 3)
    if kind == "b_cut":                                              # an array header cut short
        return tag + b"B" + b"c" + b"\1"
    return tag + bytes([rng.choice(b"?qZ!")]).replace(b"Z", b"k") + os_bytes(rng, rng.randrange(0, 4))   # unknown type


def crafted_record(rng, i, l_seq, pe):
    xm = bytes(rng.choice(b"zZxXhH.") for _ in range(l_seq))
    methyl = [b"XGZ" + rng.choice((b"CT", b"GA")) + b"\0", b"XMZ" + xm + b"\0"]
    r = rng.random()
    if r < 0.15:
        methyl[rng.randrange(2)] = rng.choice((b"XG", b"XM")) + rng.choice((b"i" + os_bytes(rng, 4), b"C\7", b"Bc" + struct.pack("<I", 2) + b"ab"))
    elif r < 0.25:
        methyl = [rng.choice((b"YDZf\0", b"ZSZ+-\0", b"XGZCT\0"))]   # to be called with a genome
    elif r < 0.30:
        methyl.append(b"MMZC+m,1,0;\0")
        methyl.append(b"MLBC" + struct.pack("<I", rng.choice((2, 2, 900))) + b"\x80\xf0")
    fields = [aux_field(rng) for _ in range(rng.randrange(0, 5))]
    for m in methyl:
        fields.insert(rng.randrange(len(fields) + 1), m)
    if rng.random() < 0.5:
        bad = malformed_field(rng, rng.choice(("z_open", "b_long", "b_cut", "unknown")))
        fields.insert(rng.randrange(len(fields) + 1), bad)          # XG / XM land before or after it
    cigar = [(0, l_seq)]
    c = rng.random()
    if c < 0.12:
        cigar = [(0, l_seq // 2), (rng.choice((10, 11, 15)), 3), (0, l_seq - l_seq // 2)]   # an unknown operation
    elif c < 0.24:
        cigar = [(0, l_seq + rng.choice((-2, -1, 1, 5)))]            # l_seq disagrees with the CIGAR
    elif c < 0.5:
        cigar = [(4, 1), (0, l_seq - 3), (2, 2), (1, 1), (3, 4), (0, 1)]
    flag, mpos, tlen = (rng.choice((0, 16)), -1, 0) if not pe else ((99, 150, 40) if i % 2 == 0 else (147, 100, -40))
    qname = (b"q%d" % (i // 2 if pe else i)) + b"\0"
    core = struct.pack("<iiBBHHHiiii", 0, 100 + (i % 2) * 50, len(qname), 60, 4680, len(cigar), flag, l_seq, 0 if pe else -1, mpos, tlen)
    cg = b"".join(struct.pack("<I", (ln << 4) | op) for op, ln in cigar)
    return core + qname + cg + bytes([0x12] * ((l_seq + 1) // 2)) + bytes([40] * l_seq) + b"".join(fields)


def crafted_files(d, n=600):
    paths = []
    for k in range(n):
        rng = random.Random(k)
        pe = k % 3 == 0
        recs = [crafted_record(rng, i, rng.randrange(4, 24), pe) for i in range(2 if pe or rng.random() < 0.5 else 1)]
        paths.append(_raw_bam(os.path.join(d, "crafted_%03d.bam" % k), recs))
    return paths


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
