"""Differential run of pattern extraction: one library per process (EPIHIP_LIB selects it), one JSON of case -> SHA-256 of
the result (or the error text) per run; two libraries behave alike where their JSON files are identical.  Needs the GPU.

    EPIHIP_LIB=/path/to/parent/libepihip.so python scratch/patterns_refactor_diff.py parent.json
    python scratch/patterns_refactor_diff.py new.json
    cmp parent.json new.json

Cases: both golden BAMs with their BEDs through extractPatterns per row, extractPatternsBed and summarisePatterns, alone and
over the argument grid of tests/test_gpu_patterns_bed.py; seeded random batches of at most 1500 rows -- sorted, unsorted or
with negative starts -- with random targets, contexts, clip, reverse offset, min_overlap (values <= 0 included), frequency
and highlight positions through rcpp_extract_patterns, rcpp_extract_patterns_multi and rcpp_summarise_patterns_multi.  The
statistics of both multi calls are part of every digest."""
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import epialleler_amd as ea  # noqa: E402
import synth_np  # noqa: E402
from test_gpu_patterns_bed import GRID  # noqa: E402

BAM = os.path.join(ROOT, "tests", "golden", "bam")
RESULTS = {}
NRANDOM = 400


def digest(reps, *more):
    h = hashlib.sha256()
    for rep in reps:
        h.update(b"|%d|%r|%r|" % (rep.nrow, getattr(rep, "bed", None), getattr(rep, "pattern_levels", None)))
        for k in rep:
            h.update(k.encode())
            h.update("\n".join(rep[k]).encode() if k == "pattern" else np.ascontiguousarray(rep[k]).tobytes())
    h.update(repr(more).encode())
    return h.hexdigest()


def stats(bam):
    out = []
    for fn in ("epi_batch_extract_patterns_multi_stats", "epi_batch_summarise_patterns_stats"):
        v = [C.c_int64(0) for _ in range(3)]
        ea._lib.check(getattr(ea._lib.load(), fn)(bam.batch(), *[C.byref(x) for x in v]))
        out.append(tuple(x.value for x in v))
    return out


def case(name, fn):
    try:
        RESULTS[name] = fn()
    except Exception as e:                                          # the message is part of the behaviour
        RESULTS[name] = "%s: %s" % (type(e).__name__, e)


def golden_cases():
    for bam, bed, nrows in (("capture.bam", "capture.bed", 565), ("amplicon010meth.bam", "amplicon.bed", 4)):
        pb = ea.preprocessBam(os.path.join(BAM, bam))
        bedp = os.path.join(BAM, bed)
        for g, kw in enumerate([{}] + GRID):
            tag = "%s %d %r" % (bam, g, sorted(kw.items()))
            rows = list(range(1, nrows + 1, 1 if g == 0 else 9)) if nrows > 4 else [1, 2, 3, 4]
            case("single " + tag, lambda: digest([ea.extractPatterns(pb, bedp, bed_row=r, **kw) for r in rows], stats(pb)))
            case("bed " + tag, lambda: digest(ea.extractPatternsBed(pb, bedp, bed_rows=rows, **kw), stats(pb)))
            case("summary " + tag, lambda: digest(ea.summarisePatterns(pb, bedp, bed_rows=rows, **kw), stats(pb)))
        hl = [61864584, 43125000, 57266200]
        case("bed hl " + bam, lambda: digest(ea.extractPatternsBed(pb, bedp, highlight_positions=hl), stats(pb)))
        case("summary hl " + bam, lambda: digest(ea.summarisePatterns(pb, bedp, highlight_positions=hl), stats(pb)))


def random_case(k):
    rng = np.random.default_rng(1000 + k)
    kind = ("sorted", "unsorted", "negative")[k % 3]
    n = int(rng.integers(1, 1501))
    n_rname = int(rng.integers(1, 4))
    span = int(rng.integers(50, 4000))
    t = synth_np.random_templates(rng, n, 0, int(rng.integers(1, 300)), n_rname, span, p_garbage=float(rng.choice([0, 0.1])))
    if kind == "unsorted":
        perm = rng.permutation(n)
        rows = [t["xm"][t["off"][i]:t["off"][i + 1]] for i in perm]
        off = np.zeros(n + 1, np.int64)
        np.cumsum([r.size for r in rows], out=off[1:])
        t = {"xm": np.concatenate(rows) if off[-1] else np.zeros(0, np.uint8), "off": off, "rname": t["rname"][perm],
             "strand": t["strand"][perm], "start": t["start"][perm]}
    elif kind == "negative":                                         # the first rows of an rname move below 0; the order holds
        r = int(rng.integers(1, n_rname + 1))
        idx = np.flatnonzero(t["rname"] == r)[:int(rng.integers(1, 6))]
        t["start"][idx] = np.sort(rng.integers(-60, 0, size=idx.size))
    nt = int(rng.integers(1, 12))
    targets = []
    for _ in range(nt):
        ts = int(rng.integers(1, span + 100))
        if rng.random() < 0.05:
            ts = -int(rng.integers(1, 50))
        targets.append((int(rng.integers(1, n_rname + 2)), ts, ts + int(rng.integers(-2, 600))))
    mo = int(rng.choice([1, 1, 5, 30, 0, -3, -40]))
    ctx = str(rng.choice(["Zz", "ZzXx", "HhXxZz", "Hh"]))
    freq = float(rng.choice([0.0, 0.01, 0.2, 1.0]))
    clip, ro = bool(rng.integers(0, 2)), int(rng.integers(0, 3))
    hl = None if k % 4 == 0 else [sorted({int(p) for p in rng.integers(min(ts, te), max(ts, te) + 1, size=int(rng.integers(0, 4)))})
                                  for _, ts, te in targets]
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"])
    try:
        tag = "random %d %s" % (k, kind)
        case(tag + " multi", lambda: digest(ea.rcpp_extract_patterns_multi(bam, targets, mo, ctx, freq, clip, ro, hl), stats(bam)))
        case(tag + " single", lambda: digest([ea.rcpp_extract_patterns(bam, tg[0], tg[1], tg[2], mo, ctx, freq, clip, ro, hl[j] if hl else ())
                                              for j, tg in enumerate(targets)], stats(bam)))
        case(tag + " summary", lambda: digest(ea.rcpp_summarise_patterns_multi(bam, targets, mo, ctx, freq, clip, ro, hl, ("Zz", "z")),
                                              stats(bam)))
    finally:
        bam.close()


def error_cases():
    t = synth_np.random_templates(np.random.default_rng(5), 200, 10, 50, 1, 500)
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"])
    try:
        wide = (1, -2 ** 31, 2 ** 31 - 1)
        case("too wide single", lambda: digest([ea.rcpp_extract_patterns(bam, *wide, 1, "Zz", 0.01, False, 0)]))
        case("too wide multi", lambda: digest(ea.rcpp_extract_patterns_multi(bam, [(1, 1, 50), wide], 1, "Zz", 0.01, False, 0), stats(bam)))
        case("too wide summary", lambda: digest(ea.rcpp_summarise_patterns_multi(bam, [(1, 1, 50), wide], 1, "Zz", 0.01, False, 0), stats(bam)))
        case("no targets", lambda: digest(ea.rcpp_extract_patterns_multi(bam, [], 1, "Zz", 0.01, False, 0), stats(bam)))
    finally:
        bam.close()


if __name__ == "__main__":
    golden_cases()
    for k in range(NRANDOM):
        random_case(k)
    error_cases()
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(RESULTS, f, indent=0, sort_keys=True)
    errors = sum(1 for v in RESULTS.values() if ": " in v)
    print("%d cases (%d of them errors) -> %s" % (len(RESULTS), errors, sys.argv[1]))
