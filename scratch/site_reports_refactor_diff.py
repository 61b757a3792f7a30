"""Differential run of the reports that count over the per-strand site table (heterogeneity, linkage, haplotype blocks,
heterogeneity comparison): one library per process (EPIHIP_LIB selects it), one JSON of case -> SHA-256 of the result (or
the error text) per run; two libraries behave alike where their JSON files are identical.  Needs the GPU.

    EPIHIP_LIB=/path/to/parent/libepihip.so python scratch/site_reports_refactor_diff.py parent.json
    python scratch/site_reports_refactor_diff.py new.json
    cmp parent.json new.json

Cases: both golden BAMs through generateHeterogeneityReport (k = 2 .. 6, with the histograms), generateLinkageReport
(D = 1, 4, 16), generateHaplotypeBlocks and compareHeterogeneity (each BAM against the other and against itself), contexts
CG and CX; seeded random batches of at most 1500 rows -- sorted, with garbage bytes, one or several sequences -- through the
rcpp_* wrappers with random k, D, min_reads, span / distance caps and max_ooctx_meth_frac, each followed by one sequence
het -> link -> blocks -> pair table fetched again -> cmp -> het on the same batch, digested step by step; the refusals of
the C entry points (bad k, bad D, a fetch without its report, blocks without a linkage report, NULL columns, a batch set
up for a sharded report), whose messages are part of the digest.  A digest covers nrow, ncommon, every column's bytes and
the histogram arrays."""
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import epialleler_amd as ea  # noqa: E402
from epialleler_amd import _lib, api  # noqa: E402
import synth_np  # noqa: E402

BAM = os.path.join(ROOT, "tests", "golden", "bam")
RESULTS = {}
NRANDOM = 300


def digest(*reps):
    h = hashlib.sha256()
    for rep in reps:
        h.update(b"|%d|%r|" % (rep.nrow, getattr(rep, "ncommon", None)))
        for k in rep:
            h.update(k.encode())
            h.update(np.ascontiguousarray(rep[k]).tobytes())
        for k in ("counts", "counts_a", "counts_b"):
            if hasattr(rep, k):
                h.update(k.encode())
                h.update(repr(getattr(rep, k).shape).encode())
                h.update(np.ascontiguousarray(getattr(rep, k)).tobytes())
    return h.hexdigest()


def case(name, fn):
    assert name not in RESULTS, name
    try:
        RESULTS[name] = fn()
    except Exception as e:                                          # the message is part of the behaviour
        RESULTS[name] = "%s: %s" % (type(e).__name__, e)


def golden_cases():
    names = ("capture.bam", "amplicon010meth.bam")
    bams = {n: ea.preprocessBam(os.path.join(BAM, n)) for n in names}
    for ctx in ("CG", "CX"):
        for n in names:
            pb, tag = bams[n], "%s %s" % (n, ctx)
            for k in range(2, 7):
                case("het %s k=%d" % (tag, k), lambda: digest(ea.rcpp_heterogeneity_report(
                    pb, "".join(ea.CONTEXT_TO_BASES[ctx][x] for x in ("ctx_meth", "ctx_unmeth")), k, 0.1, with_counts=True)))
                case("het api %s k=%d" % (tag, k), lambda: digest(ea.generateHeterogeneityReport(pb, window_context=ctx, window_sites=k)))
            for D in (1, 4, 16):
                case("link %s D=%d" % (tag, D), lambda: digest(ea.generateLinkageReport(pb, linkage_context=ctx, max_neighbours=D)))
                case("blocks %s D=%d" % (tag, D), lambda: digest(ea.generateHaplotypeBlocks(pb, linkage_context=ctx, max_neighbours=D,
                                                                                           min_reads=2, min_r2=0.2, min_sites=2)))
            case("blocks default " + tag, lambda: digest(ea.generateHaplotypeBlocks(pb, linkage_context=ctx)))
            for m in names:
                for k in (2, 4, 6):
                    case("cmp %s vs %s k=%d" % (tag, m, k), lambda: digest(ea.rcpp_heterogeneity_compare(
                        pb, bams[m], "".join(ea.CONTEXT_TO_BASES[ctx][x] for x in ("ctx_meth", "ctx_unmeth")), k, 0.1, with_counts=True)))
                case("cmp api %s vs %s" % (tag, m), lambda: digest(ea.compareHeterogeneity(pb, bams[m], window_context=ctx)))
    for pb in bams.values():
        pb.close()


def random_batch(rng, n_rname, span):
    n = int(rng.integers(1, 1501))
    alphabet = None if rng.random() < 0.5 else "Zz..Zz.xXhH"
    t = synth_np.random_templates(rng, n, int(rng.integers(0, 30)), int(rng.integers(30, 700 if rng.random() < 0.1 else 300)), n_rname, span,
                                  p_garbage=float(rng.choice([0, 0.05])), alphabet=alphabet)
    return ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"], levels=tuple("s%d" % i for i in range(n_rname)))


def random_case(j):
    rng = np.random.default_rng(7000 + j)
    n_rname, span = int(rng.integers(1, 4)), int(rng.integers(40, 3000))
    bam, other = random_batch(rng, n_rname, span), random_batch(rng, n_rname, span)
    ctx = str(rng.choice(["Zz", "ZzXx", "HhXxZz", "Hh"]))
    k, D = int(rng.integers(2, 7)), int(rng.integers(1, 17))
    mr = int(rng.choice([0, 1, 1, 2, 5]))
    cap = int(rng.choice([0, 0, 5, 40, 400]))
    oo = float(rng.choice([0.0, 0.1, 0.5, 1.0]))
    r2, ms = float(rng.choice([0.0, 0.1, 0.5, 1.0])), int(rng.integers(2, 5))
    tag = "random %d" % j
    het = lambda b: digest(ea.rcpp_heterogeneity_report(b, ctx, k, oo, mr, cap, with_counts=bool(j % 2)))
    link = lambda b: digest(ea.rcpp_linkage_report(b, ctx, D, cap, oo, mr))
    blocks = lambda b: digest(ea.rcpp_linkage_blocks(b, ctx, D, cap, oo, mr, r2, ms))
    cmp_ = lambda a, b: digest(ea.rcpp_heterogeneity_compare(a, b, ctx, k, oo, mr, cap, with_counts=bool(j % 3)))

    state = {}

    def link_first():
        rep = ea.rcpp_linkage_report(bam, ctx, D, cap, oo, mr)
        state["npairs"] = rep.nrow
        return digest(rep)

    def pairs_again():                                               # the pair table behind the blocks is still the batch's report
        return digest(api._fetch_table(bam, _lib.load().epi_batch_linkage_fetch_dev, state["npairs"], 11, api.LINKAGE_COLUMNS, False))

    try:
        case(tag + " het", lambda: het(bam))
        case(tag + " link", link_first)
        case(tag + " blocks", lambda: blocks(bam))
        case(tag + " pairs again", pairs_again)
        case(tag + " cmp", lambda: cmp_(bam, other))
        case(tag + " cmp reverse", lambda: cmp_(other, bam))
        case(tag + " cmp self", lambda: cmp_(bam, bam))
        case(tag + " het again", lambda: het(bam))
        case(tag + " het other", lambda: het(other))
        case(tag + " link other", lambda: link(other))
    finally:
        bam.close()
        other.close()


def error_cases():
    lib = _lib.load()
    t = synth_np.random_templates(np.random.default_rng(5), 300, 10, 120, 2, 600, alphabet="Zz.")
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"])
    b = bam.batch()
    CAP = 1 << 16                                                     # rows the columns below hold: no report here comes near
    ic = list(torch.zeros((11, CAP), dtype=torch.int32, device="cuda").unbind(0))
    dc = list(torch.zeros((13, CAP), dtype=torch.float64, device="cuda").unbind(0))
    ip, dp = api._ptr_array(ic), api._ptr_array(dc)
    nrow, ncommon = C.c_int64(0), C.c_int64(0)

    def rc(code):                                                    # the code and the library's message, or "ok"
        msg = lib.epi_last_error()
        return "ok" if code == 0 else "%d: %s" % (code, msg.decode("utf-8", "replace") if msg else "")

    fetches = {"het": lambda i, d: lib.epi_batch_heterogeneity_fetch_dev(b, i, d, None, None),
               "link": lambda i, d: lib.epi_batch_linkage_fetch_dev(b, i, d, None),
               "blocks": lambda i, d: lib.epi_batch_linkage_blocks_fetch_dev(b, i, d, None),
               "cmp": lambda i, d: lib.epi_batch_heterogeneity_compare_fetch_dev(b, i, d, None, None, None)}

    def all_fetches(tag):
        if max(nrow.value, ncommon.value) > CAP:
            raise SystemExit("a report of %d rows: the fetches below would write past their columns" % nrow.value)
        for name, f in fetches.items():
            case("%s: %s fetch" % (tag, name), lambda: rc(f(ip, dp)))

    def null_columns(tag, name):
        hole = api._ptr_array(ic)
        hole[2] = None
        dhole = api._ptr_array(dc)
        dhole[0] = None
        case("%s: %s fetch, NULL arrays" % (tag, name), lambda: rc(fetches[name](None, None)))
        case("%s: %s fetch, NULL int column" % (tag, name), lambda: rc(fetches[name](hole, dp)))
        case("%s: %s fetch, NULL double column" % (tag, name), lambda: rc(fetches[name](ip, dhole)))

    try:
        all_fetches("fresh batch")
        case("fresh batch: blocks", lambda: rc(lib.epi_batch_linkage_blocks_dev(b, 0.5, 3, None, C.byref(nrow))))
        for k in (-1, 0, 1, 7, 100):
            case("het k=%d" % k, lambda: rc(lib.epi_batch_heterogeneity_report_dev(b, b"Zz", k, 0.1, 1, 0, None, C.byref(nrow))))
            case("cmp k=%d" % k, lambda: rc(lib.epi_batch_heterogeneity_compare_dev(b, b, b"Zz", k, 0.1, 1, 0, None, C.byref(ncommon), C.byref(nrow))))
        case("het span=-1", lambda: rc(lib.epi_batch_heterogeneity_report_dev(b, b"Zz", 4, 0.1, 1, -1, None, C.byref(nrow))))
        case("cmp span=-1", lambda: rc(lib.epi_batch_heterogeneity_compare_dev(b, b, b"Zz", 4, 0.1, 1, -1, None, C.byref(ncommon), C.byref(nrow))))
        for D in (-1, 0, 17):
            case("link D=%d" % D, lambda: rc(lib.epi_batch_linkage_report_dev(b, b"Zz", D, 0, 0.1, 1, None, C.byref(nrow))))
        case("link dist=-1", lambda: rc(lib.epi_batch_linkage_report_dev(b, b"Zz", 4, -1, 0.1, 1, None, C.byref(nrow))))
        case("NULL arguments", lambda: [rc(lib.epi_batch_heterogeneity_report_dev(b, None, 4, 0.1, 1, 0, None, C.byref(nrow))),
                                        rc(lib.epi_batch_linkage_report_dev(None, b"Zz", 4, 0, 0.1, 1, None, C.byref(nrow))),
                                        rc(lib.epi_batch_heterogeneity_compare_dev(b, None, b"Zz", 4, 0.1, 1, 0, None, C.byref(ncommon), C.byref(nrow))),
                                        rc(lib.epi_batch_linkage_blocks_dev(b, 0.5, 3, None, None))])
        all_fetches("after refusals")

        case("het run", lambda: [rc(lib.epi_batch_heterogeneity_report_dev(b, b"Zz", 3, 0.1, 1, 0, None, C.byref(nrow))), nrow.value])
        all_fetches("after het")
        null_columns("after het", "het")
        case("after het: blocks", lambda: rc(lib.epi_batch_linkage_blocks_dev(b, 0.5, 3, None, C.byref(nrow))))
        case("link run", lambda: [rc(lib.epi_batch_linkage_report_dev(b, b"Zz", 3, 0, 0.1, 1, None, C.byref(nrow))), nrow.value])
        all_fetches("after link")
        null_columns("after link", "link")
        for r2, ms in ((-0.1, 3), (1.5, 3), (float("nan"), 3), (0.5, 1)):
            case("blocks r2=%r sites=%d" % (r2, ms), lambda: rc(lib.epi_batch_linkage_blocks_dev(b, r2, ms, None, C.byref(nrow))))
        case("blocks run", lambda: [rc(lib.epi_batch_linkage_blocks_dev(b, 0.0, 2, None, C.byref(nrow))), nrow.value])
        all_fetches("after blocks")
        null_columns("after blocks", "blocks")
        case("cmp run", lambda: [rc(lib.epi_batch_heterogeneity_compare_dev(b, b, b"Zz", 3, 0.1, 1, 0, None, C.byref(ncommon), C.byref(nrow))),
                                 ncommon.value, nrow.value])
        all_fetches("after cmp")
        null_columns("after cmp", "cmp")

        # a batch set up for a sharded report
        T = lib.epi_cx_tile_positions(b"Z")
        k0, k1 = C.c_int64(0), C.c_int64(-1)
        _lib.check(lib.epi_batch_tile_key_range_for(b, T, None, C.byref(k0), C.byref(k1)))
        keys, owned = np.asarray([k0.value], np.int64), np.asarray([1], np.int32)
        slab = torch.zeros(16 * T, dtype=torch.int32, device="cuda")
        _lib.check(lib.epi_batch_cx_set_shared(b, C.c_void_p(keys.ctypes.data), C.c_void_p(owned.ctypes.data), 1, C.c_void_p(slab.data_ptr())))
        try:
            case("sharded: het", lambda: rc(lib.epi_batch_heterogeneity_report_dev(b, b"Zz", 3, 0.1, 1, 0, None, C.byref(nrow))))
            case("sharded: link", lambda: rc(lib.epi_batch_linkage_report_dev(b, b"Zz", 3, 0, 0.1, 1, None, C.byref(nrow))))
            case("sharded: cmp", lambda: rc(lib.epi_batch_heterogeneity_compare_dev(b, b, b"Zz", 3, 0.1, 1, 0, None, C.byref(ncommon), C.byref(nrow))))
            all_fetches("sharded")
        finally:
            _lib.check(lib.epi_batch_cx_set_shared(b, None, None, 0, None))
        case("after sharded: het", lambda: digest(ea.rcpp_heterogeneity_report(bam, "Zz", 3, 0.1, with_counts=True)))
    finally:
        bam.close()


if __name__ == "__main__":
    print("library:", _lib.LIB_PATH)
    golden_cases()
    for j in range(NRANDOM):
        random_case(j)
    error_cases()
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(RESULTS, f, indent=0, sort_keys=True)
    errors = sum(1 for v in RESULTS.values() if isinstance(v, str) and ": " in v)
    print("%d cases (%d of them errors or refusals) -> %s" % (len(RESULTS), errors, sys.argv[1]))
