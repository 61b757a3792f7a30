"""extractPatternsBed on the GPU (epi_batch_extract_patterns_multi): every table equals what extractPatterns gives for
that BED row and what the CPU oracle gives, hashes included -- on the reference's fixtures for every row and over the
argument grid, on random batches through rcpp_extract_patterns_multi, on an unsorted batch and with negative coordinates
(the target-by-target path), over several scratch groups, and on a 10^7-row resident batch whose size must not show in launches or scratch."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers as H
import synth_np
import test_extract_patterns as TP
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
BAM = os.path.join(H.GOLDEN, "bam")


@pytest.fixture(scope="module")
def ea():
    import epialleler_amd
    return epialleler_amd


@pytest.fixture
def hook_env(ea, monkeypatch):
    """EPIHIP_* test hooks inside this process (the library re-reads them after every change and after the restore)."""
    lib = ea._lib.load()

    def setenv(name, value):
        monkeypatch.setenv(name, value)
        lib.epi_options_reload()
    yield setenv
    monkeypatch.undo()
    lib.epi_options_reload()


def same_table(a, b):
    assert a["positions"] == b["positions"] and a["pattern"] == b["pattern"]
    for k in ("strand", "start", "end", "nbase", "cells"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(np.asarray(a["beta"], np.float64).view(np.uint64), np.asarray(b["beta"], np.float64).view(np.uint64))


def same_report(a, b):
    """Column for column: names and order, values, the BED row and the levels."""
    assert list(a.keys()) == list(b.keys())
    for k in a:
        if k == "beta":
            assert np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64))
        else:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
    assert getattr(a, "bed", None) == getattr(b, "bed", None)
    assert a.levels == b.levels
    assert getattr(a, "pattern_levels", None) == getattr(b, "pattern_levels", None)


def stats(ea, bam):
    g, p, s = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    ea._lib.check(ea._lib.load().epi_batch_extract_patterns_multi_stats(bam.batch(), C.byref(g), C.byref(p), C.byref(s)))
    return g.value, p.value, s.value


def profiled(ea, fn, *labels):
    """fn() with the profiler on -> (result, launches per label)"""
    lib = ea._lib.load()
    lib.epi_prof_reset()
    lib.epi_prof_enable(1)
    try:
        res = fn()
    finally:
        lib.epi_prof_enable(0)
    out = []
    for lb in labels:
        ms, n = C.c_double(0), C.c_int64(0)
        lib.epi_prof_get(lb.encode(), C.byref(ms), C.byref(n))
        out.append(n.value)
    return res, out


# ---- 1. the fixtures, every row ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bam,bed,nrows,nonempty,total,largest", [("capture.bam", "capture.bed", 565, 485, 2697, 125),
                                                                   ("amplicon010meth.bam", "amplicon.bed", 4, 4, 942, 310)])
def test_every_bed_row_of_the_fixtures(ea, bam, bed, nrows, nonempty, total, largest):
    pb = ea.preprocessBam(os.path.join(BAM, bam))
    bedp = os.path.join(BAM, bed)
    reps = ea.extractPatternsBed(pb, bedp)
    assert len(reps) == nrows
    assert stats(ea, pb)[0] == 1                                   # the batched path, one group
    npat = []
    for i, rep in enumerate(reps):
        same_report(rep, ea.extractPatterns(pb, bedp, bed_row=i + 1))
        tab = TP.table_from_report(rep)
        same_table(tab, TP.oracle_patterns(bam=bam, bed=bed, bed_row=i + 1))
        npat.append(len(tab["pattern"]))
    assert sum(1 for k in npat if k) >= nonempty and sum(npat) == total and max(npat) == largest


# ---- 2. the argument grid ------------------------------------------------------------------------------------------------

GRID = ([dict(extract_context=c) for c in ("CG", "CHG", "CHH", "CxG", "CX")] +
        [dict(clip_patterns=c) for c in (False, True)] +
        [dict(min_context_freq=f) for f in (0, 0.01, 0.5, 1)] +
        [dict(match_min_overlap=m) for m in (1, 50, 10 ** 6)] +
        [dict(strand_offset=0), dict(strand_offset=2, extract_context="CG", clip_patterns=True),
         dict(extract_context="CX", clip_patterns=True, min_context_freq=0.5, match_min_overlap=50)])


@pytest.mark.parametrize("kw", GRID, ids=lambda kw: ",".join("%s=%s" % it for it in kw.items()))
@pytest.mark.parametrize("bam,bed,rows", [("capture.bam", "capture.bed", list(range(1, 566, 9))),
                                          ("amplicon010meth.bam", "amplicon.bed", None)])
def test_argument_grid(ea, bam, bed, rows, kw):
    pb = ea.preprocessBam(os.path.join(BAM, bam))
    bedp = os.path.join(BAM, bed)
    reps = ea.extractPatternsBed(pb, bedp, bed_rows=rows, **kw)
    rows = rows if rows is not None else [1, 2, 3, 4]
    assert len(reps) == len(rows)
    for r, rep in zip(rows, reps):
        same_report(rep, ea.extractPatterns(pb, bedp, bed_row=r, **kw))
        same_table(TP.table_from_report(rep), TP.oracle_patterns(bam=bam, bed=bed, bed_row=r, **kw))
    if kw.get("match_min_overlap", 1) == 10 ** 6:
        assert not any(bool(rep) for rep in reps)                  # no read is that long
    elif kw.get("min_context_freq", 0.01) < 1:                     # (a position every read of a target covers is rare)
        assert any(bool(rep) for rep in reps)


def test_highlight_positions_over_several_targets(ea):
    pb = ea.preprocessBam(os.path.join(BAM, "capture.bam"))
    bed = ea.readBed(os.path.join(BAM, "capture.bed"))
    # the SNV of the reference's test inside a small BED of overlapping, nested and distant targets
    b = ea.Bed(["chr17", "chr17", "chr17", "chr20", "chr17"], [61864583, 61864500, 61864584, 57266125, 61864586],
               [61864585, 61864700, 61864584, 57268185, 61864600])
    cases = ([61864584], [61864584, 61864584, 61864584], [61864584, 61864586], [1, 2, -61864584],
             [61864590, 61864584, 57266200, 57266200, 61864599, 5], list(range(61864580, 61864592)))
    for hl in cases:
        reps = ea.extractPatternsBed(pb, b, highlight_positions=hl)
        assert len(reps) == 5
        for r, rep in enumerate(reps):
            same_report(rep, ea.extractPatterns(pb, b, bed_row=r + 1, highlight_positions=hl))
    # (test_gpu_patterns.py:52-58: duplicated / out-of-target positions change nothing)
    one = ea.extractPatternsBed(pb, "chr17:61864583-61864585", highlight_positions=[61864584, 61864584, 61864584])
    two = ea.extractPatternsBed(pb, "chr17:61864583-61864585", highlight_positions=[61864584, 61864586])
    same_report(one[0], two[0])
    assert "61864584" in one[0] and len(one) == 1
    same_report(ea.extractPatternsBed(pb, "chr17:61864583-61864585")[0],
                ea.extractPatternsBed(pb, "chr17:61864583-61864585", highlight_positions=[1, 2, -61864584])[0])
    # highlight positions of the whole BED: every 40th row's start
    hl = [int(p) for p in bed.start[::40]] + [int(bed.start[0])]
    reps = ea.extractPatternsBed(pb, bed, bed_rows=list(range(1, 566, 40)), highlight_positions=hl)
    for r, rep in zip(range(1, 566, 40), reps):
        same_report(rep, ea.extractPatterns(pb, bed, bed_row=r, highlight_positions=hl))


def test_bed_forms_and_row_lists(ea):
    path = os.path.join(BAM, "capture.bam")
    pb = ea.preprocessBam(path)
    bedp = os.path.join(BAM, "capture.bed")
    # zero-based BED
    for r, rep in zip((1, 2, 300), ea.extractPatternsBed(pb, bedp, bed_rows=[1, 2, 300], zero_based_bed=True)):
        same_report(rep, ea.extractPatterns(pb, bedp, bed_row=r, zero_based_bed=True))
    # "chr:start-end", from the file (preprocessBam runs inside) and with preprocessBam's arguments
    for kw in ({}, {"min_mapq": 30}):
        reps = ea.extractPatternsBed(path, "chr20:57266125-57268185", **kw)
        assert len(reps) == 1 and reps[0]
        same_report(reps[0], ea.extractPatterns(path, "chr20:57266125-57268185", **kw))
    same_table(TP.table_from_report(ea.extractPatternsBed(path, "chr20:57266125-57268185")[0]),
               TP.oracle_patterns(bam="capture.bam", bed="chr20:57266125-57268185"))
    # order, duplicates and missing rows
    rows = [3, 3, 1, 999, 0]
    reps = ea.extractPatternsBed(pb, bedp, bed_rows=rows)
    assert len(reps) == 5
    for r, rep in zip(rows, reps):
        same_report(rep, ea.extractPatterns(pb, bedp, bed_row=r))
    assert not reps[3] and not reps[4] and not hasattr(reps[3], "bed")
    assert reps[0].bed == reps[1].bed == ea.readBed(bedp).names()[2]
    assert ea.extractPatternsBed(pb, bedp, bed_rows=[]) == []
    assert len(ea.extractPatternsBed(pb, bedp, bed_rows=np.asarray([565, 1]))) == 2
    # a chromosome the BAM does not have
    b = ea.Bed(["chrNone", "chr20"], [1, 57266125], [10 ** 8, 57268185])
    reps = ea.extractPatternsBed(pb, b)
    assert not reps[0] and reps[1]
    same_report(reps[0], ea.extractPatterns(pb, b, bed_row=1))


# ---- 3. random batches through rcpp_extract_patterns_multi ---------------------------------------------------------------

def oracle_table(t, target, mo, ctx, freq, clip, ro, hl):
    o = orc.extract_patterns(t["xm"], t["off"], t["rname"], t["strand"], t["start"], target[0], target[1], target[2], mo, ctx, freq,
                             clip, ro, list(hl))
    return TP.table_from(o["strand"], o["start"], o["end"], o["nbase"], o["beta"], ["%016X" % int(v) for v in o["fnv"]],
                         o["positions"], o["cells"])


def check_multi(ea, t, targets, mo=1, ctx="Zz", freq=0.01, clip=False, ro=0, hl=None, batched=True, single=False):
    """rcpp_extract_patterns_multi on the templates t against the oracle (single: against rcpp_extract_patterns);
    -> (patterns in all tables, the call's statistics)"""
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"])
    try:
        reps = ea.rcpp_extract_patterns_multi(bam, targets, mo, ctx, freq, clip, ro, hl)
        st = stats(ea, bam)
        assert len(reps) == len(targets)
        if targets and len(t["start"]):
            assert (st[0] >= 1) == batched
        n = 0
        for k, (tg, rep) in enumerate(zip(targets, reps)):
            tab = TP.table_from_report(rep)
            h = hl[k] if hl is not None else ()
            if single:
                same_table(tab, TP.table_from_report(ea.rcpp_extract_patterns(bam, tg[0], tg[1], tg[2], mo, ctx, freq, clip, ro, h)))
            else:
                same_table(tab, oracle_table(t, tg, mo, ctx, freq, clip, ro, h))
            if rep:
                assert np.all(rep["seqnames"] == tg[0])
            n += len(tab["pattern"])
        return n, st
    finally:
        bam.close()


def merge(parts):
    """Templates (dicts of SoA columns) -> one batch sorted by (rname, start), stable."""
    rname = np.concatenate([p["rname"] for p in parts]); start = np.concatenate([p["start"] for p in parts])
    strand = np.concatenate([p["strand"] for p in parts])
    rows = [p["xm"][p["off"][i]:p["off"][i + 1]] for p in parts for i in range(len(p["start"]))]
    order = np.lexsort((start, rname))
    off = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([rows[i].size for i in order], out=off[1:])
    xm = np.concatenate([rows[i] for i in order]) if rows else np.zeros(0, np.uint8)
    return {"xm": xm, "off": off, "rname": rname[order].astype(np.int32), "strand": strand[order].astype(np.int32),
            "start": start[order].astype(np.int32)}


def random_targets(rng, k, n_rname, span, width):
    out = []
    for _ in range(k):
        ts = int(rng.integers(1, span))
        out.append((int(rng.integers(1, n_rname + 1)), ts, ts + int(rng.integers(0, width))))
    return out


def test_random_batches_and_arguments(ea):
    rng = np.random.default_rng(2024)
    total = 0
    for it in range(30):
        t = synth_np.random_templates(rng, int(rng.integers(1, 1500)), 0, int(rng.integers(1, 500)), int(rng.integers(1, 4)),
                                      int(rng.integers(50, 4000)), p_garbage=float(rng.choice([0, 0.1])))
        targets = random_targets(rng, int(rng.integers(1, 12)), 3, 4000, 600)
        ctx = str(rng.choice(["Zz", "ZzXx", "HhXxZz", "Hh"]))
        hl = [sorted({int(p) for p in rng.integers(ts, te + 1, size=int(rng.integers(0, 4)))}) for _, ts, te in targets]
        total += check_multi(ea, t, targets, int(rng.integers(1, 30)), ctx, float(rng.choice([0.0, 0.01, 0.2])), bool(rng.integers(0, 2)),
                             int(rng.integers(0, 3)), hl if it % 3 else None)[0]
    assert total > 300


def test_target_shapes(ea):
    rng = np.random.default_rng(7)
    t = synth_np.random_templates(rng, 3000, 20, 200, 2, 6000, alphabet="..zZxXhH")
    # overlapping, nested, identical, empty (no read: beyond the span), an rname no row has, position 1, descending order
    targets = [(1, 1000, 1500), (1, 1200, 1300), (1, 1250, 1250), (1, 1000, 1500), (1, 1000, 1500), (1, 1400, 2400),
               (2, 50000, 50100), (1, 7000, 7000), (3, 1000, 1500), (9, 1, 100), (-2 ** 31, 1, 100),
               (1, 1, 1), (1, 1, 60), (2, 1, 5000), (2, 5900, 5800)]
    for clip in (False, True):
        n, st = check_multi(ea, t, targets, clip=clip, ro=1)
        assert n > 1000 and st[0] == 1
    n, _ = check_multi(ea, t, sorted(targets, key=lambda g: (-g[0], -g[1])), ctx="ZzXxHh", freq=0.0)
    assert n > 1000
    # both strands with every reverse offset (a CpG track: the minus strand's calls sit one position to the right)
    for ro in (0, 1, 2):
        for clip in (False, True):
            assert check_multi(ea, t, targets[:6] + targets[11:14], ctx="ZzXx", ro=ro, clip=clip, freq=0.05)[0] > 300
    # min_overlap below 1 lets abutting rows in: the candidate range widens with it.  Against the single call (the
    # contract): its window of positions assumes an overlap, so it drops the far positions of such rows, and so does this
    for mo in (0, -3, -40):
        assert check_multi(ea, t, targets, mo=mo, single=True)[0] > 1000
    # ntargets 0 and 1
    assert check_multi(ea, t, [])[0] == 0
    assert check_multi(ea, t, [(2, 3000, 3100)])[0] > 10
    # an empty batch
    e = {"xm": np.zeros(0, np.uint8), "off": np.zeros(1, np.int64), "rname": np.zeros(0, np.int32), "strand": np.zeros(0, np.int32),
         "start": np.zeros(0, np.int32)}
    assert check_multi(ea, e, targets[:3])[0] == 0


def test_one_long_row_among_short_rows(ea):
    rng = np.random.default_rng(11)
    short = synth_np.random_templates(rng, 4000, 50, 150, 2, 30000, alphabet="...zZxh")
    long_ = synth_np.random_templates(rng, 1, 10000, 10000, 1, 2, alphabet="..zZ")
    long_["start"][:] = 8000
    t = merge([short, long_])
    assert int(np.diff(t["off"]).max()) == 10000
    targets = [(1, 17000, 17500), (1, 17999, 17999), (1, 18000, 18010), (1, 7900, 8000), (1, 100, 600), (2, 17000, 17500), (1, 12000, 12000)]
    for clip in (False, True):
        n, st = check_multi(ea, t, targets, clip=clip, ro=1)
        assert n > 50
    # the long row is one of the patterns of the targets it covers, and of no other
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"])
    try:
        reps = ea.rcpp_extract_patterns_multi(bam, targets, 1, "Zz", 0.0, False, 0)
        has = [bool(rep) and bool(np.any((rep["start"] == 8000) & (rep["end"] == 17999))) for rep in reps]
        assert has == [True, True, False, True, False, False, True]
    finally:
        bam.close()


def test_deep_pile_up(ea):
    rng = np.random.default_rng(13)
    pile = synth_np.random_templates(rng, 6000, 100, 400, 1, 40, alphabet="..zZzZxh")
    pile["start"] += 5000
    rest = synth_np.random_templates(rng, 2000, 50, 300, 2, 12000, alphabet="..zZxh")
    t = merge([pile, rest])
    targets = [(1, 5100, 5200), (1, 100, 600), (1, 5040, 5041), (1, 9000, 9500), (2, 5100, 5200)]
    n, st = check_multi(ea, t, targets, freq=0.01)
    assert n > 12000 and st[1] > 12000                           # the pile-up is in two targets
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"])
    try:
        reps = ea.rcpp_extract_patterns_multi(bam, targets, 1, "Zz", 0.01, False, 0)
        assert len(reps[0]["pattern"]) >= 6000
    finally:
        bam.close()


def test_several_scratch_groups(ea, hook_env):
    rng = np.random.default_rng(17)
    t = synth_np.random_templates(rng, 5000, 50, 250, 2, 20000, alphabet="..zZxXh")
    targets = random_targets(rng, 60, 2, 20000, 700)
    hl = [sorted({int(p) for p in rng.integers(ts, te + 1, size=2)}) for _, ts, te in targets]
    want_n, st = check_multi(ea, t, targets, hl=hl, ro=1)
    assert st[0] == 1 and want_n > 2000
    for cap in (1 << 16, 1 << 13, 1):                             # 64 KiB, 8 KiB, and a cap below every single target
        hook_env("EPIHIP_PAT_GROUP_BYTES", str(cap))
        n, st2 = check_multi(ea, t, targets, hl=hl, ro=1)
        assert n == want_n and st2[1] == st[1]
        assert st2[0] >= 3 and (cap > 1 or st2[0] == len(targets))
        assert st2[2] <= st[2]


# ---- 4. an unsorted batch ------------------------------------------------------------------------------------------------

def test_unsorted_batch_takes_the_target_by_target_path(ea):
    rng = np.random.default_rng(19)
    t = synth_np.random_templates(rng, 2500, 20, 200, 2, 5000, alphabet="..zZxXhH")
    a, b = t["rname"] == 1, t["rname"] == 2
    u = merge([H.subset(t, b)])
    v = merge([H.subset(t, a)])
    # the rname 2 block first: descending code order
    off = np.concatenate([u["off"], v["off"][1:] + u["off"][-1]])
    t2 = {"xm": np.concatenate([u["xm"], v["xm"]]), "off": off, "rname": np.concatenate([u["rname"], v["rname"]]),
          "strand": np.concatenate([u["strand"], v["strand"]]), "start": np.concatenate([u["start"], v["start"]])}
    assert t2["rname"][0] == 2 and t2["rname"][-1] == 1
    targets = random_targets(rng, 25, 2, 5000, 500) + [(1, 1, 1), (3, 1, 100)]
    hl = [[ts] for _, ts, te in targets]
    n, st = check_multi(ea, t2, targets, hl=hl, ro=1, batched=False)
    assert n > 1000 and st == (0, 0, 0)
    # the same rows sorted give the same patterns, by the batched path
    n2, st2 = check_multi(ea, merge([t2]), targets, hl=hl, ro=1)
    assert n2 == n and st2[0] == 1


def test_negative_coordinates_take_the_target_by_target_path(ea):
    rng = np.random.default_rng(29)
    t = synth_np.random_templates(rng, 300, 20, 80, 2, 2000, alphabet="..zZxXhH")
    assert t["rname"][4] == 1 and t["rname"][-1] == 2
    t["start"][:5] = np.sort(rng.integers(-40, 0, size=5))         # the first rows of rname 1: the order holds
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"])
    try:
        # rows with a negative start on a target's rname; no such row, but a target with a negative start (it covers every
        # row of rname 2, so its window holds all their positions)
        for targets in ([(1, 100, 400), (2, 100, 400), (1, 1, 50), (2, 1500, 1900), (2, 5000, 5100)],
                        [(2, 100, 400), (2, -5, 2100), (2, 1, 1)]):
            reps = ea.rcpp_extract_patterns_multi(bam, targets, 1, "Zz", 0.01, False, 0)
            assert stats(ea, bam) == (0, 0, 0)
            assert sum(bool(rep) for rep in reps) >= 2
            for tg, rep in zip(targets, reps):
                tab = TP.table_from_report(rep)
                same_table(tab, TP.table_from_report(ea.rcpp_extract_patterns(bam, tg[0], tg[1], tg[2], 1, "Zz", 0.01, False, 0)))
                if tg[0] == 2:                                     # (a row with a negative start overlaps every target of rname 1)
                    same_table(tab, oracle_table(t, tg, 1, "Zz", 0.01, False, 0, ()))
    finally:
        bam.close()


# ---- 5. the structure ----------------------------------------------------------------------------------------------------

def test_block_edges_of_the_all_rows_pass(ea):
    rng = np.random.default_rng(31)
    for n in (1, 255, 256, 257, 513):
        t = synth_np.random_templates(rng, n, 20, 80, 1, 300, alphabet="..zZxXhH")
        bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"])
        try:
            for tg, npat in (((1, 1, 400), n), ((1, 1000, 1100), 0)):     # every row, no row
                tab = TP.table_from_report(ea.rcpp_extract_patterns(bam, tg[0], tg[1], tg[2], 1, "ZzXxHh", 0.0, False, 0))
                same_table(tab, oracle_table(t, tg, 1, "ZzXxHh", 0.0, False, 0, ()))
                assert len(tab["pattern"]) == npat                 # (a row of 20 bytes without a context byte: 4^-20)
        finally:
            bam.close()


def test_single_call_keeps_its_label_and_the_multi_statistics(ea):
    rng = np.random.default_rng(37)
    t = synth_np.random_templates(rng, 300, 20, 80, 2, 2000, alphabet="..zZxXhH")
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"])
    try:
        ea.rcpp_extract_patterns_multi(bam, [(1, 100, 400), (2, 100, 400)], 1, "Zz", 0.01, False, 0)
        st = stats(ea, bam)
        assert st[0] == 1 and st[1] > 0 and st[2] > 0
        rep, counts = profiled(ea, lambda: ea.rcpp_extract_patterns(bam, 1, 100, 400, 1, "Zz", 0.01, False, 0),
                               "extract_patterns_multi", "extract_patterns")
        assert rep and counts[0] == 0 and counts[1] >= 1
        assert stats(ea, bam) == st
    finally:
        bam.close()



def test_launches_do_not_grow_with_the_targets(ea):
    pb = ea.preprocessBam(os.path.join(BAM, "capture.bam"))
    bedp = os.path.join(BAM, "capture.bed")
    pb.batch()
    counts = {}
    for k in (50, 565):
        reps, (multi, single) = profiled(ea, lambda: ea.extractPatternsBed(pb, bedp, bed_rows=list(range(1, k + 1))),
                                         "extract_patterns_multi", "extract_patterns")
        assert len(reps) == k and stats(ea, pb)[0] == 1
        counts[k] = multi
        assert single == 0
    assert counts[50] == counts[565] and 1 <= counts[50] <= 4


def test_ten_million_rows_cost_what_the_targets_hold(ea):
    import torch
    from epialleler_amd import synth
    n = 10 ** 7
    bam = synth.generate_device(n, read_len=100, n_chr=4, depth=30, seed=5)
    try:
        bam.batch()
        start = bam.dev["start"]
        rng = np.random.default_rng(23)
        rows = np.sort(rng.integers(0, n, size=100))
        rn = bam.dev["rname"][torch.as_tensor(rows, device=start.device)].cpu().numpy()
        st = start[torch.as_tensor(rows, device=start.device)].cpu().numpy()
        targets = [(int(r), int(s), int(s) + 499) for r, s in zip(rn, st)]
        reps, (launches, _) = profiled(ea, lambda: ea.rcpp_extract_patterns_multi(bam, targets, 1, "Zz", 0.01, False, 1),
                                       "extract_patterns_multi", "extract_patterns")
        groups, pairs, scratch = stats(ea, bam)
        assert groups == 1 and 1 <= launches <= 4
        # the documented bound (include/epihip.h): 40 B per pair + 8 B per window position, 32 B per overlapping row + 4 B per
        # cell, 200 B per target, 1/8 of slack -- and nothing of the 8 B per row of the batch (80 MB) the single call takes
        npat = sum(len(r["pattern"]) if r else 0 for r in reps)
        cells = sum((len(r) - 7) * len(r["pattern"]) if r else 0 for r in reps)
        window = sum(e - s + 2 * 100 + 1 + 8 for _, s, e in targets)
        bound = (40 * pairs + 8 * window + 32 * pairs + 4 * cells + 200 * len(targets)) * 9 // 8 + 16 * 256
        assert 0 < scratch <= bound and scratch < 8 * n // 2
        assert pairs < 100 * 30 * 20 and npat > 100                # ~ depth x (500 + 100) / 100 = 180 candidate rows per target
        for k in range(0, 100, 10):
            same_report(reps[k], ea.rcpp_extract_patterns(bam, *targets[k], 1, "Zz", 0.01, False, 1))
        assert sum(bool(reps[k]) for k in range(0, 100, 10)) >= 8
    finally:
        bam.close()
