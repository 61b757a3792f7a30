"""summarisePatterns on the GPU (epi_batch_summarise_patterns_multi): for every target the Report equals a plain
order-preserving group-by on (pattern, cells) of extractPatterns' own Report -- pattern, positions, cells, count and beta
(bitwise), in the order of first appearance.  On the reference's eight extractPatterns calls, on a synthetic pile-up
with one pattern on most of the rows, on groups cut into several batches of results, on table slices at the minimum
capacity with a probe that wraps, on unsorted rows (the target-by-target
path), under the result-neutral hooks in a fresh process, and with the profiler's launch counts."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import test_extract_patterns as TP

pytestmark = pytest.mark.gpu
BAM = os.path.join(H.GOLDEN, "bam")
HERE = os.path.dirname(os.path.abspath(__file__))
LEVELS = ("chrA", "chrB")


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


# ---- the yardstick ---------------------------------------------------------------------------------------------------

def position_columns(rep):
    return [k for k in rep if k.lstrip("-").isdigit()]


def summary_np(rep, bin_context="CG"):
    """patterns[, .(count=.N), by=c("pattern", base.positions)] plus beta (R/plotPatterns.R:172-184) of an extractPatterns
    Report, restated plainly: -> {"columns": names in order, "pattern", "cells" [ncol][nuniq], "count", "beta"} or None."""
    if not rep:
        return None
    pos = position_columns(rep)
    cells = np.stack([np.asarray(rep[k]) for k in pos])
    index, first, count = {}, [], []
    for i in range(cells.shape[1]):
        key = (rep["pattern"][i], cells[:, i].tobytes())
        if key not in index:
            index[key] = len(first)
            first.append(i)
            count.append(0)
        count[index[key]] += 1
    c = H.CONTEXT_TO_BASES[bin_context]
    meth_codes = {TP.LEVELS.index(ch) + 1 for ch in c["ctx_meth"]}
    unmeth_codes = {TP.LEVELS.index(ch) + 1 for ch in c["ctx_unmeth"]}
    beta = []
    for i in first:
        meth = sum(1 for v in cells[:, i] if int(v) in meth_codes)
        unmeth = sum(1 for v in cells[:, i] if int(v) in unmeth_codes)
        beta.append(meth / (meth + unmeth) if meth + unmeth > 0 else 0.0)
    return {"columns": ["pattern"] + pos + ["count", "beta"], "pattern": [rep["pattern"][i] for i in first],
            "cells": cells[:, first], "count": np.asarray(count, np.int64), "beta": np.asarray(beta, np.float64)}


def same_summary(got, rep, bin_context="CG"):
    """got: a Report of summarisePatterns; rep: extractPatterns' Report for the same target and arguments"""
    want = summary_np(rep, bin_context)
    if want is None:
        assert not got and got.nrow == 0
        assert getattr(got, "bed", None) == getattr(rep, "bed", None)
        return
    assert list(got.keys()) == want["columns"]
    assert list(got["pattern"]) == want["pattern"]
    pos = position_columns(got)
    for k, col in zip(pos, want["cells"]):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], col), k
    assert np.array_equal(got["count"], want["count"])
    assert got["beta"].dtype == np.float64 and np.array_equal(got["beta"].view(np.uint64), want["beta"].view(np.uint64))
    assert int(got["count"].sum()) == rep.nrow
    assert got.bed == rep.bed and got.levels == rep.levels and got.pattern_levels == rep.pattern_levels


def digest(reps):
    """One hash over every column of a list of Reports (what the hook runs in a child process are compared by)."""
    h = hashlib.sha1()
    for rep in reps:
        h.update(b"|%d|" % rep.nrow)
        for k in rep:
            h.update(k.encode())
            v = rep[k]
            h.update("\n".join(v).encode() if k == "pattern" else np.ascontiguousarray(v).tobytes())
    return h.hexdigest()


def stats(ea, bam):
    g, p, f = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    ea._lib.check(ea._lib.load().epi_batch_summarise_patterns_stats(bam.batch(), C.byref(g), C.byref(p), C.byref(f)))
    return g.value, p.value, f.value


# ---- 1. the reference's extractPatterns calls --------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(TP.CALLS))
def test_fixture_calls(ea, name):
    kw = dict(TP.CALLS[name])
    bam, bed, row = os.path.join(BAM, kw.pop("bam")), kw.pop("bed"), kw.pop("bed_row", 1)
    bedp = bed if ":" in bed else os.path.join(BAM, bed)
    pb = ea.preprocessBam(bam)
    got = ea.summarisePatterns(pb, bedp, bed_rows=[row], **kw)
    assert len(got) == 1
    same_summary(got[0], ea.extractPatterns(pb, bedp, bed_row=row, **kw))
    assert stats(ea, pb)[0] == 1 and stats(ea, pb)[2] == 0        # the batched path, grouped on the device
    # (patterns, unique, largest count) of the call, recomputed from the CPU oracle
    o = TP.oracle_patterns(**TP.CALLS[name])
    groups = {}
    for i, p in enumerate(o["pattern"]):
        key = (p, o["cells"][:, i].tobytes())
        groups[key] = groups.get(key, 0) + 1
    assert len(groups) == len(set(o["pattern"]))                   # here the hash alone gives the same groups
    assert (int(got[0]["count"].sum()), got[0].nrow, int(got[0]["count"].max())) == (len(o["pattern"]), len(groups), max(groups.values()))


def test_every_row_of_the_capture_bed(ea):
    pb = ea.preprocessBam(os.path.join(BAM, "capture.bam"))
    bedp = os.path.join(BAM, "capture.bed")
    got = ea.summarisePatterns(pb, bedp)
    want = ea.extractPatternsBed(pb, bedp)
    assert len(got) == len(want) == 565
    for g, w in zip(got, want):
        same_summary(g, w)
    assert sum(g.nrow for g in got) > 2000


# ---- 2. a synthetic pile-up ----------------------------------------------------------------------------------------------

def pile_up(seed=3):
    """~5000 rows of 60 bytes at chrA:1000, both strands, from 40 XM strings: string 0 on 3200 rows, 600 of them in one
    run (whole waves and workgroups of one key), six strings once somewhere and one once as the very last row, two strings
    without any context byte, the rest spread at random."""
    rng = np.random.default_rng(seed)
    base = np.array(list("." * 60))
    base[rng.choice(60, 14, replace=False)] = list("zZzZzZzZxXhHzZ")
    strings = ["".join(base)]
    while len(strings) < 38:
        s = base.copy()
        for p in rng.choice(60, int(rng.integers(1, 4)), replace=False):
            s[p] = rng.choice(list("zZxXhH.")) if s[p] == "." else {"z": "Z", "Z": "z", "x": "X", "X": "x", "h": "H", "H": "h"}[s[p]]
        s = "".join(s)
        if s not in strings:
            strings.append(s)
    strings += ["." * 60, "-" * 60]                     # no context byte in any context
    body = [0] * 2600 + list(rng.integers(8, 38, size=1700)) + [38] * 60 + [39] * 40
    rng.shuffle(body)
    body[1000:1000] = [0] * 600
    for k, at in zip(range(1, 7), sorted(rng.choice(len(body), 6, replace=False))):
        body.insert(int(at), k)
    body.append(7)
    strand = [1 if j == 0 else int(rng.integers(1, 3)) for j in body]
    assert body.count(0) >= 3000 and all(body.count(k) == 1 for k in range(1, 8)) and body[-1] == 7 and len(body) > 5000
    return H.templates_from_xm([strings[j] for j in body], [1000] * len(body), strand)


@pytest.fixture(scope="module")
def pile(ea):
    t = pile_up()
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"], levels=LEVELS)
    bed = ea.Bed(["chrA", "chrA", "chrB"], [1000, 1010, 1000], [1059, 1069, 1059])
    yield bam, bed
    bam.close()


PILE_ROWS = [1, 1, 2, 3, 99]           # the window, the same again, shifted by 10, a contig without rows, outside the BED
PILE_KW = [dict(), dict(clip_patterns=True), dict(highlight_positions=[1005, 1030, 1064]),
           dict(extract_context="CG", strand_offset=1, bin_context="CX"), dict(extract_context="CX", clip_patterns=True),
           dict(extract_context="CX", bin_context="CG"), dict(extract_context="CxG", bin_context="CHH", highlight_positions=[1012])]


@pytest.mark.parametrize("freq", [0.01, 0.5])
@pytest.mark.parametrize("kw", PILE_KW, ids=lambda kw: ",".join("%s=%s" % it for it in kw.items()) or "default")
def test_pile_up(ea, pile, kw, freq):
    bam, bed = pile
    got = ea.summarisePatterns(bam, bed, bed_rows=PILE_ROWS, min_context_freq=freq, **kw)
    assert len(got) == len(PILE_ROWS) and stats(ea, bam)[0] >= 1 and stats(ea, bam)[2] == 0
    ekw = {k: v for k, v in kw.items() if k != "bin_context"}
    reps = {r: ea.extractPatterns(bam, bed, bed_row=r, min_context_freq=freq, **ekw) for r in set(PILE_ROWS)}
    for r, g in zip(PILE_ROWS, got):
        same_summary(g, reps[r], kw.get("bin_context", "CG"))
        assert (int(g["count"].sum()) if g else 0) == reps[r].nrow
    assert not got[3] and not got[4] and not hasattr(got[4], "bed")
    assert int(got[0]["count"].max()) >= 3000 and got[0].nrow < reps[1].nrow
    if freq == 0.5:                                                # columns dropped: different reads collapse to equal cells
        loose = ea.summarisePatterns(bam, bed, bed_rows=[1], min_context_freq=0.01, **kw)[0]
        assert got[0].nrow < loose.nrow and len(position_columns(got[0])) < len(position_columns(loose))


def test_pile_up_with_colliding_keys(ea, pile, hook_env):
    """EPIHIP_PAT_HASH_BITS=3: at most eight keys per target, so different patterns meet in one table entry, the verify
    pass flags the target and the host groups it by (hash, cells): the same tables."""
    bam, bed = pile
    plain = ea.summarisePatterns(bam, bed, bed_rows=PILE_ROWS, extract_context="CX")
    assert stats(ea, bam)[2] == 0
    hook_env("EPIHIP_PAT_HASH_BITS", "3")
    hooked = ea.summarisePatterns(bam, bed, bed_rows=PILE_ROWS, extract_context="CX")
    assert stats(ea, bam)[2] == 3                                  # rows 1, 1 and 2
    assert digest(hooked) == digest(plain)
    for r, g in zip(PILE_ROWS, hooked):
        same_summary(g, ea.extractPatterns(bam, bed, bed_row=r, extract_context="CX"))


def summarise_launches(ea, fn):
    """fn() with the profiler on -> (its result, "summarise_patterns" sequences: one per batch of results)"""
    lib = ea._lib.load()
    lib.epi_prof_reset()
    lib.epi_prof_enable(1)
    try:
        res = fn()
    finally:
        lib.epi_prof_enable(0)
    n = C.c_int64(0)
    lib.epi_prof_get(b"summarise_patterns", None, C.byref(n))
    return res, n.value


# the pile-up's windows, the empty contig between them: six deep targets of ~5000 slots each
BATCH_ROWS = [1, 2, 3, 1, 1, 99, 2, 3, 2]


def planned_cuts(needs, cap):
    """include/epihip.h, Memory: consecutive targets share a group (a batch of results) while their needs stay under the
    cap, and a target above it runs alone -> the cuts as lists of target indices"""
    out, total = [[]], 0
    for k, need in enumerate(needs):
        if out[-1] and total > 0 and total + need > cap:
            out.append([])
            total = 0
        out[-1].append(k)
        total += need
    return out


@pytest.mark.parametrize("bits", [None, "3"])
@pytest.mark.parametrize("per_batch", [1, 2])
def test_several_batches_of_results_in_one_group(ea, pile, hook_env, per_batch, bits):
    """A cap between the deep targets' pass-1 need and their result need, so that a group of several targets is cut into
    several batches of results, of one or of two deep targets: the later batches start at a target, a slot, a cell and a
    table entry other than 0.  The expected groups and batches restate the header's Memory paragraph: pass 1 takes 40 B
    per candidate row + 8 B per window position + 128 B; the results 64 B per slot, 8 B per cell and 16 B per table entry."""
    bam, bed = pile
    rows = [r for r in BATCH_ROWS if r <= 3]
    reps = {r: ea.extractPatterns(bam, bed, bed_row=r) for r in set(rows)}
    slots = {1: bam.n, 2: bam.n, 3: 0}                             # every row overlaps both windows, none is on chrB
    tcap = 8
    while tcap < 2 * bam.n:
        tcap *= 2
    pass1 = [40 * slots[r] + 8 * (59 + 2 * 60 + 1 + 8) + 128 for r in rows]
    result = [(64 + 8 * len(position_columns(reps[r]))) * slots[r] + 16 * tcap if slots[r] else 0 for r in rows]
    cap = per_batch * max(result) + 4096
    assert 3 * max(pass1) < cap < (per_batch + 1) * min(x for x in result if x)
    groups = planned_cuts(pass1, cap)
    batches = [b for g in groups for b in planned_cuts([result[k] for k in g], cap) if any(result[g[k]] for k in b)]
    assert len(batches) > len(groups)
    plain = ea.summarisePatterns(bam, bed, bed_rows=BATCH_ROWS)
    hook_env("EPIHIP_PAT_GROUP_BYTES", str(cap))
    if bits:
        hook_env("EPIHIP_PAT_HASH_BITS", bits)
    got, launches = summarise_launches(ea, lambda: ea.summarisePatterns(bam, bed, bed_rows=BATCH_ROWS))
    st = stats(ea, bam)
    print("cap", cap, "groups", st[0], "of", len(groups), "batches", launches, "of", len(batches), "fallback", st[2])
    assert st[0] == len(groups) and launches == len(batches) and launches > st[0]
    assert st[2] == (6 if bits else 0)                             # every deep target, those of the later batches included
    assert digest(got) == digest(plain)
    for r, g in zip(BATCH_ROWS, got):
        same_summary(g, reps[r] if r <= 3 else ea.extractPatterns(bam, bed, bed_row=r))


# ---- 3. small targets: table slices at the minimum capacity ------------------------------------------------------------

def test_targets_with_3_and_70_slots_and_many_small_ones(ea):
    rng = np.random.default_rng(5)
    letters = list("zZ")
    xm, start = [], []
    for at, n in [(1000, 3), (2000, 70)] + [(3000 + 100 * k, 4) for k in range(30)]:
        seen = set()
        while len(seen) < n:                                       # n different patterns at one start
            seen.add("".join(rng.choice(letters, 12)))
        xm += sorted(seen)
        start += [at] * n
    t = H.templates_from_xm(xm, start, [1] * len(xm))
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"], levels=LEVELS)
    try:
        bed = ea.Bed(["chrA"] * 32, [1000, 2000] + [3000 + 100 * k for k in range(30)], [1011, 2011] + [3011 + 100 * k for k in range(30)])
        got = ea.summarisePatterns(bam, bed, extract_context="CG", strand_offset=0, min_context_freq=0)
        assert stats(ea, bam) == (1, len(xm), 0)
        assert [g.nrow for g in got] == [3, 70] + [4] * 30
        for r, g in enumerate(got):
            same_summary(g, ea.extractPatterns(bam, bed, bed_row=r + 1, extract_context="CG", strand_offset=0, min_context_freq=0))
            assert np.all(g["count"] == 1)
        # A probe wraps around the end of a slice when more keys have their home in the slice's last j entries than j
        # (whatever the order of insertion).  The home is pat_probe's in csrc/patterns.hip: the high half of
        # key x 0x9E3779B97F4A7C15, masked to the capacity (the power of two >= 2 x slots, 8 at the least).
        def wraps(g):
            cap = 8
            while cap < 2 * g.nrow:
                cap *= 2
            home = [(((int(p, 16) * 0x9E3779B97F4A7C15) & (2 ** 64 - 1)) >> 32) & (cap - 1) for p in g["pattern"]]
            return any(sum(h >= cap - j for h in home) > j for j in range(1, cap))
        assert sum(wraps(g) for g in got) >= 1
    finally:
        bam.close()


# ---- 4. unsorted rows ------------------------------------------------------------------------------------------------------

def unsorted_pile_up(ea):
    """The rows of pile_up(seed=9) and 80 more at chrA:5000, in a random order"""
    t = pile_up(seed=9)
    n = len(t["start"])
    far = H.templates_from_xm(["zZ.zZ" * 12] * 50 + ["Zz.zz" * 12] * 30, [5000] * 80, [1] * 80)
    rows = [t["xm"][t["off"][i]:t["off"][i + 1]] for i in range(n)] + [far["xm"][far["off"][i]:far["off"][i + 1]] for i in range(80)]
    start = np.concatenate([t["start"], far["start"]]); strand = np.concatenate([t["strand"], far["strand"]])
    perm = np.random.default_rng(1).permutation(n + 80)
    off = np.zeros(n + 81, np.int64)
    np.cumsum([rows[i].size for i in perm], out=off[1:])
    return ea.ProcessedBam.from_arrays(np.concatenate([rows[i] for i in perm]), off, np.ones(n + 80, np.int32), strand[perm], start[perm],
                                       levels=LEVELS)


def test_unsorted_rows_take_the_target_by_target_path(ea):
    bam = unsorted_pile_up(ea)
    try:
        bed = ea.Bed(["chrA", "chrA", "chrB"], [1000, 5000, 1000], [1059, 5059, 1059])
        got = ea.summarisePatterns(bam, bed, bed_rows=[2, 1, 3, 1])
        assert stats(ea, bam) == (0, 0, 3)                         # no group ran; three targets with patterns, grouped on the host
        for r, g in zip([2, 1, 3, 1], got):
            same_summary(g, ea.extractPatterns(bam, bed, bed_row=r))
        assert got[0].nrow == 2 and sorted(got[0]["count"]) == [30, 50] and int(got[1]["count"].max()) >= 3000 and not got[2]
    finally:
        bam.close()


def test_twenty_targets_of_the_target_by_target_path(ea):
    """One scratch serves the whole list: every target's summary is that of its own extractPatterns call"""
    bam = unsorted_pile_up(ea)
    try:
        # windows over the pile-up and the far rows, gaps without a row, and chrB
        starts = [940 + 10 * k for k in range(14)] + [3000, 4990, 5000, 5059, 5060, 1000]
        bed = ea.Bed(["chrA"] * 19 + ["chrB"], starts, [s + 24 for s in starts])
        got = ea.summarisePatterns(bam, bed)
        reps = [ea.extractPatterns(bam, bed, bed_row=r + 1) for r in range(20)]
        nonempty = sum(bool(rep) for rep in reps)
        assert len(got) == 20 and 10 <= nonempty < 20
        assert stats(ea, bam) == (0, 0, nonempty)
        for g, rep in zip(got, reps):
            same_summary(g, rep)
    finally:
        bam.close()


# ---- 5. the hooks, in a fresh process -------------------------------------------------------------------------------------

def worker_reports(ea):
    """What _patterns_summary_worker.py summarises: both fixtures' BEDs, with two sets of arguments."""
    out = []
    for bam, bed in (("capture.bam", "capture.bed"), ("amplicon010meth.bam", "amplicon.bed")):
        pb = ea.preprocessBam(os.path.join(BAM, bam))
        for kw in ({}, {"clip_patterns": True, "extract_context": "CX", "highlight_positions": [43125000, 61864584]}):
            out.append((ea.summarisePatterns(pb, os.path.join(BAM, bed), **kw), stats(ea, pb)))
    return out


@pytest.fixture(scope="module")
def plain_digests(ea):
    for k in ("EPIHIP_PAT_GROUP_BYTES", "EPIHIP_PAT_HASH_BITS"):
        assert k not in os.environ
    runs = worker_reports(ea)
    assert all(st[0] == 1 and st[2] == 0 for _, st in runs)
    return [digest(reps) for reps, _ in runs]


@pytest.mark.parametrize("hook,value", [("EPIHIP_PAT_GROUP_BYTES", "20000"), ("EPIHIP_PAT_HASH_BITS", "3")])
def test_hooks_are_result_neutral(plain_digests, hook, value):
    e = dict(os.environ)
    e[hook] = value
    r = subprocess.run([sys.executable, os.path.join(HERE, "_patterns_summary_worker.py")], env=e, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("summary ")]
    assert len(lines) == 4
    assert [ln[1] for ln in lines] == plain_digests
    groups, fallback = [int(ln[2]) for ln in lines], [int(ln[4]) for ln in lines]
    if hook == "EPIHIP_PAT_GROUP_BYTES":
        assert groups[0] >= 10 and groups[1] >= 10 and fallback == [0, 0, 0, 0]   # capture.bed: a few targets per group
    else:
        assert groups == [1, 1, 1, 1] and all(f > 0 for f in fallback)


# ---- 6. profiling ---------------------------------------------------------------------------------------------------------

def test_profiler_counts_the_summary_launches(ea, pile):
    bam, bed = pile
    lib = ea._lib.load()

    def launches(fn):
        lib.epi_prof_reset()
        lib.epi_prof_enable(1)
        try:
            fn()
        finally:
            lib.epi_prof_enable(0)
        n = C.c_int64(0)
        lib.epi_prof_get(b"summarise_patterns", None, C.byref(n))
        return n.value
    assert launches(lambda: ea.summarisePatterns(bam, bed)) == 1                           # one group, one batch of results
    assert launches(lambda: ea.summarisePatterns(bam, ea.Bed(["chrB", "chrA"], [1000, 9000], [1059, 9059]))) == 0
