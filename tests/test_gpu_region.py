"""generateRegionReport on the GPU (epi_batch_region_report_dev) against the loop restatement of its definitions
(tests/region_np.py): integers equal, doubles bit for bit -- on the reference's fixtures, against a recomputation from
extractPatternsBed, at the seams of the definitions on crafted rows, in both accumulation regimes and both row shapes, on fuzz
batches, over several counter groups, with errors and ownership pinned, and composed with generateHaplotypeBlocks."""
import contextlib
import ctypes as C
import functools
import gc
import os

import numpy as np
import pytest

import helpers as H
import region_np as RN
import synth_np

pytestmark = pytest.mark.gpu
BAM = os.path.join(H.GOLDEN, "bam")
LEVELS = ("chrA", "chrB", "chrC")
FIXTURES = {"capture": ("capture.bam", "capture.bed"), "amplicon": ("amplicon010meth.bam", "amplicon.bed")}


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


def make(ea, t):
    return ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"], LEVELS)


def check(ea, t, regions, context="CG", bam=None, label="", **kw):
    """rcpp_region_report on the batch of t against the restatement -> the restatement's table"""
    arg = dict(min_sites=4, max_sites=64, reverse_offset=RN.default_offset(context), u_max=0.25, m_min=0.75, max_oo=0.1)
    arg.update(kw)
    ctx = RN.ctx_letters(context)
    own = bam is None
    bam = make(ea, t) if own else bam
    try:
        got = ea.rcpp_region_report(bam, regions, ctx, arg["min_sites"], arg["max_sites"], arg["reverse_offset"], arg["u_max"], arg["m_min"],
                                    arg["max_oo"])
    finally:
        if own:
            bam.close()
    want = RN.restate(t, regions, ctx, **arg)
    assert list(got.keys()) == list(RN.COLUMNS)
    RN.same(got, want, label)
    return want


# ---- 1. the fixtures --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def fixture_bam(which):
    import epialleler_amd as ea
    return ea.preprocessBam(os.path.join(BAM, FIXTURES[which][0]))


@functools.lru_cache(maxsize=None)
def fixture_regions(which):
    import epialleler_amd as ea
    bed = ea.readBed(os.path.join(BAM, FIXTURES[which][1]))
    return RN.bed_regions(fixture_bam(which).levels, bed.chrom, bed.start, bed.end)


@functools.lru_cache(maxsize=None)
def fixture_want(which, kw):
    """The restatement's table of a fixture (computed once per argument set; read-only)"""
    kw = dict(kw)
    arg = dict(min_sites=kw.get("min_sites", 4), max_sites=kw.get("max_sites", 64), reverse_offset=1, max_oo=kw.get("max_outofcontext_beta", 0.1))
    return RN.restate(fixture_bam(which).host, fixture_regions(which), "Zz", **arg)


FIXTURE_ARGS = [{}, dict(max_outofcontext_beta=1.0), dict(max_sites=16), dict(min_sites=1), dict(min_sites=8)]


@pytest.mark.parametrize("kw", FIXTURE_ARGS, ids=lambda kw: ",".join("%s=%s" % it for it in kw.items()) or "defaults")
@pytest.mark.parametrize("which", ["capture", "amplicon"])
def test_fixtures(ea, which, kw):
    pb = fixture_bam(which)
    got = ea.generateRegionReport(pb, os.path.join(BAM, FIXTURES[which][1]), **kw)
    want = fixture_want(which, tuple(sorted(kw.items())))
    assert list(got.keys()) == list(ea.REGION_COLUMNS) and got.levels["rname"] == pb.levels
    RN.same(got, want, which)
    if which == "capture":
        assert pb.n == 2968 and got.nrow == 565
        if kw == dict(max_outofcontext_beta=1.0):          # the counts of the fixture with the read rule off
            assert (want["nreads"] > 0).sum() >= 479 and (want["kreads"] > 0).sum() >= 371 and (want["ndiscordant"] > 0).sum() >= 217
            assert want["maxsites"].max() == 39
        if kw == dict(max_sites=16):
            assert want["nlong"].max() > 0
        assert (want["kreads"] > 0).sum() > 100 and (want["ndiscordant"] > 0).sum() > 50
    else:
        assert got.nrow == 4 and np.all(want["kreads"] > 0) and want["nreads"].max() <= 238
        assert np.all(want["ndiscordant"] > 0) or "max_sites" in kw          # (reads of 17 to 19 sites are long at max_sites = 16)


# ---- 2. against extractPatternsBed --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["capture", "amplicon"])
def test_against_extract_patterns(ea, which):
    """With the read rule off, the columns recomputed from extractPatternsBed(clip_patterns=False, min_context_freq=0): every
    table's position columns inside the region, the calls of a pattern row in position order, runs per row.  extractPatterns
    takes the rows whose own span [start, start + len) overlaps the target; a reverse-strand row that starts up to
    strand_offset behind the region's end can have a call inside it and is no pattern row, so the regions with such a row
    are left out here (the capture fixture has no such region)."""
    pb = fixture_bam(which)
    bedp = os.path.join(BAM, FIXTURES[which][1])
    chrom, rs, re_ = fixture_regions(which)
    got = ea.generateRegionReport(pb, bedp, max_outofcontext_beta=1.0)
    reps = ea.extractPatternsBed(pb, bedp, clip_patterns=False, min_context_freq=0, strand_offset=1)
    t = pb.host
    compared = 0
    for g, rep in enumerate(reps):
        behind = (t["rname"] == chrom[g]) & (t["strand"] == 2) & (t["start"] > re_[g]) & (t["start"] <= re_[g] + 1)
        if behind.any():
            continue
        compared += 1
        rows = []
        if rep:
            pos = sorted(int(k) for k in rep if k.lstrip("-").isdigit() and rs[g] <= int(k) <= re_[g])
            cells = np.stack([rep[str(p)] for p in pos], axis=1) if pos else np.zeros((rep.nrow, 0), np.int32)
            rows = [[bool(c < 8) for c in row[row != H.NA_INT]] for row in cells]
        c, d, _ = RN.region_row(rows, 4, 64, 0.25, 0.75)
        for k, v in c.items():
            assert got[k][g] == v, (g, k)
        for k, v in d.items():
            assert np.float64(v).view(np.uint64) == got[k][g:g + 1].view(np.uint64)[0], (g, k)
    assert compared >= 0.9 * len(reps) and (got["kreads"] > 0).sum() >= (4 if which == "amplicon" else 371)


# ---- 3. seams ---------------------------------------------------------------------------------------------------------------

def test_seams_of_a_region(ea):
    """Calls exactly at start and end; the reverse strand's offset at the end; a run cut at either end of the clip; the read
    rule; a region without a row, on another sequence, on an absent one; repeated, nested and descending regions."""
    xms = ["Z....z", "Z", "Z", "zZZZzzZZZz", "ZzZzHHH", "z.z", "Z..z"]
    starts = [10, 16, 17, 30, 50, 10, 100]
    strands = [1, 2, 2, 1, 1, 2, 1]
    t = H.templates_from_xm(xms, starts, strands, rnames=[1, 1, 1, 1, 1, 1, 2])
    regions = ([1, 1, 1, 1, 1, 1, 1, 1, 2, 3, H.NA_INT, 1, 1, 1],
               [10, 11, 15, 16, 32, 50, 60, 1, 100, 100, 10, 10, 12, 10],
               [15, 14, 15, 16, 37, 56, 70, 200, 103, 103, 15, 15, 13, 15])
    w = check(ea, t, regions, min_sites=1)
    # 10-15: "Z....z" gives Z at 10 and z at 15; the '-' row "Z" at 16 is at 15 (in), the one at 17 at 16 (out); "z.z"- is at 9 and 11
    assert (w["nreads"][0], w["tbase"][0], w["mbase"][0]) == (3, 4, 2)
    assert w["nreads"][1] == 1 and w["tbase"][1] == 1                   # 11-14: the z at 11 alone
    assert (w["nreads"][2], w["tbase"][2]) == (2, 2) and (w["nreads"][3], w["tbase"][3], w["mbase"][3]) == (1, 1, 1)
    assert (w["tbase"][4], w["mbase"][4], w["maxsites"][4]) == (6, 4, 6) and w["mbs"][4] == (4 + 4) / 36    # ZZ zz ZZ: both runs cut
    assert w["nreads"][5] == 0 and np.isnan(w["mhl"][5])                 # the row there is dropped by the read rule
    assert w["nreads"][6] == 0 and w["nreads"][7] == 5 and w["nreads"][8] == 1 and w["nreads"][9] == 0 and w["nreads"][10] == 0
    assert w["rname"][10] == H.NA_INT
    for k in RN.COLUMNS[3:]:
        assert w[k].view(np.uint64 if w[k].dtype == np.float64 else np.int32)[0] == w[k].view(np.uint64 if w[k].dtype == np.float64 else np.int32)[11], k
    check(ea, t, regions, max_oo=1.0, min_sites=2)
    check(ea, t, tuple(a[::-1] for a in regions), min_sites=1, label="descending")
    check(ea, t, regions, context="CX", min_sites=1, reverse_offset=0)


@pytest.mark.parametrize("max_sites", [1, 64, 256])
def test_seams_of_the_site_limits(ea, max_sites):
    """n = max_sites and max_sites + 1 (the second row is long: in nlong and nowhere else), n = min_sites - 1 and min_sites"""
    rng = np.random.default_rng(max_sites)
    pat = lambda n: "".join("Z" if v else "z" for v in rng.random(n) < 0.6)
    xms = [pat(max_sites), pat(max_sites + 1), "Z" * max_sites, "Z" * (max_sites + 1), "z.Z" * 2, "Zz.ZZ"]
    xms = [".".join(x) if i == 0 else x for i, x in enumerate(xms)]        # (one row with gaps between its calls)
    t = H.templates_from_xm(xms, [5] * len(xms), [1] * len(xms))
    min_sites = min(4, max_sites)
    w = check(ea, t, ([1], [1], [2000]), min_sites=min_sites, max_sites=max_sites)
    if max_sites >= 4:
        assert (w["nreads"][0], w["nlong"][0], w["kreads"][0], w["maxsites"][0]) == (6, 2, 4, max_sites)
    else:
        assert (w["nreads"][0], w["nlong"][0], w["kreads"][0], w["maxsites"][0]) == (6, 4, 2, 1)
    w = check(ea, t, ([1], [1], [2000]), min_sites=max_sites, max_sites=max_sites)
    assert w["kreads"][0] == 2
    if max_sites == 64:
        w = check(ea, t, ([1, 1], [5, 5], [8, 9]), min_sites=4)              # "Zz.ZZ" cut to 3 calls and to 4; the gapped row has 2 and 3
        assert w["kreads"].tolist() == [3, 4] and w["nreads"].tolist() == [6, 6]


def test_seams_of_the_uxm_thresholds(ea):
    """m exactly on either threshold: 1 of 4 at 0.25 is U, 3 of 4 at 0.75 is M; and the products that are not exact"""
    xms = ["Zzzz", "ZZZz", "ZZzz", "zzzz", "ZZZZ", "Zzz", "ZZz", "Zzzzzzzzzz", "ZZZZZZZzzz"]
    t = H.templates_from_xm(xms, [1] * len(xms), [1] * len(xms))
    w = check(ea, t, ([1], [1], [20]), min_sites=3)
    assert (w["n_u"][0], w["n_x"][0], w["n_m"][0]) == (3, 4, 2)
    for u, m in ((0.0, 1.0), (0.1, 0.7), (1 / 3, 2 / 3), (0.3, 0.30000000000000004), (0.0, 1e-9)):
        check(ea, t, ([1], [1], [20]), min_sites=3, u_max=u, m_min=m)


def test_no_region_and_no_row(ea):
    t = H.templates_from_xm(["Z.z.Z"], [1], [1])
    w = check(ea, t, ([], [], []))
    assert all(w[k].size == 0 for k in RN.COLUMNS)
    empty = H.templates_from_xm([], [], [])
    w = check(ea, empty, ([1, 2, H.NA_INT], [1, 5, 1], [10, 2, 10]))
    assert w["nreads"].tolist() == [0, 0, 0] and np.all(np.isnan(w["beta"])) and w["start"].tolist() == [1, 5, 1]
    check(ea, empty, ([], [], []))


# ---- 4. accumulation regimes and row shapes ------------------------------------------------------------------------------------

def cpg_batch(rng, nrow, length, span, every=6, p_meth=0.5, rnames=1, other=""):
    """Rows of `length` bases with a CpG at every position that is a multiple of `every`, ragged starts in [1, span]"""
    starts = np.sort(rng.integers(1, span + 1, nrow))
    letters = np.frombuffer(("Zz." + other).encode(), np.uint8)
    xms = []
    for st in starts:
        pos = np.arange(st, st + length)
        row = np.where(pos % every == 0, np.where(rng.random(length) < p_meth, letters[0], letters[1]), letters[2])
        if other:
            o = rng.random(length) < 0.02
            row = np.where(o & (pos % every != 0), letters[3 + rng.integers(0, len(other), length)], row)
        xms.append(row.astype(np.uint8).tobytes().decode())
    return H.templates_from_xm(xms, starts.tolist(), rng.integers(1, 3, nrow).tolist(), rnames=np.sort(rng.integers(1, rnames + 1, nrow)).tolist())


def test_deep_region_many_workgroups(ea):
    """20 000 rows of 60 bytes on one region (many workgroups add to its counters) between two regions over a part of them,
    whose pair counts are odd: the boundaries between the regions' pairs fall inside a chunk of pairs, whatever its size"""
    rng = np.random.default_rng(1)
    t = cpg_batch(rng, 20000, 60, 40, other="xh")
    mid = int(np.median(t["start"]))
    assert (t["start"] >= mid + 48 - 59).sum() % 2 == 1 and (t["start"] >= mid + 49 - 59).sum() % 2 == 1     # their candidate rows
    w = check(ea, t, ([1, 1, 1], [mid + 48, 1, mid + 49], [200, 200, 200]))   # (a row reaches start + 59: its calls there, if any)
    assert w["nreads"][1] == 20000 and 3000 < w["nreads"][0] < 17000 and w["kreads"][0] > 1000 and w["kreads"][2] > 1000


def test_one_row_per_region_and_alternating_depths(ea):
    rng = np.random.default_rng(2)
    xms = ["".join(rng.choice(list("Zz"), 8)) for _ in range(64)]
    t = H.templates_from_xm(xms, [100 * i + 1 for i in range(64)], [1] * 64)
    w = check(ea, t, ([1] * 64, [100 * i + 1 for i in range(64)], [100 * i + 50 for i in range(64)]))
    assert w["nreads"].tolist() == [1] * 64 and w["kreads"].tolist() == [1] * 64
    # regions of 1 row and of 300 rows in turn
    xms, starts, regs = [], [], ([], [], [])
    for i in range(12):
        for _ in range(1 if i % 2 == 0 else 300):
            xms.append("".join(rng.choice(list("Zz."), 30, p=[0.2, 0.2, 0.6])))
            starts.append(1000 * i + 1 + int(rng.integers(0, 5)))
        regs[0].append(1); regs[1].append(1000 * i + 1); regs[2].append(1000 * i + 40)
    t = H.templates_from_xm(xms, starts, rng.integers(1, 3, len(xms)).tolist())
    w = check(ea, t, regs, min_sites=2)
    assert w["nreads"][0::2].max() <= 1 and w["nreads"][1::2].min() > 250


def test_long_rows_under_short_regions(ea):
    """Rows of 3000 bytes (a wave per pair) under regions of 40 bases, at the rows' ends and in their middle"""
    rng = np.random.default_rng(3)
    t = cpg_batch(rng, 60, 3000, 500, every=5, other="xhhhhhhhhH")            # (the read rule drops about half of the rows)
    assert t["off"][-1] > 512 * 60 and 20 < H.mhl_keep_np(t["xm"], t["off"], "Zz", 0, 0.1).sum() < 40
    st = [1, 300, 480, 501, 1500, 2990, 3400, 3490, 3600]
    w = check(ea, t, ([1] * len(st), st, [s + 39 for s in st]), min_sites=2)
    assert w["nreads"][4] > 30 and w["maxsites"].max() == 8 and w["nreads"][-1] == 0
    w = check(ea, t, ([1], [1], [4000]), max_sites=256, min_sites=1)          # every row is long: 600 calls
    assert w["nlong"][0] == w["nreads"][0] > 30 and w["maxsites"][0] == 0


def test_adopted_without_realignment_equals_uploaded(ea):
    import torch
    rng = np.random.default_rng(4)
    t = synth_np.random_templates(rng, 500, 1, 90, 2, 1500)
    regions = ([1, 2, 1, 2], [1, 1, 700, 400], [1500, 800, 900, 1600])
    ctx = RN.ctx_letters("CG")
    up = make(ea, t)
    nb = int(t["off"][-1])
    xm = torch.full(((nb + 15) // 16 * 16 + 64,), 0xFB, dtype=torch.uint8, device="cuda:0")
    xm[:nb] = torch.from_numpy(t["xm"]).cuda()
    dev = {k: torch.from_numpy(t[k]).cuda() for k in ("off", "rname", "strand", "start")}
    ad = ea.ProcessedBam.from_device(xm, nb, dev["off"], dev["rname"], dev["strand"], dev["start"], LEVELS, realign=False)
    try:
        a = ea.rcpp_region_report(up, regions, ctx, 2, 64, 1, 0.25, 0.75, 0.5)
        b = ea.rcpp_region_report(ad, regions, ctx, 2, 64, 1, 0.25, 0.75, 0.5)
        assert ea._lib.load().epi_batch_layout(ad.batch()) == 0 and ea._lib.load().epi_batch_layout(up.batch()) == 16
    finally:
        up.close()
        ad.close()
    RN.same(a, b, "adopted")
    RN.same(a, RN.restate(t, regions, ctx, min_sites=2, max_oo=0.5), "uploaded")
    assert a["kreads"].min() >= 20


# ---- 5. fuzz ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("context", ["CG", "CHG", "CHH", "CxG", "CX"])
@pytest.mark.parametrize("seed", [11, 12, 13])
def test_fuzz(ea, seed, context):
    rng = np.random.default_rng(1000 * seed + list(H.CONTEXT_TO_BASES).index(context))
    nseq = 2 + seed % 2
    t = synth_np.random_templates(rng, 400, 0, 300, nseq, 3000)
    chrom = rng.integers(1, nseq + 2, 50)                                   # (one code beyond the batch's)
    start = rng.integers(-50, 3300, 50)
    end = start + rng.integers(-2, 400, 50)
    kw = dict(min_sites=int(rng.integers(1, 6)), max_sites=int(rng.choice([6, 16, 64, 256])), max_oo=float(rng.choice([0.25, 0.5, 1.0])))     # (the letters are uniform: 0.1 keeps next to no row)
    kw["min_sites"] = min(kw["min_sites"], kw["max_sites"])
    w = check(ea, t, (chrom, start, end), context=context, **kw)
    assert (w["nreads"] > 0).sum() >= 5 and w["kreads"].max() > 0 and w["ndiscordant"].max() > 0    # (0.25 keeps few rows, the others most)


# ---- 6. groups --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", [20000, 1000])
def test_counter_groups(ea, hook_env, cap):
    """(3 * 64 + 16) * 8 + 16 = 1680 bytes per region: 11 regions per group under 20 000 bytes, and under 1000 bytes every region
    is above the cap and runs alone"""
    pb = fixture_bam("capture")
    bedp = os.path.join(BAM, FIXTURES["capture"][1])
    hook_env("EPIHIP_RGN_GROUP_BYTES", str(cap))
    got = ea.generateRegionReport(pb, bedp)
    RN.same(got, fixture_want("capture", ()), "cap %d" % cap)


# ---- 7. errors and ownership ------------------------------------------------------------------------------------------------

def allocations(ea):
    live, nbytes = C.c_int64(-1), C.c_int64(-1)
    ea._lib.check(ea._lib.load().epi_device_allocations(C.byref(live), C.byref(nbytes)))
    return live.value, nbytes.value


@contextlib.contextmanager
def nothing_left(ea):
    gc.collect()
    before = allocations(ea)
    yield
    gc.collect()
    assert allocations(ea) == before


def raw_call(ea, bam, regions, min_sites=4, max_sites=64, fill=-7):
    """epi_batch_region_report_dev on columns filled with a sentinel -> (return code, the columns)"""
    import torch
    from epialleler_amd.api import _ptr_array, _stream
    dev = "cuda:%d" % bam.device
    reg = [torch.tensor(np.asarray(r, np.int32), device=dev) for r in regions]
    n = len(regions[0])
    icols = list(torch.full((15, n), fill, dtype=torch.int32, device=dev).unbind(0))
    dcols = list(torch.full((6, n), float(fill), dtype=torch.float64, device=dev).unbind(0))
    rc = ea._lib.load().epi_batch_region_report_dev(bam.batch(), *[C.c_void_p(r.data_ptr()) for r in reg], n, b"Zz", min_sites, max_sites, 1,
                                                    0.25, 0.75, 0.1, _ptr_array(icols), _ptr_array(dcols), _stream(bam.device))
    torch.cuda.synchronize()
    return rc, [c.cpu().numpy() for c in icols + dcols]


def test_errors_and_ownership(ea):
    rng = np.random.default_rng(7)
    t = cpg_batch(rng, 300, 80, 800, rnames=2)
    regions = ([1, 2, 1], [100, 500, 300], [300, 600, 320])
    assert RN.restate(t, regions, "Zz")["kreads"].min() >= 10
    bam = make(ea, t)
    bam.batch()
    unsorted = make(ea, dict(t, start=t["start"][::-1].copy()))
    unsorted.batch()
    E = ea._lib
    try:
        with nothing_left(ea):
            rc, cols = raw_call(ea, bam, regions)
            assert rc == E.EPI_OK and cols[3].min() > 0 and not np.any(cols[0] == -7)
        with nothing_left(ea):
            for kw in (dict(min_sites=0), dict(min_sites=65), dict(max_sites=257), dict(max_sites=0, min_sites=1)):
                rc, cols = raw_call(ea, bam, regions, **kw)
                assert rc == E.EPI_ERR_ARG and all(np.all(c == -7) for c in cols), kw
            assert b"max_sites" in E.load().epi_last_error()
        with nothing_left(ea):
            rc, cols = raw_call(ea, unsorted, regions)
            assert rc == E.EPI_ERR_UNSORTED and b"PRE-SORTED" in E.load().epi_last_error()
            assert all(np.all(c == -7) for c in cols)
        with nothing_left(ea):
            with pytest.raises(ea.EpihipError) as ei:
                ea.rcpp_region_report(unsorted, regions, "Zz", 4, 64, 1, 0.25, 0.75, 0.1)
            assert ei.value.code == E.EPI_ERR_UNSORTED
            with pytest.raises(ea.EpihipError) as ei:
                ea.rcpp_region_report(bam, regions, "Zz", 4, 64, 1, 0.75, 0.25, 0.1)
            assert ei.value.code == E.EPI_ERR_ARG and "u_max" in str(ei.value)
    finally:
        bam.close()
        unsorted.close()


# ---- 8. composition ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("as_device", [False, True])
def test_blocks_as_regions(ea, as_device):
    """generateRegionReport(bam, generateHaplotypeBlocks(bam, ...)): the blocks as a host Report and as a device Report give
    what the same blocks give as a Bed"""
    import test_gpu_ownership as OWN
    t = OWN.cpg_rows(9)                                      # 300 rows of 80 bases, a CpG every 6 bases, two sequences
    bam = make(ea, t)
    try:
        blocks = ea.generateHaplotypeBlocks(bam, min_reads=2, min_r2=0.0, min_sites=2, as_device=as_device)
        nb = blocks.nrow
        assert nb >= 1
        got = ea.generateRegionReport(bam, blocks, min_sites=2)
        host = {k: (v.cpu().numpy() if as_device else v) for k, v in blocks.items()}
        bed = ea.Bed([LEVELS[r - 1] for r in host["rname"]], host["start"], host["end"])
        same_as = ea.generateRegionReport(bam, bed, min_sites=2)
        dev = ea.generateRegionReport(bam, blocks, min_sites=2, as_device=True)
    finally:
        bam.close()
    RN.same(got, same_as, "blocks")
    RN.same({k: v.cpu().numpy() for k, v in dev.items()}, same_as, "device table")
    RN.same(got, RN.restate(t, (host["rname"], host["start"], host["end"]), "Zz", min_sites=2), "restatement")
    assert got.nrow == nb and got["kreads"].max() > 0 and np.array_equal(got["start"], host["start"])
