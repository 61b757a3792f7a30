"""CX reports written by the tile kernel itself (direct mode): the first report on a batch goes through the row pool and
the gather, and the batch keeps its tile offsets; a second one with the same contexts gets columns of that size and the
tile kernel writes them at those offsets.  Both tables must be bitwise equal and equal to the oracle, over tile counts
that are and are not multiples of the eight XCDs, gaps between tiles, several reference sequences, ragged and gapped rows;
pile-ups and a capacity one row short must fall back to the pool and give the same table.  Tiles whose row count changed
since the kept report (the unused low nibbles under failed reads, rows rewritten in place) must fall back as well and
replace the record; alternating contexts keep one record at a time."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

C2B = H.CONTEXT_TO_BASES
CODES = np.frombuffer(b".......hhxzZHXuU", np.uint8)


@pytest.fixture(scope="module")
def ea():
    import epialleler_amd
    return epialleler_amd


@pytest.fixture
def hook_env(ea, monkeypatch):
    """Sets EPIHIP_* test hooks inside this process: the library reads its switches once, so it is told to re-read
    them after every change (epi_options_reload) and once more when the environment has been restored."""
    lib = ea._lib.load()

    def setenv(name, value):
        monkeypatch.setenv(name, value)
        lib.epi_options_reload()
    yield setenv
    monkeypatch.undo()
    lib.epi_options_reload()


def letters_to_xm(rng, ch):
    return (((rng.integers(0, 16, size=ch.size) << 4) | (((ch.astype(np.int64) + 2) >> 2) & 15))).astype(np.uint8)


def segments_batch(seed, segs, T, lens="uniform", depth=4):
    """Rows covering exactly the tiles [first, first + count) of reference sequence rname for every (rname, first, count) in
    `segs` (tiles of T positions on the absolute grid; segments of one rname in increasing order, gaps between them)."""
    rng = np.random.default_rng(seed)
    rn, st, ln = [], [], []
    for rname, first, count in segs:
        lo, hi = first * T, (first + count) * T               # positions [lo, hi)
        n = max(2, (hi - lo) * depth // 300)
        if lens == "uniform":
            L = np.full(n, 300)
        else:
            L = rng.integers(120, 481, size=n)
        s = rng.integers(lo, hi - L + 1)
        s[0], L[0] = lo, 300                                   # the first and the last position of the segment are covered
        L[-1] = 300
        s[-1] = hi - 300
        rn.append(np.full(n, rname)); st.append(s); ln.append(L)
    rname, start, L = np.concatenate(rn), np.concatenate(st), np.concatenate(ln)
    order = np.lexsort((start, rname))
    rname, start, L = rname[order].astype(np.int32), start[order].astype(np.int32), L[order]
    off = np.zeros(L.size + 1, np.int64)
    np.cumsum(L, out=off[1:])
    ch = CODES[rng.integers(0, CODES.size, size=int(off[-1]))]
    xm = letters_to_xm(rng, ch)
    if lens == "gapped":                                       # a 50-byte run of '+' (skipped) in every fourth row
        for r in range(0, L.size, 4):
            g0 = off[r] + L[r] // 2 - 25
            xm[g0:g0 + 50] = 0xFB
    strand = rng.integers(1, 3, size=L.size).astype(np.int32)
    return {"xm": xm, "off": off, "rname": rname, "strand": strand, "start": start}


def ntiles(ea, bam, ctx):
    lib = ea._lib.load()
    T = lib.epi_cx_tile_positions(C2B[ctx]["ctx_meth"].encode())
    k0, k1 = C.c_int64(0), C.c_int64(0)
    ea._lib.check(lib.epi_batch_tile_key_range_for(bam.batch(), T, None, C.byref(k0), C.byref(k1)))
    return k1.value - k0.value + 1


def report(ea, bam, ctx, fused, cap=None, letters=None, thr=(2, 0.5, 0.1), pass_=None):
    """One report through the C entry point that takes the caller's columns: (table, written).  ctx names the
    thresholding context of a fused report; letters are the report's contexts (default: ctx's methylated letters);
    thr = (min_n, min_beta, max_oo) of a fused report; pass_ = the int32 pass column of an unfused one (None: all TRUE)."""
    import torch
    lib = ea._lib.load()
    b = bam.batch()
    c = C2B[ctx]
    letters = (c["ctx_meth"] if letters is None else letters).encode()
    if cap is None:
        rec = C.c_int64(-1)
        ea._lib.check(lib.epi_batch_cx_report_capacity(b, letters, C.byref(rec)))
        cap = max(rec.value, 0)
    buf = torch.full((6, max(cap, 1)), -7, dtype=torch.int32, device="cuda:%d" % bam.device)
    cols = (C.c_void_p * 6)(*[t.data_ptr() for t in buf.unbind(0)])
    nrow, written = C.c_int64(0), C.c_int(0)
    stream = ea.api._stream(bam.device)
    if fused:
        rc = lib.epi_batch_cytosine_report_into_dev(b, c["ctx_meth"].encode(), c["ctx_unmeth"].encode(), c["ooctx_meth"].encode(),
                                                    c["ooctx_unmeth"].encode(), int(thr[0]), float(thr[1]), float(thr[2]), letters,
                                                    None, cols if cap else None, cap, stream, C.byref(nrow), C.byref(written))
    else:
        p = None if pass_ is None else torch.from_numpy(np.ascontiguousarray(pass_, np.int32)).to(buf.device)
        rc = lib.epi_batch_cx_report_into_dev(b, C.c_void_p(p.data_ptr()) if p is not None and bam.n else None, letters,
                                              cols if cap else None, cap, stream, C.byref(nrow), C.byref(written))
    ea._lib.check(rc)
    n = nrow.value
    if not written.value:
        if n > buf.shape[1]:
            buf = torch.empty((6, n), dtype=torch.int32, device=buf.device)
        if n:
            ea._lib.check(lib.epi_batch_cx_fetch_dev(b, (C.c_void_p * 6)(*[t.data_ptr() for t in buf.unbind(0)]), stream))
    torch.cuda.synchronize()
    names = ("rname", "strand", "pos", "context", "meth", "unmeth")
    return {k: buf[i, :n].cpu().numpy() for i, k in enumerate(names)}, bool(written.value)


def oracle(t, ctx, fused):
    c = C2B[ctx]
    if fused:
        p = orc.threshold_reads(t["xm"], t["off"], c["ctx_meth"], c["ctx_unmeth"], c["ooctx_meth"], c["ooctx_unmeth"], 2, 0.5, 0.1)
    else:
        p = np.ones(t["start"].size, np.int32)
    return orc.cx_report(t["xm"], t["off"], t["rname"], t["strand"], t["start"], p, c["ctx_meth"])


def pool_then_direct(ea, t, ctx, fused, expect_direct=True, want_tiles=None):
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"])
    try:
        if want_tiles is not None:
            assert ntiles(ea, bam, ctx) == want_tiles
        first, w1 = report(ea, bam, ctx, fused)
        assert not w1                                          # nothing recorded yet: the pool path
        second, w2 = report(ea, bam, ctx, fused)
        assert w2 == expect_direct
        H.assert_reports_equal(first, second)
        H.assert_reports_equal(second, oracle(t, ctx, fused))
        return bam, second
    finally:
        bam.close()


@pytest.mark.parametrize("ctx", ["CG", "CX"])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("count", [1, 5, 31, 32, 33, 63, 64, 65, 67, 129, 259])
def test_tile_counts(ea, ctx, fused, count):
    """A single tile, tile counts around multiples of 8 and of 32 (the tile order deals XCDs contiguous eighths)."""
    T = ea._lib.load().epi_cx_tile_positions(C2B[ctx]["ctx_meth"].encode())
    t = segments_batch(count, [(1, 3, count)], T)
    pool_then_direct(ea, t, ctx, fused, want_tiles=count)


@pytest.mark.parametrize("ctx", ["CG", "CX"])
@pytest.mark.parametrize("lens", ["uniform", "ragged", "gapped"])
def test_rows_and_gaps(ea, ctx, lens):
    """Several reference sequences, gaps between tile runs inside one, ragged and gapped rows; fused and unfused."""
    T = ea._lib.load().epi_cx_tile_positions(C2B[ctx]["ctx_meth"].encode())
    segs = [(1, 1, 40), (1, 45, 3), (1, 60, 70), (2, 7, 1), (2, 9, 90), (5, 100, 17)]
    t = segments_batch(("uniform", "ragged", "gapped").index(lens) + (10 if ctx == "CX" else 0), segs, T, lens=lens)
    for fused in (True, False):
        pool_then_direct(ea, t, ctx, fused)


def test_python_api_reports_twice(ea):
    """The Python entry points hand over their columns: the second report is written by the tile kernel, same table."""
    T = ea._lib.load().epi_cx_tile_positions(b"Z")
    t = segments_batch(7, [(1, 2, 70), (3, 0, 9)], T, lens="ragged")
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"])
    try:
        want = oracle(t, "CG", True)
        a = ea.generateCytosineReport(bam)
        b = ea.generateCytosineReport(bam)
        c = ea.generateCytosineReport(bam, as_device=True)
        H.assert_reports_equal(dict(a), want)
        H.assert_reports_equal(dict(b), want)
        H.assert_reports_equal({k: v.cpu().numpy() for k, v in dict(c).items()}, want)
        assert dict(c)["pos"].shape[0] == want["pos"].size
        d = ea.rcpp_cx_report(bam, None, "Z")
        e = ea.rcpp_cx_report(bam, None, "Z")
        H.assert_reports_equal(dict(d), dict(e))
        H.assert_reports_equal(dict(e), oracle(t, "CG", False))
    finally:
        bam.close()


def test_no_reportable_rows(ea):
    """Rows without a single call of the context: an empty table, on both calls."""
    rng = np.random.default_rng(3)
    n, L = 400, 200
    ch = np.frombuffer(b"......hhxx", np.uint8)[rng.integers(0, 10, size=n * L)]
    t = {"xm": letters_to_xm(rng, ch), "off": np.arange(n + 1, dtype=np.int64) * L, "rname": np.ones(n, np.int32),
         "strand": rng.integers(1, 3, size=n).astype(np.int32), "start": np.sort(rng.integers(1, 30000, size=n)).astype(np.int32)}
    for fused in (True, False):
        bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"])
        try:
            for _ in range(2):
                got, _w = report(ea, bam, "CG", fused)
                assert got["pos"].size == 0
                H.assert_reports_equal(got, oracle(t, "CG", fused))
        finally:
            bam.close()


@pytest.mark.parametrize("ctx", ["CG", "CX"])
def test_pileup_falls_back(ea, ctx):
    """Positions covered by more than 255 rows: deep tiles finish in later kernels, so the pool path runs again."""
    T = ea._lib.load().epi_cx_tile_positions(C2B[ctx]["ctx_meth"].encode())
    t = segments_batch(11, [(1, 0, 12)], T)
    rng = np.random.default_rng(12)
    k = 700                                                    # 700 rows starting at one position
    p = H.templates_from_xm(["".join(chr(c) for c in CODES[rng.integers(0, CODES.size, size=250)]) for _ in range(k)],
                            [5 * T + 100] * k, list(rng.integers(1, 3, size=k)), [1] * k)
    keys = np.concatenate([t["start"], p["start"]])
    order = np.argsort(keys, kind="stable")
    rows = [t["xm"][t["off"][i]:t["off"][i + 1]] for i in range(t["start"].size)] + \
           [p["xm"][p["off"][i]:p["off"][i + 1]] for i in range(p["start"].size)]
    rows = [rows[i] for i in order]
    off = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([r.size for r in rows], out=off[1:])
    m = {"xm": np.concatenate(rows), "off": off, "rname": np.ones(len(rows), np.int32),
         "strand": np.concatenate([t["strand"], np.asarray(p["strand"], np.int32)])[order],
         "start": keys[order].astype(np.int32)}
    for fused in (True, False):
        pool_then_direct(ea, m, ctx, fused, expect_direct=False)


@pytest.mark.parametrize("fused", [True, False])
def test_capacity_one_row_short_falls_back(ea, fused):
    T = ea._lib.load().epi_cx_tile_positions(b"Z")
    t = segments_batch(5, [(1, 1, 66)], T, lens="ragged")
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"])
    try:
        first, w1 = report(ea, bam, "CG", fused)
        assert not w1 and first["pos"].size > 1
        short, w2 = report(ea, bam, "CG", fused, cap=first["pos"].size - 1)
        assert not w2
        H.assert_reports_equal(first, short)
        full, w3 = report(ea, bam, "CG", fused)
        assert w3
        H.assert_reports_equal(first, full)
        H.assert_reports_equal(full, oracle(t, "CG", fused))
    finally:
        bam.close()


# ---- the per-tile count check: row counts that change between reports with the same contexts -------------------------

def tile_counts(tab, T):
    """Rows per tile of a table on the kernels' absolute grid (tiles.hip: tile = (pos + kPosBias) >> log2(T))."""
    key = (tab["rname"].astype(np.int64) << 32) | ((tab["pos"].astype(np.int64) + (1 << 31)) // T)
    u, c = np.unique(key, return_counts=True)
    return dict(zip(u.tolist(), c.tolist()))


def capacity(ea, bam, letters):
    rec = C.c_int64(-2)
    ea._lib.check(ea._lib.load().epi_batch_cx_report_capacity(bam.batch(), letters.encode(), C.byref(rec)))
    return rec.value


def garbage_batch(seed, nibbles, T, frac=0.3):
    """Rows of segments_batch with a fraction of the bytes' low nibbles replaced by codes the packer never produces:
    under a failed read nibble 1 adds coverage twice, 3 is skipped, 4 counts as '.' (rcpp_cx_report.cpp:122-127)."""
    t = segments_batch(seed, [(1, 1, 20), (2, 4, 9)], T)
    rng = np.random.default_rng(seed + 1)
    g = rng.random(t["xm"].size) < frac
    t["xm"][g] = ((t["xm"][g] & 0xF0) | rng.choice(np.asarray(nibbles, np.uint8), size=int(g.sum()))).astype(np.uint8)
    return t


def cx_oracle(t, p, letters):
    return orc.cx_report(t["xm"], t["off"], t["rname"], t["strand"], t["start"], p, letters)


@pytest.mark.parametrize("fused", [False, True])
def test_garbage_nibbles_fall_back(ea, fused):
    """A report with every read passing keeps its tile offsets; one where reads fail (all FALSE, or a fused threshold that
    fails some) counts the garbage nibbles differently: the direct launch must notice, fall back to the pool and replace
    the record, so that the same call once more is written directly."""
    T = ea._lib.load().epi_cx_tile_positions(b"Z")
    t = garbage_batch(31, (1, 3, 4), T)
    n = t["start"].size
    c = C2B["CG"]
    thr = (2, 0.5, 1.0)
    if fused:
        p = orc.threshold_reads(t["xm"], t["off"], c["ctx_meth"], c["ctx_unmeth"], c["ooctx_meth"], c["ooctx_unmeth"], *thr)
        assert 0 < p.sum() < n
    else:
        p = np.zeros(n, np.int32)
    want0, want1 = cx_oracle(t, None, "Z"), cx_oracle(t, p, "Z")
    assert tile_counts(want0, T) != tile_counts(want1, T)     # (what makes this batch a test of the check)
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"])
    try:
        got, w = report(ea, bam, "CG", False)
        assert not w
        H.assert_reports_equal(got, want0)
        assert capacity(ea, bam, "Z") == want0["pos"].size
        got, w = report(ea, bam, "CG", fused, thr=thr, pass_=None if fused else p)
        assert not w                                           # a direct launch was made, its counts differed
        H.assert_reports_equal(got, want1)
        assert capacity(ea, bam, "Z") == want1["pos"].size     # the record was replaced ...
        got, w = report(ea, bam, "CG", fused, thr=thr, pass_=None if fused else p)
        assert w                                               # ... so the same call is now written directly
        H.assert_reports_equal(got, want1)
        got, w = report(ea, bam, "CG", False)                  # and back
        assert not w
        H.assert_reports_equal(got, want0)
    finally:
        bam.close()


@pytest.mark.parametrize("nibble,grow", [(3, True), (1, False)])
def test_python_columns_after_fallback(ea, nibble, grow):
    """rcpp_cx_report allocates as many rows as the kept report had; after a fallback the table may be larger (nibble 3
    skipped under a failed read: the coverage drops) -- the columns are allocated again -- or smaller (1: doubled coverage)."""
    T = ea._lib.load().epi_cx_tile_positions(b"Z")
    t = garbage_batch(40 + nibble, (nibble,), T)
    n = t["start"].size
    p = np.zeros(n, np.int32)
    want0, want1 = cx_oracle(t, None, "Z"), cx_oracle(t, p, "Z")
    assert (want1["pos"].size > want0["pos"].size) if grow else (want1["pos"].size < want0["pos"].size)
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"])
    try:
        H.assert_reports_equal(dict(ea.rcpp_cx_report(bam, None, "Z")), want0)
        for _ in range(2):                                     # fallback (record replaced), then direct
            H.dirty_allocator(bam)
            H.assert_reports_equal(dict(ea.rcpp_cx_report(bam, p, "Z")), want1)
            assert capacity(ea, bam, "Z") == want1["pos"].size
        got, w = report(ea, bam, "CG", False, pass_=p)
        assert w
        H.assert_reports_equal(got, want1)
    finally:
        bam.close()


def test_rewrite_in_place(ea):
    """A zero-copy batch whose XM bytes are rewritten on the device (same rows, so the tile count stays): 'Z' <-> 'z'
    keeps every tile's row count (written directly, new values); '.' <-> 'Z' changes them (fallback).  The report must
    never be the old table; an error must say the rows changed."""
    import torch
    T = ea._lib.load().epi_cx_tile_positions(b"Z")
    t = segments_batch(17, [(1, 2, 30), (4, 0, 5)], T, lens="ragged")
    nb = int(t["off"][-1])
    xm = torch.full(((nb + 15) // 16 * 16 + 16,), 0xFB, dtype=torch.uint8, device="cuda:0")
    xm[:nb] = torch.from_numpy(t["xm"]).cuda()
    dev = lambda k: torch.from_numpy(np.ascontiguousarray(t[k])).cuda()
    bam = ea.ProcessedBam.from_device(xm, nb, dev("off"), dev("rname"), dev("strand"), dev("start"), realign=False)
    try:
        want = cx_oracle(t, None, "Z")
        for expect in (False, True):
            got, w = report(ea, bam, "CG", False)
            assert w == expect
            H.assert_reports_equal(got, want)
        rows = np.zeros(t["start"].size, bool)
        rows[::3] = True
        mask = np.repeat(rows, np.diff(t["off"]))
        for a, b in ((7, 15), (12, 7)):                        # 'Z' <-> 'z', then '.' <-> 'Z'
            new = t["xm"].copy()
            lo = new & 15
            sel_a, sel_b = mask & (lo == a), mask & (lo == b)
            new[sel_a] = (new[sel_a] & 0xF0) | b
            new[sel_b] = (new[sel_b] & 0xF0) | a
            xm[:nb] = torch.from_numpy(new).cuda()
            torch.cuda.synchronize()
            old, t = want, dict(t, xm=new)
            want = cx_oracle(t, None, "Z")
            assert not all(np.array_equal(old[k], want[k]) for k in want)
            same_counts = tile_counts(old, T) == tile_counts(want, T)
            assert same_counts == (a == 7)
            try:
                got, w = report(ea, bam, "CG", False)
            except ea._lib.EpihipError as e:
                assert "changed" in str(e)
            else:
                assert w == same_counts
                H.assert_reports_equal(got, want)
            got, w = report(ea, bam, "CG", False)
            H.assert_reports_equal(got, want)
    finally:
        bam.close()


def test_context_alternation(ea):
    """One record per batch: a report with other contexts replaces it, the same contexts twice in a row are written
    directly ("Zz" is not "Z": the lower-case letter adds its context index)."""
    T = ea._lib.load().epi_cx_tile_positions(b"Z")
    t = segments_batch(23, [(1, 0, 25), (2, 3, 40)], T, lens="ragged")
    seq = ("Z", "ZX", "Z", "Z", "Zz", "Zz", "ZXH", "ZXH", "Z")
    expect = (False, False, False, True, False, True, False, True, False)
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"])
    try:
        flags = []
        for letters in seq:
            got, w = report(ea, bam, "CG", False, letters=letters)
            H.assert_reports_equal(got, cx_oracle(t, None, letters))
            flags.append(w)
        assert tuple(flags) == expect
    finally:
        bam.close()


def test_heavy_tiles_worked_in_place(ea, hook_env):
    """EPIHIP_HEAVY_ROWS=100 on a batch without deep positions but with tiles of ~200 candidate rows: the pool report
    sets them aside (heavy path), the direct report works them in place."""
    hook_env("EPIHIP_HEAVY_ROWS", "100")
    T = ea._lib.load().epi_cx_tile_positions(b"Z")
    t = segments_batch(29, [(1, 0, 12), (3, 5, 6)], T, depth=25)
    L = np.diff(t["off"])
    s = t["start"].astype(np.int64)
    x = np.arange(t["start"].size - 255)
    assert not np.any((t["rname"][x + 255] == t["rname"][x]) & (s[x + 255] < s[x] + L[x]))    # no position deeper than 255
    assert np.bincount(((s + (1 << 31)) // T - ((1 << 31) // T)).astype(np.int64)).max() > 100  # rows starting in one tile
    for fused in (False, True):
        bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"])
        try:
            first, w1 = report(ea, bam, "CG", fused)
            second, w2 = report(ea, bam, "CG", fused)
            assert not w1 and w2
            H.assert_reports_equal(first, oracle(t, "CG", fused))
            H.assert_reports_equal(second, oracle(t, "CG", fused))
        finally:
            bam.close()
