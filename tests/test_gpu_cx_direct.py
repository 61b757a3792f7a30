"""CX reports written by the tile kernel itself (direct mode): the first report on a batch goes through the row pool and
the gather, and the batch keeps its tile offsets; a second one with the same contexts gets columns of that size and the
tile kernel writes them at those offsets.  Both tables must be bitwise equal and equal to the oracle, over tile counts
that are and are not multiples of the eight XCDs, gaps between tiles, several reference sequences, ragged and gapped rows;
pile-ups and a capacity one row short must fall back to the pool and give the same table."""
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


def report(ea, bam, ctx, fused, cap=None):
    """One report through the C entry point that takes the caller's columns: (table, written)."""
    import torch
    lib = ea._lib.load()
    b = bam.batch()
    c = C2B[ctx]
    letters = c["ctx_meth"].encode()
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
                                                    c["ooctx_unmeth"].encode(), 2, 0.5, 0.1, letters, None, cols if cap else None,
                                                    cap, stream, C.byref(nrow), C.byref(written))
    else:
        rc = lib.epi_batch_cx_report_into_dev(b, None, letters, cols if cap else None, cap, stream, C.byref(nrow), C.byref(written))
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
