"""epi_batch_mbias_report_dev at the seams of its kernel (csrc/mbias.hip), the smallest shapes at which it can go wrong: row
lengths around the table width and around twice it (where the two tables meet and overlap, and where a row gets a middle that
is streamed in 16-byte chunks), a row beyond 64 KiB and one whose middle passes the middle's flush, row counts around a
workgroup's slice and beyond the workgroup cap (workgroups without rows), slices longer than the flush period of the packed
fields, the bytes both tables count under several offsets per thread, table widths around the workgroup size, one strand and strands in turn, and rows without a classed byte.  Compared
with tests/mbias_np.py as test_gpu_mbias.py does; a batch of repeated rows is restated once per distinct row (the counters
are sums over rows)."""
import numpy as np
import pytest

import mbias_np as MB
from test_gpu_mbias import ea, make, same_report  # noqa: F401

pytestmark = pytest.mark.gpu

# the kernel's constants (csrc/mbias.hip)
WG = 256               # MB_WG: threads of a workgroup = offsets a thread slot holds
RIF = 8                # MB_RIF: rows in flight
SLICE_MIN = 64         # MB_SLICE_MIN: rows of a workgroup's slice, at least
MAX_WG = 1024          # MB_MAX_WG: workgroups at most; beyond SLICE_MIN * MAX_WG rows the slices grow
FLUSH = 1016           # MB_FLUSH: rows between two flushes of the 10-bit fields
MID_FLUSH = 63         # MB_MID_FLUSH: 16-byte chunks per thread between two flushes of the middle's fields
# a row longer than 2 * max_offset has a middle: bytes [max_offset, L - max_offset), WG * 16 bytes a step

ALPHABET = np.frombuffer(b".hxzZHXuU+-", np.uint8)


def rows_of(rng, lengths, strands):
    """Random rows of the given lengths over the whole alphabet (every 16th byte raw: the unused codes)"""
    lengths = np.asarray(lengths, np.int64)
    off = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    nb = int(off[-1])
    ch = ALPHABET[rng.integers(0, ALPHABET.size, nb)].astype(np.int64)
    xm = ((rng.integers(0, 16, nb) << 4) | (((ch + 2) >> 2) & 15)).astype(np.uint8)
    xm[::16] = rng.integers(0, 256, xm[::16].size).astype(np.uint8)
    n = lengths.size
    return {"xm": xm, "off": off, "rname": np.ones(n, np.int32), "strand": np.asarray(strands, np.int32), "start": np.arange(1, n + 1, dtype=np.int32)}


def repeated(row_bytes, strands, n):
    """n rows: row x has the bytes row_bytes[x % len(row_bytes)] and the strand strands[x % len(strands)] (equal lengths)"""
    k = len(row_bytes)
    assert len(strands) == k and len({len(r) for r in row_bytes}) == 1
    L = len(row_bytes[0])
    letters = np.frombuffer(b"".join(row_bytes), np.uint8).astype(np.int64)
    unit = (0x10 | (((letters + 2) >> 2) & 15)).astype(np.uint8)
    xm = np.concatenate([np.tile(unit, n // k), unit[:(n % k) * L]])
    return {"xm": xm, "off": np.arange(n + 1, dtype=np.int64) * L, "rname": np.ones(n, np.int32),
            "strand": np.resize(np.asarray(strands, np.int32), n), "start": np.arange(1, n + 1, dtype=np.int32)}


def check(ea, t, max_offset, want_counts=None, label=""):
    tab, tot = MB.counts(t["xm"], t["off"], t["strand"], max_offset) if want_counts is None else want_counts
    bam = make(ea, t)
    try:
        got = ea.rcpp_mbias_report(bam, max_offset)
    finally:
        bam.close()
    same_report(got, MB.table(tab), MB.totals_table(tot), label=label)
    return tab, tot


def repeated_counts(row_bytes, strands, n, max_offset):
    """The counters of repeated(...): each distinct row restated once, times the number of its copies"""
    k = len(row_bytes)
    tab = np.zeros((2, 2, 3, max_offset, 2), np.int64)
    tot = np.zeros((2, 3, 2), np.int64)
    for i in range(k):
        one = repeated([row_bytes[i]], [strands[i]], 1)
        a, b = MB.counts(one["xm"], one["off"], one["strand"], max_offset)
        copies = n // k + (1 if i < n % k else 0)
        tab += copies * a
        tot += copies * b
    return tab, tot


# ---- row lengths and table widths ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", [1, 17, WG - 1, WG, WG + 1, 1024])
def test_row_lengths_around_the_table_width(ea, M):
    """L = 0, 1, 15, 16, 17, M - 1, M, M + 1, 2 M - 1, 2 M, 2 M + 1 and one row of 70 000 bytes (beyond a 16-bit length and 64 KiB),
    each length on both strands, the strands in turn; again with every row on one strand"""
    rng = np.random.default_rng(100 + M)
    lengths = [0, 1, 15, 16, 17, M - 1, M, M + 1, 2 * M - 1, 2 * M, 2 * M + 1, 2 * M + 15, 2 * M + 16, 2 * M + 17, 2 * M + WG * 16 + 3]
    lengths = [v for v in lengths for _ in range(2)] + [70000]
    n = len(lengths)
    t = rows_of(rng, lengths, 1 + np.arange(n) % 2)
    tab, tot = check(ea, t, M, label="strands in turn")
    assert tot.min() > 0 and tab[0].sum() > 0 and tab[1].sum() > 0
    for s in (1, 2):
        check(ea, dict(t, strand=np.full(n, s, np.int32)), M, label="strand %d" % s)


def test_middle_beyond_its_flush(ea):
    """One row whose middle gives a thread more than MID_FLUSH chunks (a field of 10 bits would carry at 64 chunks of one letter),
    between two short rows on the other strand"""
    L = (MID_FLUSH + 10) * WG * 16 + 2 * 150 + 5
    rows = [b"Zz", b"Z" * L, b"xH."]
    lengths = [len(r) for r in rows]
    letters = np.frombuffer(b"".join(rows), np.uint8).astype(np.int64)
    t = {"xm": (0x10 | (((letters + 2) >> 2) & 15)).astype(np.uint8), "off": np.concatenate(([0], np.cumsum(lengths))).astype(np.int64),
         "rname": np.ones(3, np.int32), "strand": np.asarray([1, 2, 1], np.int32), "start": np.asarray([1, 2, 3], np.int32)}
    want_tot = np.zeros((2, 3, 2), np.int64)
    want_tot[1, 2, 0] = L
    want_tot[0, 2] = (1, 1)
    want_tot[0, 1, 1] = 1
    want_tot[0, 0, 0] = 1
    tab, tot = check(ea, t, 150)
    assert np.array_equal(tot, want_tot) and tab[0, 1, 2, :, 0].tolist() == [1] * 150


# ---- row counts ---------------------------------------------------------------------------------------------------------------

ROW_A, ROW_B = b"ZzXxHhZzXxHhZ.U-", b"hHxXzZ-U.ZhHxXzZ"


@pytest.mark.parametrize("n", [0, 1, RIF - 1, RIF, RIF + 1, SLICE_MIN - 1, SLICE_MIN, SLICE_MIN + 1, 2 * SLICE_MIN + 1])
def test_row_counts_around_a_slice(ea, n):
    rng = np.random.default_rng(200 + n)
    t = rows_of(rng, rng.integers(0, 60, n), rng.integers(1, 3, n))
    check(ea, t, 24, label="%d rows" % n)


def test_workgroups_without_rows(ea):
    """70 000 rows of 16 identical bytes: beyond SLICE_MIN * MAX_WG rows the slices grow to 72 rows (a multiple of RIF), so the
    last 51 of the 1024 workgroups have no row; every owned cell exceeds 65 535"""
    n = 70000
    slice_rows = -(-(-(-n // MAX_WG)) // RIF) * RIF
    assert slice_rows == 72 and slice_rows * (MAX_WG - 51) >= n
    for strands, label in (([1], "one strand"), ([1, 2], "strands in turn")):
        rows = [ROW_A] * len(strands)
        tab, _ = check(ea, repeated(rows, strands, n), 16, repeated_counts(rows, strands, n, 16), label=label)
        if len(strands) == 1:
            assert tab[0, 0].max() == n > 65535 and tab[0, 1].max() == 0


@pytest.mark.parametrize("slice_rows", [FLUSH - RIF, FLUSH, FLUSH + RIF, 2 * FLUSH + RIF])
@pytest.mark.parametrize("short", [0, 1])
def test_slices_around_the_flush_period(ea, slice_rows, short):
    """MAX_WG slices of slice_rows rows (the last one a row short, or not): every workgroup's fields pass FLUSH rows of one
    letter per cell, which ten bits do not hold"""
    n = MAX_WG * slice_rows - short
    rows, strands = [ROW_A, ROW_A, ROW_B], [1, 2, 2]
    tab, _ = check(ea, repeated(rows, strands, n), 16, repeated_counts(rows, strands, n, 16), label="%d rows" % n)
    assert tab.max() > n // 4


@pytest.mark.parametrize("M,slice_rows", [(2 * WG, 520), (3 * WG, 344), (4 * WG, 264)])
def test_double_counted_bytes_in_wide_tables(ea, M, slice_rows):
    """Tables of 2, 3 and 4 offsets per thread under rows of max_offset + 7 identical bytes on one strand: every end byte but
    the last 7 is in the start table as well, so a thread takes one such byte per row at each of its offsets, all of one class.
    MAX_WG slices of more than 1023 / (offsets per thread) rows: were those bytes counted in one packed field for all of a
    thread's offsets, the field would carry and the totals (not the tables) come out wrong."""
    noff = M // WG
    assert slice_rows % RIF == 0 and slice_rows * noff > 1023 and slice_rows < FLUSH
    n = MAX_WG * slice_rows
    rows, strands = [b"h" * (M + 7)], [1]
    tab, tot = check(ea, repeated(rows, strands, n), M, repeated_counts(rows, strands, n, M), label="max_offset %d" % M)
    assert tot[0, 0, 1] == n * (M + 7) and tot.sum() == n * (M + 7) and tab[0, 0, 0, :, 1].tolist() == [n] * M == tab[1, 0, 0, :, 1].tolist()


def test_no_classed_byte(ea):
    rng = np.random.default_rng(5)
    n = 300
    lengths = rng.integers(0, 400, n)
    off = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    xm = np.where(rng.random(int(off[-1])) < 0.5, 0xFB, 0x1C).astype(np.uint8)                   # the filler and '.'
    t = {"xm": xm, "off": off, "rname": np.ones(n, np.int32), "strand": rng.integers(1, 3, n).astype(np.int32), "start": np.arange(1, n + 1, dtype=np.int32)}
    tab, tot = check(ea, t, 150)
    assert not tab.any() and not tot.any()
