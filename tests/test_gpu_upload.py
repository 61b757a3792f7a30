"""Uploads that cross piece boundaries with real content: epi_batch_upload sends the packed bytes in pieces (64 MiB from
pageable memory through the pinned staging buffers; nbytes / 8, clamped to 16..256 MiB, straight from pinned memory) and
places the rows of each piece -- parts of rows that straddle a boundary included -- while the next one is on the link.
EPIHIP_UPLOAD_PIECE shrinks the pieces so that a few MiB cross hundreds of boundaries.  The whole device arena is compared
byte for byte with one built here; then thresholding, CX and lMHL run against the oracle.  Random content over many pieces
makes a missing double-buffer wait likely, not certain, to show as corrupted bytes."""
import numpy as np
import pytest

import helpers as H
from oracle import oracle as orc
from test_gpu_layout import _check_layout, _view

pytestmark = pytest.mark.gpu

MiB = 1 << 20
LETTERS = np.frombuffer(b"..zZZzxXhH+-", np.uint8)


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


def content(rng, nb):
    """nb packed bytes: random high nibble, XM letters from LETTERS in the low one (uint8 all the way: cheap for 140 MiB)"""
    lut = np.zeros(256, np.uint8)
    for b in range(256):
        ch = int(LETTERS[(b & 15) % LETTERS.size])
        lut[b] = ((b >> 4) << 4) | (((ch + 2) >> 2) & 15)
    return lut[rng.integers(0, 256, size=nb, dtype=np.uint8)]


def batch_from_lens(rng, lens, span_per_row=40):
    lens = np.asarray(lens, np.int64)
    n = lens.size
    off = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    rname = np.sort(rng.integers(1, 3, n)).astype(np.int32)
    start = np.zeros(n, np.int32)
    for r in (1, 2):
        m = rname == r
        start[m] = np.sort(rng.integers(1, max(int(m.sum()) * span_per_row, 2), int(m.sum())))
    return {"xm": content(rng, int(off[-1])), "off": off, "rname": rname, "strand": rng.integers(1, 3, n).astype(np.int32),
            "start": start}


def boundary_batch(rng, piece, total=8 * MiB):
    """Random ragged rows of about `total` bytes with, at piece boundaries: a row that ends / starts exactly there, three
    empty rows, one row longer than two pieces; the first and last rows empty."""
    lens = [0]
    while sum(lens) < total:
        lens.append(int(rng.integers(0, 700)))
    lens.insert(len(lens) // 3, 2 * piece + 12345)                   # longer than two pieces
    lens.append(0)
    lens = np.asarray(lens, np.int64)

    def split_at(lens, b, empties):
        ends = np.cumsum(lens)
        x = int(np.searchsorted(ends, b, "right"))                   # the row holding byte b (or starting at it)
        s = int(ends[x] - lens[x])
        if s == b:
            return np.concatenate((lens[:x], [0] * empties, lens[x:]))
        return np.concatenate((lens[:x], [b - s], [0] * empties, [int(ends[x]) - b], lens[x + 1:]))
    nb = int(lens.sum())
    k = max(nb // piece, 4)
    lens = split_at(lens, piece * 1, 0)                             # a row ends, the next starts at the first boundary
    lens = split_at(lens, piece * (k // 2), 3)                      # empty rows at a boundary in the middle
    lens = split_at(lens, piece * (k - 1), 0)
    return batch_from_lens(rng, lens)


def pinned(ea, t):
    import torch
    cols = [torch.from_numpy(np.ascontiguousarray(t[k])).pin_memory() for k in ("xm", "off", "rname", "strand", "start")]
    return ea.ProcessedBam.from_pinned(cols[0], int(t["off"][-1]), *cols[1:])


def check_upload(ea, t, source, modulus=16, kernels=True):
    bam = pinned(ea, t) if source == "pinned" else ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"])
    try:
        xm, off, ln, layout = _view(ea, bam)
        assert layout == modulus
        _check_layout(t, xm, off, ln, modulus)
        if not kernels:
            return
        c4 = H.cls4("CG")
        want = orc.threshold_reads(t["xm"], t["off"], *c4, 2, 0.5, 0.1)
        assert np.array_equal(ea.rcpp_threshold_reads(bam, *c4, 2, 0.5, 0.1).astype(np.int32), want)
        H.assert_reports_equal(dict(ea.rcpp_cx_report(bam, want, "Z")),
                               orc.cx_report(t["xm"], t["off"], t["rname"], t["strand"], t["start"], want, "Z"))
        H.assert_reports_equal(dict(ea.rcpp_mhl_report(bam, "Zz", 0, 0, 0.1)),
                               orc.mhl_report(t["xm"], t["off"], t["rname"], t["strand"], t["start"], "Zz", 0, 0, 0.1),
                               float_cols=("length", "lmhl"))
    finally:
        bam.close()


@pytest.mark.parametrize("realign", ["16", "0"])
@pytest.mark.parametrize("piece", [4096, MiB + 13, MiB])
@pytest.mark.parametrize("source", ["pageable", "pinned"])
def test_piece_boundaries(ea, hook_env, source, piece, realign):
    """Pieces of 4 KiB (~2 000 of them), 1 MiB + 13 (boundaries off every alignment) and 1 MiB, from pageable and pinned
    memory, rows laid out congruently and back to back.  The kernels run where no row is longer than 64 KiB (the row
    of two pieces and more is then only 20 KiB); with the 1 MiB pieces it exceeds 2 MiB, and the arena check stands alone."""
    hook_env("EPIHIP_UPLOAD_PIECE", str(piece))
    hook_env("EPIHIP_REALIGN", realign)
    rng = np.random.default_rng(piece + (7 if source == "pinned" else 0))
    t = boundary_batch(rng, piece)
    check_upload(ea, t, source, modulus=int(realign), kernels=piece < 64 * 1024)


def test_shipped_piece_sizes(ea):
    """No hook: a pinned batch of ~40 MiB (three 16 MiB pieces) and a pageable one of ~140 MiB (three 64 MiB pieces)."""
    rng = np.random.default_rng(40)
    for source, total in (("pinned", 40 * MiB + 4321), ("pageable", 140 * MiB + 777)):
        lens = rng.integers(0, 700, total // 350 + 10)
        lens = lens[np.cumsum(lens) <= total]
        lens = np.append(lens, total - int(lens.sum()))
        check_upload(ea, batch_from_lens(rng, lens), source)


def test_staging_buffers_grow(ea, hook_env):
    """Uploads on one engine with growing pieces: the device staging buffers are reallocated between them (264 MiB is more
    than any piece the engine picks itself), and every upload lands whole."""
    rng = np.random.default_rng(41)
    lens = rng.integers(0, 700, (150 * MiB) // 350)
    t = batch_from_lens(rng, lens)
    for source, piece in (("pageable", None), ("pinned", 72 * MiB), ("pinned", 264 * MiB), ("pageable", 3 * MiB)):
        if piece:
            hook_env("EPIHIP_UPLOAD_PIECE", str(piece))
        check_upload(ea, t, source, kernels=False)
    c4 = H.cls4("CG")                                              # and the last batch through a kernel
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"])
    try:
        want = orc.threshold_reads(t["xm"], t["off"], *c4, 2, 0.5, 0.1)
        assert np.array_equal(ea.rcpp_threshold_reads(bam, *c4, 2, 0.5, 0.1).astype(np.int32), want)
    finally:
        bam.close()
