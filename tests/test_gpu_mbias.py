"""generateMbiasReport on the GPU (epi_batch_mbias_report_dev) against the loop restatement of its definition
(tests/mbias_np.py), every cell: on the reference's fixtures at several table widths, against the library's own packer under
trim=, on seeded random batches in both layouts, composed with the writer and preprocessBam(trim=suggestTrim(...)), and with
errors, ownership and the other reports' state pinned."""
import contextlib
import ctypes as C
import functools
import gc
import os

import numpy as np
import pytest

import helpers as H
import mbias_np as MB
import synth_np

pytestmark = pytest.mark.gpu
BAM = os.path.join(H.GOLDEN, "bam")
LEVELS = ("chrA", "chrB", "chrC")
FIXTURES = {"capture": "capture.bam", "amplicon": "amplicon010meth.bam"}
WIDTHS = (1, 16, 17, 150, 1024)


@pytest.fixture(scope="module")
def ea():
    import epialleler_amd
    return epialleler_amd


def make(ea, t):
    return ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"], LEVELS)


def host(rep):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in rep.items()}


def same_report(got, want, want_totals, label=""):
    assert list(got.keys()) == list(MB.COLUMNS)
    MB.same(host(got), want, label)
    MB.same(dict(got.totals), want_totals, label + " totals")
    assert all(isinstance(v, np.ndarray) for v in got.totals.values())
    assert got.levels["end"] == ("start", "end")


def check(ea, t, max_offset, bam=None, label=""):
    """rcpp_mbias_report on the batch of t against the restatement -> the restatement's (table, totals)"""
    own = bam is None
    bam = make(ea, t) if own else bam
    try:
        got = ea.rcpp_mbias_report(bam, max_offset)
    finally:
        if own:
            bam.close()
    want = MB.restate(t, max_offset)
    same_report(got, *want, label=label)
    return want


# ---- 1. the fixtures --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def fixture_bam(which):
    import epialleler_amd as ea
    return ea.preprocessBam(os.path.join(BAM, FIXTURES[which]))


@functools.lru_cache(maxsize=None)
def fixture_counts(which):
    """The restatement's counters of a fixture at the widest table (computed once; read-only): a narrower table is its first
    max_offset offsets, the totals are the same (tests/test_mbias_host.py checks both on the restatement)"""
    t = fixture_bam(which).host
    return MB.counts(t["xm"], t["off"], t["strand"], 1024)


def fixture_want(which, max_offset, context="CX"):
    tab, tot = fixture_counts(which)
    return MB.table(tab[:, :, :, :max_offset], context), MB.totals_table(tot, context)


@pytest.mark.parametrize("max_offset", WIDTHS)
@pytest.mark.parametrize("which", ["capture", "amplicon"])
def test_fixtures(ea, which, max_offset):
    pb = fixture_bam(which)
    want = fixture_want(which, max_offset)
    same_report(ea.generateMbiasReport(pb, max_offset=max_offset), *want, label="generate")
    same_report(ea.rcpp_mbias_report(pb, max_offset), *want, label="rcpp")
    assert want[0]["meth"].size == 12 * max_offset and want[1]["meth"].sum() > 500
    if which == "capture":
        assert pb.n == 2968 and want[0]["meth"].max() > 0
    if max_offset == 150:                                    # the default
        same_report(ea.generateMbiasReport(pb), *want, label="default")


def test_trim_shifts_the_tables(ea):
    """The library's own packer under trim = (3, 5): the start table moves by 3 offsets, the end table by 5, and the totals lose
    exactly the cells of the removed offsets (no template is shorter than 33 bytes, so none vanishes and no removed byte is in
    both tables).  The shift holds at the offsets no removed byte of the OTHER end reaches: the 5 bytes cut from the end of a
    template of L bytes sat at start offsets L - 5 .. L - 1, so the tables are compared whole at max_offset = shortest template
    - 8 and over that prefix at the default width; beyond it the trimmed table is the restatement of the trimmed rows."""
    path = os.path.join(BAM, FIXTURES["capture"])
    whole = fixture_bam("capture")
    cut = ea.preprocessBam(path, trim=(3, 5))
    assert cut.n == whole.n
    assert np.array_equal(np.diff(cut.host["off"]), np.diff(whole.host["off"]) - 8)
    safe = int(np.diff(whole.host["off"]).min()) - 8
    assert safe == 92
    tab, tot = fixture_counts("capture")
    left = tot - tab[0][:, :, :3].sum(axis=2) - tab[1][:, :, :5].sum(axis=2)
    assert left.sum() < tot.sum()
    shifted = np.stack([tab[0][:, :, 3:3 + safe], tab[1][:, :, 5:5 + safe]])
    same_report(ea.generateMbiasReport(path, trim=(3, 5), max_offset=safe), MB.table(shifted), MB.totals_table(left), label="trim")
    got = ea.generateMbiasReport(path, trim=(3, 5))
    want, want_tot = MB.restate(cut.host, 150)
    same_report(got, want, want_tot, label="trim, restated")
    MB.same(dict(got.totals), MB.totals_table(left), "totals at the default width")
    prefix = got["offset"] < safe
    wide = MB.table(np.stack([tab[0][:, :, 3:153], tab[1][:, :, 5:155]]))
    MB.same({k: v[prefix] for k, v in host(got).items()}, {k: v[prefix] for k, v in wide.items()}, "the prefix at the default width")


# ---- 2. seeded random batches -----------------------------------------------------------------------------------------------

def permuted(t, order):
    """The rows of t in another order"""
    lens = np.diff(t["off"])
    pieces = [t["xm"][t["off"][x]:t["off"][x + 1]] for x in order]
    out = {k: t[k][order] for k in ("rname", "strand", "start")}
    out["xm"] = np.concatenate(pieces) if pieces else np.zeros(0, np.uint8)
    out["off"] = np.concatenate(([0], np.cumsum(lens[order]))).astype(np.int64)
    return out


def fuzz_batch(seed, n=400):
    """Both strands, the whole code alphabet (filler, '.', U / u and, through raw bytes, the unused codes), lengths 0 to 700"""
    rng = np.random.default_rng(seed)
    t = synth_np.random_templates(rng, n, 0, 700, 3, 5000, p_garbage=0.1, alphabet=".hxzZHXuU+-")
    assert np.unique(t["xm"] & 15).size == 16 and np.diff(t["off"]).min() < 16 and np.diff(t["off"]).max() > 680
    return t, rng


@pytest.mark.parametrize("max_offset", [16, 150, 300, 1024])
@pytest.mark.parametrize("seed", [21, 22])
def test_fuzz_uploaded(ea, seed, max_offset):
    t, rng = fuzz_batch(seed)
    tab, tot = check(ea, t, max_offset, label="sorted")
    assert (tab["meth"] > 0).sum() > max_offset and tot["meth"].min() > 100
    u = permuted(t, rng.permutation(t["strand"].size))                   # rows need not be sorted
    check(ea, u, max_offset, label="unsorted")


@pytest.mark.parametrize("max_offset", [17, 150])
def test_fuzz_adopted_without_realignment(ea, max_offset):
    """Adopted with realign=False the rows lie back to back, at any byte alignment; uploaded they are laid out by start position"""
    import torch
    t, _ = fuzz_batch(23)
    nb = int(t["off"][-1])
    xm = torch.full(((nb + 15) // 16 * 16 + 64,), 0xF7, dtype=torch.uint8, device="cuda:0")      # (0xF7 behind the rows: a CG call if read)
    xm[:nb] = torch.from_numpy(t["xm"]).cuda()
    dev = {k: torch.from_numpy(t[k]).cuda() for k in ("off", "rname", "strand", "start")}
    ad = ea.ProcessedBam.from_device(xm, nb, dev["off"], dev["rname"], dev["strand"], dev["start"], LEVELS, realign=False)
    up = make(ea, t)
    try:
        check(ea, t, max_offset, bam=ad, label="adopted")
        check(ea, t, max_offset, bam=up, label="uploaded")
        assert ea._lib.load().epi_batch_layout(ad.batch()) == 0 and ea._lib.load().epi_batch_layout(up.batch()) == 16
    finally:
        ad.close()
        up.close()


def test_empty_batch(ea):
    tab, tot = check(ea, H.templates_from_xm([], [], []), 150)
    assert tab["meth"].size == 1800 and not tab["meth"].any() and not tab["unmeth"].any() and np.all(np.isnan(tab["beta"]))
    assert not tot["meth"].any() and not tot["unmeth"].any()


# ---- 3. composition -----------------------------------------------------------------------------------------------------------

def test_device_table(ea):
    import torch
    pb = fixture_bam("amplicon")
    dev = ea.generateMbiasReport(pb, max_offset=64, as_device=True)
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in dev.values())
    assert [dev[k].dtype for k in MB.COLUMNS] == [torch.int32] * 6 + [torch.float64]
    same_report(dev, *fixture_want("amplicon", 64), label="device")


@pytest.mark.parametrize("as_device", [False, True])
@pytest.mark.parametrize("context", ["CG", "CHG", "CHH", "CxG", "CX"])
def test_report_context_selects_rows(ea, context, as_device):
    pb = fixture_bam("capture")
    got = ea.generateMbiasReport(pb, report_context=context, max_offset=40, as_device=as_device)
    same_report(got, *fixture_want("capture", 40, context), label=context)
    whole = host(ea.generateMbiasReport(pb, max_offset=40))
    keep = np.isin(whole["context"], MB.CONTEXT_CODES[context])
    MB.same(host(got), {k: v[keep] for k, v in whole.items()}, "rows of CX")
    assert got.nrow == 4 * 40 * len(MB.CONTEXT_CODES[context])


def test_write_report_labels(ea, tmp_path):
    pb = fixture_bam("amplicon")
    path = str(tmp_path / "mbias.tsv")
    assert ea.generateMbiasReport(pb, report_file=path, max_offset=5) is None
    want, _ = fixture_want("amplicon", 5)
    with open(path) as f:
        lines = [ln.rstrip("\n").split("\t") for ln in f]
    assert lines[0] == list(MB.COLUMNS) and len(lines) == 61
    ends, strands, ctxs = ("start", "end"), ("+", "-"), {2: "CHH", 6: "CHG", 7: "CG"}
    for i, row in enumerate(lines[1:]):
        assert row[:6] == [ends[want["end"][i] - 1], strands[want["strand"][i] - 1], ctxs[int(want["context"][i])], str(want["offset"][i]),
                           str(want["meth"][i]), str(want["unmeth"][i])], i
        assert (row[6] == "") == bool(np.isnan(want["beta"][i])) and (row[6] == "" or abs(float(row[6]) - want["beta"][i]) < 1e-12)


@pytest.mark.parametrize("which", ["capture", "amplicon"])
def test_suggest_trim_feeds_preprocess_bam(ea, which):
    path = os.path.join(BAM, FIXTURES[which])
    rep = ea.generateMbiasReport(path)
    for kw in ({}, dict(min_calls=1, max_delta=0.02), dict(context="CX", min_calls=10, run=5)):
        trim = ea.suggestTrim(rep, **kw)
        assert trim == MB.suggest_trim(host(rep), **kw) and all(0 <= v <= 75 for v in trim)
        cut = ea.preprocessBam(path, trim=trim)
        lens = np.diff(fixture_bam(which).host["off"])
        assert cut.n == lens.size
        if sum(trim) < lens.min():
            assert np.array_equal(np.diff(cut.host["off"]), lens - sum(trim))
    assert ea.suggestTrim(ea.generateMbiasReport(path, as_device=True)) == ea.suggestTrim(rep)


# ---- 4. errors, ownership and the other reports' state --------------------------------------------------------------------------

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


def raw_call(ea, bam, max_offset, counts=True, totals=True, batch=True, fill=-7):
    """epi_batch_mbias_report_dev on arrays filled with a sentinel -> (return code, counts, totals)"""
    import torch
    from epialleler_amd.api import _stream
    dev = "cuda:%d" % bam.device
    c = torch.full((24 * 1024,), fill, dtype=torch.int64, device=dev)
    t = torch.full((12,), fill, dtype=torch.int64, device=dev)
    rc = ea._lib.load().epi_batch_mbias_report_dev(bam.batch() if batch else None, max_offset, C.c_void_p(c.data_ptr()) if counts else None,
                                                   C.c_void_p(t.data_ptr()) if totals else None, _stream(bam.device))
    torch.cuda.synchronize()
    return rc, c.cpu().numpy(), t.cpu().numpy()


def test_errors_and_ownership(ea):
    t, _ = fuzz_batch(31, n=100)
    bam = make(ea, t)
    bam.batch()
    x = int(np.flatnonzero(np.diff(t["off"]) > 0)[50])                    # a row with bytes gets strand 3
    bad = make(ea, dict(t, strand=np.where(np.arange(100) == x, 3, t["strand"]).astype(np.int32)))
    bad.batch()
    E = ea._lib
    try:
        with nothing_left(ea):
            rc, c, tt = raw_call(ea, bam, 150)
            tab, tot = MB.counts(t["xm"], t["off"], t["strand"], 150)
            assert rc == E.EPI_OK and np.array_equal(c[:3600], tab.reshape(-1)) and np.all(c[3600:] == -7) and np.array_equal(tt, tot.reshape(-1))
        with nothing_left(ea):
            for kw, name in ((dict(max_offset=0), b"max_offset"), (dict(max_offset=1025), b"max_offset"), (dict(max_offset=-1), b"max_offset"),
                             (dict(max_offset=16, counts=False), b"d_counts"), (dict(max_offset=16, totals=False), b"d_totals"),
                             (dict(max_offset=16, batch=False), b"batch")):
                rc, c, tt = raw_call(ea, bam, **kw)
                assert rc == E.EPI_ERR_ARG and np.all(c == -7) and np.all(tt == -7), kw
                assert name in E.load().epi_last_error(), kw
        with nothing_left(ea):
            rc, c, tt = raw_call(ea, bad, 16)
            assert rc == E.EPI_ERR_ARG and b"strand" in E.load().epi_last_error() and np.all(c == -7) and np.all(tt == -7)
            with pytest.raises(ea.EpihipError) as ei:
                ea.rcpp_mbias_report(bad, 16)
            assert ei.value.code == E.EPI_ERR_ARG
        with pytest.raises(ValueError):
            ea.rcpp_mbias_report(bam, 1025)
    finally:
        bam.close()
        bad.close()


def assert_same_table(a, b, label):
    assert list(a.keys()) == list(b.keys()), label
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape, (label, k)
        assert np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x, y.view(np.uint64) if y.dtype == np.float64 else y), (label, k)


def test_other_reports_are_not_disturbed(ea):
    """A cytosine report, an lMHL report and a heterogeneity report before and after an M-bias call on the same batch; the M-bias
    table itself on a second call"""
    t = H.load_bam("capture.bam")
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"], t["levels"])
    others = (("cytosine", lambda: ea.generateCytosineReport(bam)), ("lMHL", lambda: ea.generateMhlReport(bam)),
              ("heterogeneity", lambda: ea.generateHeterogeneityReport(bam)))
    try:
        first = ea.rcpp_mbias_report(bam, 150)
        for label, report in others:
            before = report()
            with nothing_left(ea):
                again = ea.rcpp_mbias_report(bam, 150)
                assert_same_table(again, first, "M-bias after " + label)
                assert_same_table(again.totals, first.totals, "totals after " + label)
                del again
            after = report()
            assert before.nrow > 0
            assert_same_table(after, before, label)
        same_report(first, *fixture_want("capture", 150), label="batch from arrays")
    finally:
        bam.close()
