"""mergeCpgStrands and smoothCytosineReport on the GPU: epi_cx_merge_strands_dev and epi_cx_smooth_dev against the numpy
restatement (tests/smooth_np.py) on the hand-written tables, on seeded fuzz tables (both strands and three contexts
interleaved over two rnames), on the small clusters, the cluster cuts, zero coverage and large positions; every error, each
writing nothing; ownership; and the sequence of report, merge and smooth on a fixture BAM.  test_gpu_smooth_seams.py has the
sizes at the fit kernel's tile and staging seams and the window limit.

Integer columns are compared exactly, beta, smoothed and weight bit for bit (NaN where the restatement has NaN): no
tolerance anywhere."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers as H
import smooth_np as S

pytestmark = pytest.mark.gpu

LEVELS = ("chrA", "chrB", "chrC")
MARK = -7


@pytest.fixture(scope="module")
def ea():
    import epialleler_amd
    return epialleler_amd


def dev_report(ea, t, levels=LEVELS):
    import torch
    return ea.Report({k: torch.from_numpy(np.ascontiguousarray(t[k])).cuda() for k in S.CX}, levels)


def allocations(ea):
    live, nbytes = C.c_int64(-1), C.c_int64(-1)
    ea._lib.check(ea._lib.load().epi_device_allocations(C.byref(live), C.byref(nbytes)))
    return live.value, nbytes.value


def gpu_smooth(ea, t, **kw):
    rep = ea.rcpp_cx_smooth(dev_report(ea, t), **kw)
    assert list(rep) == list(S.SMOOTH_COLUMNS) and rep.levels["rname"] == LEVELS
    return rep


def check_smooth(ea, t, what="", **kw):
    got, want = gpu_smooth(ea, t, **kw), S.smooth_np(t, **kw)
    S.same(got, want, what)
    assert (got.ncluster, got.max_window) == (want["ncluster"], want["max_window"]), what
    return got


def gpu_merge(ea, t):
    rep = ea.rcpp_cx_merge_strands(dev_report(ea, t))
    assert list(rep) == list(S.CX) and rep.levels["rname"] == LEVELS
    return rep


def check_merge(ea, t, what=""):
    got, want = gpu_merge(ea, t), S.merge_np(t)
    for k in S.CX:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), (what, k)
    assert (got.nmerged, got.nmoved, got.nkept) == (want["nmerged"], want["nmoved"], want["nkept"]), what
    return got


def raw_smooth(ea, t, bandwidth=1000, min_sites=70, max_gap=10 ** 8, degree=2):
    """epi_cx_smooth_dev itself, into columns filled with a mark: (rc, ncluster, max_window, columns, message)."""
    import torch
    from epialleler_amd import _lib, api
    lib = _lib.load()
    rep = dev_report(ea, t)
    n = t["pos"].size
    icols = list(torch.full((9, max(n, 1)), MARK, dtype=torch.int32, device="cuda").unbind(0))
    dcols = list(torch.full((3, max(n, 1)), float(MARK), dtype=torch.float64, device="cuda").unbind(0))
    ncluster, max_window = C.c_int64(-1), C.c_int64(-1)
    rc = lib.epi_cx_smooth_dev(api._engine(0), api._ptr_array([rep[k] for k in S.CX]), n, bandwidth, min_sites, max_gap, degree,
                               api._ptr_array(icols), api._ptr_array(dcols), api._stream(0), C.byref(ncluster), C.byref(max_window))
    torch.cuda.synchronize()
    return rc, ncluster.value, max_window.value, [c.cpu().numpy() for c in icols + dcols], lib.epi_last_error()


def raw_merge(ea, t, cap):
    """epi_cx_merge_strands_dev itself, into columns filled with a mark: (rc, (nrow, nmerged, nmoved, nkept), columns, message)."""
    import torch
    from epialleler_amd import _lib, api
    lib = _lib.load()
    rep = dev_report(ea, t)
    out = list(torch.full((6, max(cap, 1)), MARK, dtype=torch.int32, device="cuda").unbind(0))
    counts = [C.c_int64(-1) for _ in range(4)]
    rc = lib.epi_cx_merge_strands_dev(api._engine(0), api._ptr_array([rep[k] for k in S.CX]), t["pos"].size, api._ptr_array(out), cap,
                                      api._stream(0), *[C.byref(c) for c in counts])
    torch.cuda.synchronize()
    return rc, tuple(c.value for c in counts), [c.cpu().numpy() for c in out], lib.epi_last_error()


def _untouched(cols):
    return all(np.all(c == MARK) for c in cols)


# ---- merge ---------------------------------------------------------------------------------------------------------------

def test_merge_hand_written(ea):
    got = check_merge(ea, S.MERGE_KAT)
    assert S.rows_of(got) == S.rows_of(S.MERGE_KAT_WANT)
    for rows in ([(1, 1, 10, S.CG, 3, 1), (1, 2, 11, S.CG, 2, 4)], [(1, 2, 11, S.CG, 2, 4)], [(1, 1, 10, S.CHH, 1, 1), (1, 2, 11, S.CG, 2, 4)],
                 [(1, 2, 10, S.CHG, 1, 1), (1, 2, 11, S.CG, 2, 4)], [(1, 2, 1, S.CG, 2, 4)], [(1, 2, 2, S.CG, 2, 4)],
                 [(1, 1, 10, S.CHG, 1, 0), (1, 2, 10, S.CHH, 0, 1), (1, 1, 11, S.CG, 0, 0)], [(1, 1, 10, S.CG, 2 ** 31 - 2, 0), (1, 2, 11, S.CG, 1, 0)],
                 [(1, 2, 2 ** 31 - 1, S.CG, 1, 0)], [(0, 1, 2 ** 31 - 2, S.CG, 1, 0), (0, 2, 2 ** 31 - 1, S.CG, 1, 5)]):
        check_merge(ea, S.cx_table(rows), rows)
    empty = gpu_merge(ea, S.cx_table([]))
    assert empty.nrow == 0 and (empty.nmerged, empty.nmoved, empty.nkept) == (0, 0, 0)


@pytest.mark.parametrize("group", range(4))
def test_merge_fuzz(ea, group):
    """20 seeded tables of at most 3000 rows; the merged table passes the smoother's own order check"""
    for seed in range(5 * group, 5 * group + 5):
        rng = np.random.default_rng(7000 + seed)
        t = S.random_cx(rng, int(rng.integers(1, 3001)) if seed % 5 else 3000)
        got = check_merge(ea, t, seed)
        merged = {k: got[k] for k in S.CX}
        assert S.is_sorted(merged)
        check_smooth(ea, merged, seed, bandwidth=50, min_sites=5, degree=1)
        if t["pos"].size > 500:
            assert got.nmerged > 20 and got.nmoved > 5 and got.nkept > 5


def test_merge_errors_write_nothing_and_keep_nothing(ea):
    from epialleler_amd import _lib
    gpu_merge(ea, S.MERGE_KAT)                                          # (the engine and its buffers exist from here on)
    before = allocations(ea)
    n = S.MERGE_KAT["pos"].size
    swapped = {k: v[[0, 2, 1] + list(range(3, n))] for k, v in S.MERGE_KAT.items()}
    for t, word in ((swapped, b"ascending"), (S.cx_table([(1, 1, 10, 7, 1, 1), (1, 1, 10, 7, 1, 1)]), b"ascending"),
                    (S.cx_table([(1, 3, 10, 7, 1, 1)]), b"strand"), (S.cx_table([(1, 0, 10, 7, 1, 1)]), b"strand"),
                    (S.cx_table([(1, 1, 10, 7, -1, 1)]), b"negative"), (S.cx_table([(1, 1, 10, 7, 1, -2 ** 31)]), b"negative"),
                    (S.MERGE_OVERFLOW, b"2^31 - 1"), (S.cx_table([(1, 1, 10, 7, 0, 2 ** 30), (1, 2, 11, 7, 0, 2 ** 30)]), b"2^31 - 1")):
        rc, counts, cols, msg = raw_merge(ea, t, 64)
        assert rc == _lib.EPI_ERR_ARG and word in msg and counts == (0, 0, 0, 0) and _untouched(cols), word
    want = S.merge_np(S.MERGE_KAT)
    need = want["pos"].size
    rc, counts, cols, msg = raw_merge(ea, S.MERGE_KAT, need - 1)
    assert rc == _lib.EPI_ERR_ARG and counts[0] == need and b"14 rows to write, room for 13" in msg and _untouched(cols)
    rc, counts, cols, msg = raw_merge(ea, S.MERGE_KAT, need)
    assert rc == _lib.EPI_OK and counts == (need, 2, 3, 4)
    for k, c in zip(S.CX, cols):
        assert np.array_equal(c[:need], want[k]), k
    rc, counts, cols, msg = raw_merge(ea, S.MERGE_KAT, -1)
    assert rc == _lib.EPI_ERR_ARG and b"negative" in msg
    with pytest.raises(ea.EpihipError) as ei:
        gpu_merge(ea, swapped)
    assert ei.value.code == _lib.EPI_ERR_ARG
    assert allocations(ea) == before                                    # successful and failing calls alike


# ---- smooth --------------------------------------------------------------------------------------------------------------

def _cluster_table(sizes, gap, rng):
    """One series of clusters of the given sizes, `gap` apart, sites 1 to 40 apart inside"""
    pos, at = [], 100
    for c in sizes:
        p = at + np.cumsum(rng.integers(1, 41, c))
        pos.append(p)
        at = int(p[-1]) + gap
    pos = np.concatenate(pos)
    cov = rng.poisson(5, pos.size)
    meth = rng.binomial(cov, 0.5)
    return S.series_table([(1, 1, S.CG, pos, meth, cov - meth)])


@pytest.mark.parametrize("min_sites", [1, 2, 3, 70])
@pytest.mark.parametrize("degree", [0, 1, 2])
def test_small_clusters(ea, min_sites, degree):
    rng = np.random.default_rng(min_sites)
    sizes = sorted({1, 2, 3, max(min_sites - 1, 1), min_sites, min_sites + 1})
    t = _cluster_table(sizes, 501, rng)
    for bandwidth in (1, 30, 1000):
        got = check_smooth(ea, t, (sizes, bandwidth), bandwidth=bandwidth, min_sites=min_sites, max_gap=500, degree=degree)
        assert got.ncluster == len(sizes)
    assert got["nsites"][0] == 1 and got["degree"][0] <= 0             # a cluster of one site: its own beta, or NaN
    assert set(np.unique(got["degree"]).tolist()) <= set(range(-1, degree + 1))


def test_cluster_cuts(ea):
    pos = np.asarray([100, 150, 250, 351, 400, 500])                   # gaps 50, 100, 101, 49, 100
    cov = np.asarray([4, 6, 3, 8, 2, 5])
    meth = np.asarray([1, 6, 0, 4, 2, 1])
    one = S.series_table([(1, 1, S.CG, pos, meth, cov - meth)])
    assert check_smooth(ea, one, bandwidth=1000, min_sites=3, max_gap=100).ncluster == 2       # a gap of max_gap does not cut
    assert check_smooth(ea, one, bandwidth=1000, min_sites=3, max_gap=101).ncluster == 1
    assert check_smooth(ea, one, bandwidth=1000, min_sites=3, max_gap=99).ncluster == 4
    assert check_smooth(ea, one, bandwidth=1000, min_sites=3, max_gap=0).ncluster == 6
    # an rname change cuts, however close the positions; so do the strand and the context
    two = S.series_table([(1, 1, S.CG, pos, meth, cov - meth), (2, 1, S.CG, pos + 1, meth, cov - meth), (2, 2, S.CG, pos + 1, cov - meth, meth),
                          (2, 1, S.CHH, pos + 2, meth, cov - meth)])
    got = check_smooth(ea, two, bandwidth=1000, min_sites=3)
    assert got.ncluster == 4 and got.max_window == 6


def test_zero_coverage(ea):
    rng = np.random.default_rng(9)
    pos, meth, unmeth = S.random_series(rng, 300, "uniform", zero_frac=0.5)
    dead = (pos * 0).astype(np.int64)
    t = S.series_table([(1, 1, S.CG, pos, meth, unmeth), (2, 1, S.CG, pos[:40], dead[:40], dead[:40])])
    for degree in (0, 2):
        got = check_smooth(ea, t, bandwidth=100, min_sites=5, degree=degree)
        live = got["rname"] == 1
        assert np.isnan(got["beta"][live]).sum() > 100 and not np.isnan(got["smoothed"][live]).all()
        assert np.isnan(got["smoothed"][~live]).all() and (got["degree"][~live] == -1).all() and (got["weight"][~live] == 0).all()
        assert (got["nsites"][~live] >= 3).all()                        # sites at any coverage (those at exactly H_i, at most two, are outside)


def test_large_positions(ea):
    rng = np.random.default_rng(10)
    gaps = rng.integers(1, 300, 400)
    pos = 2 ** 31 - 1 - np.cumsum(gaps)[::-1] + gaps[0]
    pos[-1] = 2 ** 31 - 1
    assert (np.diff(pos) > 0).all() and pos.max() == 2 ** 31 - 1
    cov = rng.poisson(6, pos.size)
    meth = rng.binomial(cov, 0.3)
    far = np.asarray([0, 1, 2 ** 30, 2 ** 31 - 2])                      # one cluster under max_gap 2^31 - 1: H up to 2^31 - 2
    t = S.series_table([(1, 1, S.CG, pos, meth, cov - meth), (1, 2, S.CG, far, far * 0 + 3, far * 0 + 1)])
    got = check_smooth(ea, t, bandwidth=1000, min_sites=70, max_gap=2 ** 31 - 1)
    assert got["halfwidth"].max() == 2 ** 31 - 2
    check_smooth(ea, t, bandwidth=2 ** 30, min_sites=3, max_gap=2 ** 31 - 1, degree=1)
    check_merge(ea, t)


@pytest.mark.parametrize("group", range(8))
def test_smooth_fuzz(ea, group):
    """40 seeded tables of at most 3000 rows: both strands and three contexts interleaved over two rnames"""
    for seed in range(5 * group, 5 * group + 5):
        rng = np.random.default_rng(9000 + seed)
        t = S.random_cx(rng, int(rng.integers(1, 3001)) if seed % 8 else 3000)
        kw = dict(bandwidth=int(rng.choice([1, 2, 50, 1000])), min_sites=int(rng.choice([1, 2, 3, 5, 20, 70])),
                  max_gap=int(rng.choice([0, 40, 300, 10 ** 8])), degree=int(rng.integers(0, 3)))
        got = check_smooth(ea, t, (seed, kw), **kw)
        if seed % 8 == 0:
            assert set(got["strand"].tolist()) == {1, 2} and set(got["context"].tolist()) == {S.CG, S.CHG, S.CHH}
            assert set(got["rname"].tolist()) == {1, 2}


def test_defaults_and_host_reports(ea):
    rng = np.random.default_rng(77)
    t = S.random_cx(rng, 2500)
    want = S.smooth_np(t)
    S.same(gpu_smooth(ea, t), want)
    host = ea.Report(t, LEVELS)
    got = ea.smoothCytosineReport(host)
    assert isinstance(got["smoothed"], np.ndarray) and got.levels == host.levels and (got.ncluster, got.max_window) == (want["ncluster"], want["max_window"])
    S.same(got, want)
    dev = ea.smoothCytosineReport(dev_report(ea, t), bandwidth=80, min_sites=9, degree=1)
    assert dev["smoothed"].is_cuda and dev.levels["rname"] == LEVELS
    S.same({k: v.cpu().numpy() for k, v in dev.items()}, S.smooth_np(t, bandwidth=80, min_sites=9, degree=1))
    m_host, m_want = ea.mergeCpgStrands(host), S.merge_np(t)
    assert isinstance(m_host["pos"], np.ndarray) and S.rows_of(m_host) == S.rows_of(m_want) and m_host.nmerged == m_want["nmerged"]
    m_dev = ea.mergeCpgStrands(dev_report(ea, t))
    assert m_dev["pos"].is_cuda and (m_dev.nmerged, m_dev.nmoved, m_dev.nkept) == (m_want["nmerged"], m_want["nmoved"], m_want["nkept"])
    # int64 host columns are taken when their values fit
    wide = ea.Report({k: v.astype(np.int64) for k, v in t.items()}, LEVELS)
    S.same(ea.smoothCytosineReport(wide), want)


def test_smooth_errors_write_nothing_and_keep_nothing(ea):
    from epialleler_amd import _lib
    ok = S.MERGE_KAT
    gpu_smooth(ea, ok)
    before = allocations(ea)
    n = ok["pos"].size
    swapped = {k: v[[0, 2, 1] + list(range(3, n))] for k, v in ok.items()}
    for t, word in ((swapped, b"ascending"), (S.cx_table([(1, 1, 10, 7, 1, 1), (1, 1, 10, 7, 1, 1)]), b"ascending"),
                    (S.cx_table([(1, 2, 10, 7, 1, 1), (1, 1, 10, 7, 1, 1)]), b"ascending"), (S.cx_table([(1, 3, 10, 7, 1, 1)]), b"strand"),
                    (S.cx_table([(1, 0, 10, 7, 1, 1)]), b"strand"), (S.cx_table([(1, 1, 10, 8, 1, 1)]), b"context"),
                    (S.cx_table([(1, 1, 10, -1, 1, 1)]), b"context"), (S.cx_table([(1, 1, -10, 7, 1, 1)]), b"negative pos"),
                    (S.cx_table([(1, 1, 10, 7, -1, 1)]), b"negative count"), (S.cx_table([(1, 1, 10, 7, 1, -2 ** 31)]), b"negative count")):
        rc, ncluster, max_window, cols, msg = raw_smooth(ea, t)
        assert rc == _lib.EPI_ERR_ARG and word in msg and (ncluster, max_window) == (0, 0) and _untouched(cols), word
    for kw, word in ((dict(bandwidth=0), b"bandwidth"), (dict(bandwidth=2 ** 30 + 1), b"bandwidth"), (dict(min_sites=0), b"min_sites"),
                     (dict(min_sites=S.MAX_WINDOW + 1), b"min_sites"), (dict(max_gap=-1), b"max_gap"), (dict(degree=3), b"degree"),
                     (dict(degree=-1), b"degree")):
        rc, ncluster, max_window, cols, msg = raw_smooth(ea, ok, **kw)
        assert rc == _lib.EPI_ERR_ARG and word in msg and (ncluster, max_window) == (0, 0) and _untouched(cols), word
    rc, ncluster, max_window, cols, msg = raw_smooth(ea, S.cx_table([]))
    assert rc == _lib.EPI_OK and (ncluster, max_window) == (0, 0) and _untouched(cols)
    empty = gpu_smooth(ea, S.cx_table([]))
    assert empty.nrow == 0 and empty["smoothed"].dtype == np.float64 and (empty.ncluster, empty.max_window) == (0, 0)
    rc, ncluster, max_window, cols, msg = raw_smooth(ea, ok)
    want = S.smooth_np(ok)
    assert rc == _lib.EPI_OK and (ncluster, max_window) == (want["ncluster"], want["max_window"])
    S.same(dict(zip(S.SMOOTH_COLUMNS, cols)), want)
    with pytest.raises(ea.EpihipError) as ei:
        gpu_smooth(ea, swapped)
    assert ei.value.code == _lib.EPI_ERR_ARG
    assert allocations(ea) == before                                    # successful and failing calls alike


# ---- sequence ------------------------------------------------------------------------------------------------------------

def _host(rep):
    return {k: v.cpu().numpy().copy() for k, v in rep.items()}


@pytest.mark.parametrize("name,kw", [("amplicon010meth.bam", dict()), ("capture.bam", dict(threshold_reads=False, report_context="CX"))])
def test_report_merge_smooth_sequence(ea, name, kw):
    path = os.path.join(H.GOLDEN, "bam", name)
    bam = ea.preprocessBam(path)
    first = ea.generateCytosineReport(bam, as_device=True, **kw)
    first_host = _host(first)
    assert first.nrow > 50
    merged = ea.mergeCpgStrands(first)
    merged_host = _host(merged)
    live = allocations(ea)
    smooth_kw = dict(bandwidth=40, min_sites=7, max_gap=200)
    one = ea.smoothCytosineReport(merged, **smooth_kw)
    two = ea.smoothCytosineReport(merged, **smooth_kw)
    assert allocations(ea) == live
    one_host, two_host = _host(one), _host(two)
    S.same(two_host, one_host)
    for k in S.CX:                                                      # the inputs are unchanged
        assert np.array_equal(first[k].cpu().numpy(), first_host[k]) and np.array_equal(merged[k].cpu().numpy(), merged_host[k]), k
    want_m = S.merge_np(first_host)
    assert S.rows_of(merged_host) == S.rows_of(want_m)
    assert (merged.nmerged, merged.nmoved, merged.nkept) == (want_m["nmerged"], want_m["nmoved"], want_m["nkept"])
    assert merged.nmerged > 0 or name != "capture.bam"                  # (an amplicon may cover one strand only)
    S.same(one_host, S.smooth_np(merged_host, **smooth_kw))
    again = ea.generateCytosineReport(bam, as_device=True, **kw)
    for k in S.CX:
        assert np.array_equal(again[k].cpu().numpy(), first_host[k]), k
    whole = ea.generateSmoothedReport(bam, **kw, **smooth_kw)
    assert list(whole) == list(S.SMOOTH_COLUMNS) and isinstance(whole["smoothed"], np.ndarray) and whole.levels["rname"] == first.levels["rname"]
    S.same(whole, one_host)
    assert (whole.ncluster, whole.max_window, whole.nmerged, whole.nmoved, whole.nkept) == (one.ncluster, one.max_window, merged.nmerged,
                                                                                          merged.nmoved, merged.nkept)
    unmerged = ea.generateSmoothedReport(path, merge_strands=False, as_device=True, **kw, **smooth_kw)
    assert unmerged["smoothed"].is_cuda and not hasattr(unmerged, "nmerged")
    S.same(_host(unmerged), S.smooth_np(first_host, **smooth_kw))


def test_smoothed_report_to_file(ea, tmp_path):
    path = os.path.join(H.GOLDEN, "bam", "amplicon010meth.bam")
    out = str(tmp_path / "smoothed.tsv")
    assert ea.generateSmoothedReport(path, out, bandwidth=40, min_sites=7) is None
    rep = ea.generateSmoothedReport(path, bandwidth=40, min_sites=7)
    with open(out) as f:
        lines = f.read().splitlines()
    assert lines[0].split("\t") == list(S.SMOOTH_COLUMNS) and len(lines) == rep.nrow + 1
    cells = [line.split("\t") for line in lines[1:]]
    assert {c[1] for c in cells} <= {"+", "-"} and {c[3] for c in cells} == {"CG"}
    smoothed = np.asarray([float(c[10]) if c[10] else np.nan for c in cells])
    assert np.allclose(smoothed, rep["smoothed"], rtol=1e-14, atol=0, equal_nan=True) and not np.isnan(smoothed).all()
