"""segmentCytosineReport on the GPU: epi_cx_segment_dev against the plain restatement (tests/segment_np.py) on hand-written
tables (no rows; chains of one, two and three sites; a model whose every path ties; runs of zero coverage; counts and positions
of 2^31 - 1 under the clip; max_coverage 1 and 5), on seeded fuzz tables (both strands and three contexts interleaved over two
rnames, depth 0 to 3, dyadic and random models), on a planted series that the refit recovers; every error, each writing
nothing; ownership; and the sequence of report, merge and segment on a fixture BAM.  test_gpu_segment_seams.py has the sizes at
the scans' thread and workgroup seams.

States, segments, counts and the score are compared exactly, the fit's doubles bit for bit: no tolerance anywhere."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers as H
import segment_np as G
import smooth_np as S

pytestmark = pytest.mark.gpu

LEVELS = ("chrA", "chrB", "chrC")
MARK = -7
DYADIC2 = ([0.25, 0.75], [[0.75, 0.25], [0.25, 0.75]], [0.5, 0.5])
MODEL3 = G.start_model((0.1, 0.5, 0.9), 0.9)


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


def gpu_segment(ea, t, model, **kw):
    rep = ea.rcpp_cx_segment(dev_report(ea, t), *model, **kw)
    assert list(rep) == list(G.SITE_COLUMNS) and list(rep.segments) == list(G.SEGMENT_COLUMNS)
    assert rep.levels["rname"] == LEVELS and rep.segments.levels["rname"] == LEVELS
    return rep


def same_result(got, want, t, what=""):
    for k in S.CX:
        assert np.array_equal(got[k], t[k]), (what, k)
    assert got["state"].dtype == np.int32 and np.array_equal(got["state"], want["state"]), (what, np.flatnonzero(got["state"] != want["state"])[:5])
    G.same_segments(got.segments, want["segments"], what)
    G.same_fit(got.fit, want["fit"], what)
    assert (got.nchain, got.nsegment) == (want["nchain"], want["nsegment"]), what


def check_segment(ea, t, model, what="", **kw):
    got, want = gpu_segment(ea, t, model, **kw), G.segment_np(t, *model, **kw)
    same_result(got, want, t, what)
    return got


def raw_segment(ea, t, model, max_gap=5000, max_coverage=1000, max_iter=10, cap=None, n=None, null=None, nstates=None):
    """epi_cx_segment_dev itself, into columns and outputs filled with a mark: (rc, (iterations, nchain, nsegment), columns, message)."""
    import torch
    from epialleler_amd import _lib, api
    lib = _lib.load()
    rep = dev_report(ea, t)
    rows = t["pos"].size
    cap = rows if cap is None else cap
    state = torch.full((max(rows, 1),), MARK, dtype=torch.int32, device="cuda")
    icols = list(torch.full((7, max(cap, 1)), MARK, dtype=torch.int32, device="cuda").unbind(0))
    dcols = list(torch.full((3, max(cap, 1)), float(MARK), dtype=torch.float64, device="cuda").unbind(0))
    p, trans, init = (np.ascontiguousarray(np.asarray(x, np.float64).reshape(-1)) for x in model)
    fit, nchain, nsegment = _lib.SegmentFit(), C.c_int64(MARK), C.c_int64(MARK)
    fit.iterations, fit.score = MARK, MARK
    in_cols, seg_i, seg_d, st = api._ptr_array([rep[k] for k in S.CX]), api._ptr_array(icols), api._ptr_array(dcols), C.c_void_p(state.data_ptr())
    if null == "in":
        in_cols[3] = None
    elif null == "seg_i":
        seg_i[6] = None
    elif null == "seg_d":
        seg_d[0] = None
    elif null == "state":
        st = None
    elif null == "all":
        in_cols = seg_i = seg_d = st = None
    rc = lib.epi_cx_segment_dev(api._engine(0), in_cols, rows if n is None else n, len(model[0]) if nstates is None else nstates, p.ctypes.data,
                                trans.ctypes.data, init.ctypes.data, max_gap, max_coverage, max_iter, st, seg_i, seg_d, cap, api._stream(0),
                                C.byref(fit), C.byref(nchain), C.byref(nsegment))
    torch.cuda.synchronize()
    return rc, (fit.iterations, nchain.value, nsegment.value), [c.cpu().numpy() for c in [state] + icols + dcols], lib.epi_last_error(), fit


def _untouched(cols):
    return all(np.all(c == MARK) for c in cols)


def one_series(meth, unmeth, pos=None, rname=1, strand=1, ctx=S.CG):
    meth, unmeth = np.asarray(meth, np.int64), np.asarray(unmeth, np.int64)
    pos = np.arange(1, meth.size + 1) * 10 if pos is None else np.asarray(pos, np.int64)
    return S.series_table([(rname, strand, ctx, pos, meth, unmeth)])


def low_depth(rng, t):
    """the table with depth 0 to 3 per row"""
    n = t["pos"].size
    cov = rng.integers(0, 4, n)
    meth = rng.binomial(cov, rng.random(n))
    out = dict(t)
    out["meth"], out["unmeth"] = meth.astype(np.int32), (cov - meth).astype(np.int32)
    return out


# ---- hand-written ----------------------------------------------------------------------------------------------------------

def test_no_rows(ea):
    got = gpu_segment(ea, S.cx_table([]), MODEL3)
    assert got.nrow == 0 and got.segments.nrow == 0 and got["state"].dtype == np.int32 and got.segments["beta"].dtype == np.float64
    assert (got.nchain, got.nsegment) == (0, 0) and got.fit["iterations"] == 0 and got.fit["score"] == 0 and got.fit["converged"] == 0
    G.same_fit(got.fit, G.segment_np(S.cx_table([]), *MODEL3)["fit"])
    rc, outs, cols, msg, fit = raw_segment(ea, S.cx_table([]), MODEL3)
    assert rc == 0 and outs == (0, 0, 0) and fit.score == 0 and fit.nstates == 3 and _untouched(cols)


@pytest.mark.parametrize("K", [2, 3, 4])
def test_short_chains(ea, K):
    rng = np.random.default_rng(K)
    for trial in range(6):
        model = G.random_model(rng, K, dyadic=trial % 2 == 0)
        # chains of 1, 2 and 3 sites: gaps above max_gap between them, two classes
        sizes = [1, 2, 3, 1, 1, 3, 2]
        pos = np.cumsum([100 if i == 0 else 1 for c in sizes for i in range(c)])
        cov = rng.integers(0, 4, pos.size)
        meth = rng.binomial(cov, 0.5)
        t = S.series_table([(1, 1, S.CG, pos, meth, cov - meth), (1, 2, S.CHH, pos[:3] + 1, meth[:3], cov[:3] - meth[:3])])
        for max_iter in (1, 4):
            got = check_segment(ea, t, model, (K, trial), max_gap=50, max_iter=max_iter)
            assert got.nchain == len(sizes) + 2                       # (the three CHH sites: one chain of 1, one of 2)
    one = check_segment(ea, S.cx_table([(2, 2, 5, S.CHG, 3, 1)]), G.random_model(rng, K, False), max_iter=3)
    assert (one.nchain, one.nsegment) == (1, 1) and one.segments["nsites"].tolist() == [1]


@pytest.mark.parametrize("K", [2, 3, 4])
def test_every_path_ties(ea, K):
    """all parameters equal and uniform: every delta ties, every psi and every end state is the smallest index"""
    rng = np.random.default_rng(20 + K)
    model = ([0.5] * K, [[1.0 / K] * K] * K, [1.0 / K] * K)
    n = 700
    cov = rng.integers(0, 4, n)
    meth = rng.binomial(cov, 0.5)
    t = one_series(meth, cov - meth)
    got = check_segment(ea, t, model, max_iter=1)
    assert (got["state"] == 0).all() and got.nsegment == 1
    assert got.fit["score"] == n * G.q(1.0 / K) + int(cov.sum()) * G.q(0.5)


def test_zero_coverage_runs(ea):
    rng = np.random.default_rng(31)
    n = 900
    cov = rng.poisson(6, n)
    cov[100:400] = 0
    cov[600:610] = 0
    cov[-50:] = 0
    meth = rng.binomial(cov, np.where(np.arange(n) < 500, 0.15, 0.85))
    dead = np.zeros(40, np.int64)
    t = S.series_table([(1, 1, S.CG, np.arange(n) * 7 + 3, meth, cov - meth), (2, 1, S.CG, np.arange(40) * 7 + 3, dead, dead)])
    for model, max_iter in ((MODEL3, 1), (MODEL3, 6), (DYADIC2, 1), (DYADIC2, 6)):
        got = check_segment(ea, t, model, max_iter=max_iter)
        live = got["rname"] == 1
        assert (got["state"][~live] == got["state"][~live][0]).all()
        assert np.isnan(got.segments["beta"][got.segments["rname"] == 2]).all() and not np.isnan(got.segments["beta"]).all()


def test_largest_counts_and_positions(ea):
    big = 2 ** 31 - 1
    pos = np.asarray([0, 1, 2 ** 30, big - 2, big - 1, big])
    meth = np.asarray([big, 0, big, 1, big, 7])
    unmeth = np.asarray([0, big, big, big, 1, 0])
    t = one_series(meth, unmeth, pos)
    for max_coverage in (1, 5, 1000, 32767):
        for max_gap in (big, 2 ** 30 - 2, 0):
            got = check_segment(ea, t, MODEL3, (max_coverage, max_gap), max_gap=max_gap, max_coverage=max_coverage, max_iter=3)
        assert got.nchain == 6 and got.segments["end"].max() == big
    got = check_segment(ea, t, MODEL3, max_gap=big, max_iter=1)
    assert got.nchain == 1 and got.segments["meth"].sum() == float(meth.sum()) and got.segments["unmeth"].sum() == float(unmeth.sum())
    assert got.segments["meth"].max() > 2 ** 31                        # a run's raw counts leave int32


@pytest.mark.parametrize("max_coverage", [1, 5])
def test_small_max_coverage(ea, max_coverage):
    rng = np.random.default_rng(max_coverage)
    n = 1500
    cov = rng.poisson(8, n)
    meth = rng.binomial(cov, np.where((np.arange(n) // 150) % 2 == 0, 0.1, 0.9))
    t = one_series(meth, cov - meth)
    for model, max_iter in ((MODEL3, 1), (DYADIC2, 1), (MODEL3, 5)):
        got = check_segment(ea, t, model, max_coverage=max_coverage, max_iter=max_iter)
    assert got.nsegment > 1


# ---- fuzz, refit -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("group", range(4))
def test_segment_fuzz(ea, group):
    """20 seeded tables of at most 3000 rows: both strands and three contexts interleaved over two rnames, depth 0 to 3"""
    for seed in range(5 * group, 5 * group + 5):
        rng = np.random.default_rng(11000 + seed)
        t = low_depth(rng, S.random_cx(rng, int(rng.integers(1, 3001)) if seed % 5 else 3000))
        K = 2 + seed % 3
        model = G.random_model(rng, K, dyadic=seed % 2 == 0)
        kw = dict(max_gap=int((40, 10 ** 8)[(seed // 2) % 2]), max_coverage=int(rng.choice([1, 2, 1000])), max_iter=(1, 5)[(seed // 4) % 2])
        got = check_segment(ea, t, model, (seed, kw), **kw)
        if seed % 5 == 0:
            assert set(got["strand"].tolist()) == {1, 2} and set(got["context"].tolist()) == {S.CG, S.CHG, S.CHH}
            assert set(got["rname"].tolist()) == {1, 2} and got.nchain >= 12


PLANTED = (0.1, 0.8)


@pytest.fixture(scope="module")
def planted():
    """about 20 000 sites in blocks of 500 that alternate between the two planted levels, depth 10; and the restatement's result
    from (0.3, 0.6), computed once"""
    rng = np.random.default_rng(2024)
    n = 20000
    level = np.where((np.arange(n) // 500) % 2 == 0, PLANTED[0], PLANTED[1])
    meth = rng.binomial(10, level)
    t = one_series(meth, 10 - meth, np.arange(n) * 50 + 1000)
    model = ([0.3, 0.6], [[0.9, 0.1], [0.1, 0.9]], [0.5, 0.5])
    return t, model, G.segment_np(t, *model)


def test_refit_recovers_a_planted_series(ea, planted):
    t, model, want = planted
    # the restatement itself meets the margin (checked here before the GPU is asked)
    assert all(abs(want["fit"]["p"][k] - PLANTED[k]) < 0.05 for k in range(2)) and want["fit"]["iterations"] > 1
    got = gpu_segment(ea, t, model)
    same_result(got, want, t)
    assert all(abs(got.fit["p"][k] - PLANTED[k]) < 0.05 for k in range(2))
    assert got.fit["trans"].shape == (2, 2) and got.fit["converged"] in (0, 1) and got.nsegment >= 40
    pure = check_segment(ea, t, model, max_iter=1)
    assert pure.fit["iterations"] == 1 and pure.fit["converged"] == 0 and pure.fit["p"].tolist() == [0.3, 0.6]


# ---- errors, ownership ---------------------------------------------------------------------------------------------------------

def test_errors_write_nothing_and_keep_nothing(ea):
    from epialleler_amd import _lib
    ok = S.MERGE_KAT
    gpu_segment(ea, ok, MODEL3)                                         # (the engine and its buffers exist from here on)
    before = allocations(ea)
    n = ok["pos"].size
    swapped = {k: v[[0, 2, 1] + list(range(3, n))] for k, v in ok.items()}
    nothing = (MARK, MARK, MARK)
    for t, word in ((swapped, b"ascending"), (S.cx_table([(1, 1, 10, 7, 1, 1), (1, 1, 10, 7, 1, 1)]), b"ascending"),
                    (S.cx_table([(1, 3, 10, 7, 1, 1)]), b"strand"), (S.cx_table([(1, 0, 10, 7, 1, 1)]), b"strand"),
                    (S.cx_table([(1, 1, 10, 8, 1, 1)]), b"context"), (S.cx_table([(1, 1, -10, 7, 1, 1)]), b"negative pos"),
                    (S.cx_table([(1, 1, 10, 7, -1, 1)]), b"negative count"), (S.cx_table([(1, 1, 10, 7, 1, -2 ** 31)]), b"negative count")):
        rc, outs, cols, msg, fit = raw_segment(ea, t, MODEL3)
        assert rc == _lib.EPI_ERR_ARG and word in msg and outs == nothing and fit.score == MARK and _untouched(cols), word
    p3, t3, i3 = MODEL3
    bad_models = [(([0.5], [[1.0]], [1.0]), 1, b"nstates"), (([0.5] * 5, [[0.2] * 5] * 5, [0.2] * 5), 5, b"nstates"),
                  (([0.0, 0.5, 0.9], t3, i3), None, b"p[0]"), (([0.1, 0.5, 1.0], t3, i3), None, b"p[2]"), (([0.1, float("nan"), 0.9], t3, i3), None, b"p[1]"),
                  ((p3, [[1.0, 0.0, 0.0]] + t3[1:], i3), None, b"trans[0][1]"), ((p3, [[0.9, 0.05, 0.06]] + t3[1:], i3), None, b"row 0"),
                  ((p3, t3[:2] + [[0.05, 0.05, 0.9 - 1e-8]], i3), None, b"row 2"), ((p3, t3, [0.5, 0.5, 2.0 ** -17]), None, b"init[2]"),
                  ((p3, t3, [0.5, 0.3, 0.3]), None, b"init does not sum")]
    for model, nstates, word in bad_models:
        rc, outs, cols, msg, fit = raw_segment(ea, ok, model, nstates=nstates)
        assert rc == _lib.EPI_ERR_ARG and word in msg and outs == nothing and _untouched(cols), word
    for kw, word in ((dict(max_coverage=0), b"max_coverage"), (dict(max_coverage=32768), b"max_coverage"), (dict(max_iter=0), b"max_iter"),
                     (dict(max_gap=-1), b"max_gap"), (dict(n=2 ** 26 + 1, null="all"), b"2^26"), (dict(null="in"), b"NULL column"),
                     (dict(null="seg_i"), b"NULL column"), (dict(null="seg_d"), b"NULL column"), (dict(null="state"), b"NULL"), (dict(cap=-1), b"negative")):
        rc, outs, cols, msg, fit = raw_segment(ea, ok, MODEL3, **kw)
        assert rc == _lib.EPI_ERR_ARG and word in msg and outs == nothing and _untouched(cols), word
    want = G.segment_np(ok, *MODEL3)
    need = want["nsegment"]
    assert need > 2
    rc, outs, cols, msg, fit = raw_segment(ea, ok, MODEL3, cap=need - 1)
    assert rc == _lib.EPI_ERR_ARG and outs == (MARK, MARK, need) and ("%d rows to write, room for %d" % (need, need - 1)).encode() in msg
    assert fit.score == MARK and _untouched(cols)
    rc, outs, cols, msg, fit = raw_segment(ea, ok, MODEL3, cap=need)
    assert rc == _lib.EPI_OK and outs == (want["fit"]["iterations"], want["nchain"], need) and fit.score == want["fit"]["score"]
    assert np.array_equal(cols[0], want["state"])
    G.same_segments(dict(zip(G.SEGMENT_COLUMNS, [c[:need] for c in cols[1:]])), want["segments"])
    with pytest.raises(ea.EpihipError) as ei:
        gpu_segment(ea, swapped, MODEL3)
    assert ei.value.code == _lib.EPI_ERR_ARG
    assert allocations(ea) == before                                    # successful and failing calls alike


def test_defaults_host_reports_and_repeat_calls(ea):
    rng = np.random.default_rng(78)
    t = S.random_cx(rng, 2500)
    before = {k: v.copy() for k, v in t.items()}
    model = G.start_model()
    want = G.segment_np(t, *model)
    host = ea.Report(t, LEVELS)
    got = ea.segmentCytosineReport(host)
    assert isinstance(got["state"], np.ndarray) and isinstance(got.segments["beta"], np.ndarray) and got.levels == host.levels
    same_result(got, want, t)
    rep = dev_report(ea, t)
    live = allocations(ea)
    one = ea.segmentCytosineReport(rep, state_beta=(0.2, 0.8), stay=0.95, max_gap=300, max_coverage=4, max_iter=3)
    two = ea.segmentCytosineReport(rep, state_beta=(0.2, 0.8), stay=0.95, max_gap=300, max_coverage=4, max_iter=3)
    assert allocations(ea) == live
    assert one["state"].is_cuda and one.segments["beta"].is_cuda and one.levels["rname"] == LEVELS
    want2 = G.segment_np(t, *G.start_model((0.2, 0.8), 0.95), max_gap=300, max_coverage=4, max_iter=3)
    for r in (one, two):
        host_r = ea.api._table_to_host(r, False)
        host_r.segments = ea.api._table_to_host(r.segments, False)
        same_result(host_r, want2, t)
    for k in S.CX:                                                      # the input is unchanged
        assert np.array_equal(rep[k].cpu().numpy(), before[k]) and np.array_equal(t[k], before[k]), k
    wide = ea.Report({k: v.astype(np.int64) for k, v in t.items()}, LEVELS)
    same_result(ea.segmentCytosineReport(wide), want, t)


# ---- sequence ------------------------------------------------------------------------------------------------------------------

def _host(rep):
    return {k: v.cpu().numpy().copy() for k, v in rep.items()}


@pytest.mark.parametrize("name,kw", [("amplicon010meth.bam", dict()), ("capture.bam", dict(threshold_reads=False, report_context="CX"))])
def test_report_merge_segment_sequence(ea, name, kw, tmp_path):
    path = os.path.join(H.GOLDEN, "bam", name)
    bam = ea.preprocessBam(path)
    first = ea.generateCytosineReport(bam, as_device=True, **kw)
    first_host = _host(first)
    merged = ea.mergeCpgStrands(first)
    merged_host = _host(merged)
    seg_kw = dict(state_beta=(0.1, 0.5, 0.9), stay=0.9, max_gap=200, max_coverage=50, max_iter=4)
    model = G.start_model(seg_kw["state_beta"], seg_kw["stay"])
    np_kw = {k: seg_kw[k] for k in ("max_gap", "max_coverage", "max_iter")}
    sites = ea.segmentCytosineReport(merged, **seg_kw)
    want = G.segment_np(merged_host, *model, **np_kw)
    assert want["nsegment"] > 1
    host_sites = ea.api._table_to_host(sites, False)
    host_sites.segments = ea.api._table_to_host(sites.segments, False)
    same_result(host_sites, want, merged_host)
    for k in S.CX:                                                      # the inputs are unchanged
        assert np.array_equal(first[k].cpu().numpy(), first_host[k]) and np.array_equal(merged[k].cpu().numpy(), merged_host[k]), k
    whole = ea.generateSegmentReport(bam, **kw, **seg_kw)
    assert list(whole) == list(G.SEGMENT_COLUMNS) and isinstance(whole["beta"], np.ndarray) and whole.levels["rname"] == first.levels["rname"]
    G.same_segments(whole, want["segments"])
    G.same_fit(whole.fit, want["fit"])
    assert list(whole.sites) == list(G.SITE_COLUMNS) and np.array_equal(whole.sites["state"], want["state"])
    assert (whole.nchain, whole.nsegment, whole.nmerged, whole.nmoved, whole.nkept) == (want["nchain"], want["nsegment"], merged.nmerged,
                                                                                      merged.nmoved, merged.nkept)
    unmerged = ea.generateSegmentReport(path, merge_strands=False, as_device=True, **kw, **seg_kw)
    assert unmerged["beta"].is_cuda and unmerged.sites["state"].is_cuda and not hasattr(unmerged, "nmerged")
    G.same_segments(_host(unmerged), G.segment_np(first_host, *model, **np_kw)["segments"])
    # the file is writeReport of the same segments
    out, ref = str(tmp_path / "segments.tsv"), str(tmp_path / "reference.tsv")
    assert ea.generateSegmentReport(bam, out, **kw, **seg_kw) is None
    ea.writeReport(whole, ref)
    with open(out) as f, open(ref) as g:
        text = f.read()
        assert text == g.read()
    lines = text.splitlines()
    assert lines[0].split("\t") == list(G.SEGMENT_COLUMNS) and len(lines) == whole.nrow + 1
    # the segments are regions: generateRegionReport takes them as they are
    if name == "amplicon010meth.bam":
        regions = ea.generateRegionReport(bam, whole)
        assert regions.nrow == whole.nrow
