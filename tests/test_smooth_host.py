"""mergeCpgStrands / smoothCytosineReport / generateSmoothedReport / rcpp_cx_merge_strands / rcpp_cx_smooth on the host side:
the exported symbols, the functions' signatures, argument checks before any I/O, the library's checks that need no device,
the loud failure without one (both steps run on the GPU; there is no CPU path), epi_cx_smooth_scratch_bytes, the merge
restatement (tests/smooth_np.py) on hand-written tables, the host epi_smooth_window bit for bit against the restatement,
and the restatement against exact rational arithmetic.

Measured on the CPU (test_restatement_against_exact_arithmetic prints it): over 15 604 windows of 200 seeded series (1 to
160 sites; uniform, geometric, bursty and all-1 gaps; 30 % of the sites without coverage; min_sites in {1, 2, 3, 5, 20, 70},
bandwidth in {1, 2, 50, 1000}) the largest absolute difference of `smoothed` from the exact fit of the same degree_used is
1.8e-12.  EXACT_BOUND is 8 times that, the margin test_gpu_cx_compare.py uses."""
import ctypes as C
import fractions
import inspect
import os
import re

import numpy as np
import pytest

import helpers as H
import smooth_np as S
import epialleler_amd as ea
from epialleler_amd import _lib

NEW_SYMBOLS = ("epi_cx_merge_strands_dev", "epi_cx_smooth_dev", "epi_cx_smooth_scratch_bytes", "epi_smooth_window", "epi_smooth_tile_sites",
               "epi_smooth_stage_sites")
EMPTY = inspect.Parameter.empty
SMOOTH_ARGS = [("bandwidth", 1000), ("min_sites", 70), ("max_gap", 10 ** 8), ("degree", 2)]
EXACT_MEASURED = 1.8e-12
EXACT_BOUND = 8 * EXACT_MEASURED


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_symbols_declared_exported_and_listed():
    _lib.build()
    with open(os.path.join(H.GOLDEN, "..", "..", "include", "epihip.h")) as f:
        text = f.read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(_lib.load(), name)
        assert re.search(r"\bint %s\(" % name, hdr)
    for name, value in (("EPI_SMOOTH_MAX_DEGREE", 2), ("EPI_SMOOTH_MAX_BANDWIDTH", 2 ** 30), ("EPI_SMOOTH_MAX_WINDOW", S.MAX_WINDOW)):
        assert re.search(r"^#define %s\s+%d$" % (name, value), hdr, flags=re.M), name
    with open(os.path.join(_lib.CSRC, "Makefile")) as f:
        mk = f.read()
    assert re.search(r"^SRCS := .*\bsmooth\.hip\b", mk, flags=re.M) and re.search(r"^HOST_SRCS := .*\bsmooth_host\.cpp\b", mk, flags=re.M)
    assert re.search(r"^smooth_host\.o: HOST_FPFLAGS := -fno-fast-math -ffp-contract=off$", mk, flags=re.M)
    assert re.search(r"^timing-smooth:", mk, flags=re.M)
    assert ea.SMOOTH_COLUMNS == S.SMOOTH_COLUMNS and ea.api.CX_COLUMNS == S.CX
    assert ea.CONTEXT_LEVELS[S.CG - 1] == "CG" and ea.CONTEXT_LEVELS[S.CHG - 1] == "CHG" and ea.CONTEXT_LEVELS[S.CHH - 1] == "CHH"
    lib = _lib.load()
    tile, stage = lib.epi_smooth_tile_sites(), lib.epi_smooth_stage_sites()
    assert 64 <= tile <= 1024 and tile % 64 == 0 and stage > tile and stage * 12 <= 64 * 1024


def test_signatures_and_defaults():
    p = inspect.signature(ea.mergeCpgStrands).parameters
    assert [(k, v.default) for k, v in p.items()] == [("report", EMPTY)]
    p = inspect.signature(ea.smoothCytosineReport).parameters
    assert [(k, v.default) for k, v in p.items()] == [("report", EMPTY)] + SMOOTH_ARGS
    p = inspect.signature(ea.rcpp_cx_merge_strands).parameters
    assert [(k, v.default) for k, v in p.items()] == [("rep", EMPTY), ("as_device", False)]
    p = inspect.signature(ea.rcpp_cx_smooth).parameters
    assert [(k, v.default) for k, v in p.items()] == [("rep", EMPTY)] + SMOOTH_ARGS + [("as_device", False)]
    p = inspect.signature(ea.generateSmoothedReport).parameters
    c = inspect.signature(ea.generateCytosineReport).parameters
    shared = [k for k in c if k not in ("gzip", "verbose", "as_device", "preprocess_args")]
    assert shared == ["bam", "report_file", "threshold_reads", "threshold_context", "min_context_sites", "min_context_beta",
                      "max_outofcontext_beta", "report_context"]
    assert [(k, v.default) for k, v in p.items() if v.kind is not v.VAR_KEYWORD] == \
        [(k, c[k].default) for k in shared] + [("merge_strands", True)] + SMOOTH_ARGS + [("gzip", False), ("verbose", False), ("as_device", False)]
    assert [k for k, v in p.items() if v.kind is v.VAR_KEYWORD] == ["preprocess_args"]


BAD_SMOOTH = [dict(bandwidth=0), dict(bandwidth=2 ** 30 + 1), dict(bandwidth=1.5), dict(bandwidth=True), dict(min_sites=0),
              dict(min_sites=S.MAX_WINDOW + 1), dict(min_sites=2.5), dict(min_sites=False), dict(max_gap=-1), dict(max_gap=2 ** 31),
              dict(max_gap=0.5), dict(degree=-1), dict(degree=3), dict(degree=1.5), dict(degree=True)]
BAD_REPORT = [dict(threshold_context="CpG"), dict(report_context="cg"), dict(merge_strands=1), dict(merge_strands=None)]
MESSAGES = {"threshold_context": "'threshold.context' should be one of 'CG', 'CHG', 'CHH', 'CxG', 'CX'",
            "report_context": "'report.context' should be one of 'CG', 'CHG', 'CHH', 'CxG', 'CX'",
            "merge_strands": "'merge.strands' should be TRUE or FALSE",
            "bandwidth": "'bandwidth' should be an integer from 1 to 1073741824", "min_sites": "'min.sites' should be an integer from 1 to 65536",
            "max_gap": "'max.gap' should be an integer from 0 to 2147483647", "degree": "'degree' should be an integer from 0 to 2"}


@pytest.mark.parametrize("kw", BAD_SMOOTH + BAD_REPORT)
def test_bad_arguments_raise_before_io(kw):
    with pytest.raises(ValueError) as ei:
        ea.generateSmoothedReport("no-such-file.bam", **kw)        # (opening it would raise "Unable to open BAM file")
    (name,) = kw
    assert MESSAGES[name] in str(ei.value) and "no-such-file" not in str(ei.value) and "open" not in str(ei.value)


@pytest.mark.parametrize("kw", BAD_SMOOTH)
def test_bad_smoothing_arguments_raise_before_the_device(kw):
    host = ea.Report(S.MERGE_KAT, ["chr1", "chr2"])
    (name,) = kw
    for fn in (ea.smoothCytosineReport, ea.rcpp_cx_smooth):        # (without a device the next step would raise EpihipError or TypeError)
        with pytest.raises(ValueError) as ei:
            fn(host, **kw)
        assert MESSAGES[name] in str(ei.value)


def test_good_arguments_reach_the_file():
    for kw in (dict(bandwidth=1, min_sites=1, max_gap=0, degree=0), dict(bandwidth=2 ** 30, min_sites=S.MAX_WINDOW, max_gap=2 ** 31 - 1),
               dict(merge_strands=False, report_context="CX", threshold_reads=False), dict(threshold_context=None, degree=1)):
        with pytest.raises(Exception) as ei:
            ea.generateSmoothedReport("no-such-file.bam", **kw)
        assert not isinstance(ei.value, ValueError) or "should be" not in str(ei.value)


def test_table_checks_need_no_device():
    with pytest.raises(TypeError) as ei:
        ea.mergeCpgStrands(ea.Report(dict(rname=np.zeros(1, np.int32)), ["chr1"]))
    assert "'strand'" in str(ei.value)
    bad = dict(S.MERGE_KAT)
    bad["meth"] = bad["meth"].astype(np.float64)
    for fn in (ea.mergeCpgStrands, ea.smoothCytosineReport):
        with pytest.raises(TypeError) as ei:
            fn(ea.Report(bad, ["chr1", "chr2"]))
        assert "'meth'" in str(ei.value)
    for fn in (ea.rcpp_cx_merge_strands, ea.rcpp_cx_smooth):      # host tables are no device Reports
        with pytest.raises(TypeError):
            fn(ea.Report(S.MERGE_KAT, ["chr1", "chr2"]))


def test_null_and_bad_arguments_of_the_library():
    lib = _lib.load()
    n = [C.c_int64(-1) for _ in range(4)]
    refs = [C.byref(x) for x in n]
    cols = (C.c_void_p * 9)()
    assert lib.epi_cx_merge_strands_dev(None, cols, 0, cols, 0, None, *refs) == _lib.EPI_ERR_ARG and b"NULL" in lib.epi_last_error()
    assert lib.epi_cx_smooth_dev(None, cols, 0, 1000, 70, 10 ** 8, 2, cols, cols, None, refs[0], refs[1]) == _lib.EPI_ERR_ARG
    assert b"NULL" in lib.epi_last_error() and n[0].value == 0 and n[1].value == 0
    assert lib.epi_cx_smooth_dev(None, cols, 0, 1000, 70, 10 ** 8, 2, cols, cols, None, None, refs[1]) == _lib.EPI_ERR_ARG
    # the limits come before anything else: no engine is needed to be told
    for args, word in (((0, 70, 1, 2), b"bandwidth"), ((2 ** 30 + 1, 70, 1, 2), b"bandwidth"), ((1000, 0, 1, 2), b"min_sites"),
                       ((1000, S.MAX_WINDOW + 1, 1, 2), b"min_sites"), ((1000, 70, -1, 2), b"max_gap"), ((1000, 70, 1, 3), b"degree"),
                       ((1000, 70, 1, -1), b"degree")):
        assert lib.epi_cx_smooth_dev(None, cols, 1, *args, cols, cols, None, refs[0], refs[1]) == _lib.EPI_ERR_ARG
        assert word in lib.epi_last_error(), args
    assert lib.epi_cx_smooth_dev(None, cols, -1, 1000, 70, 1, 2, cols, cols, None, refs[0], refs[1]) == _lib.EPI_ERR_ARG
    assert lib.epi_cx_smooth_dev(None, cols, 2 ** 31, 1000, 70, 1, 2, cols, cols, None, refs[0], refs[1]) == _lib.EPI_ERR_ARG
    assert b"rows" in lib.epi_last_error()


def test_scratch_bytes():
    lib = _lib.load()
    out = C.c_int64(-1)
    blocks = lambda n: (n + 4095) // 4096
    want = lambda n: 0 if n == 0 else 24 * n + blocks(n) * 2048 + 4 * ((7 * n + 2) // 2 * 2) + blocks(n) * 4 + 64
    for n in (0, 1, 2, 4096, 4097, 2 ** 31 - 1):
        assert lib.epi_cx_smooth_scratch_bytes(n, C.byref(out)) == _lib.EPI_OK and out.value == want(n), n
    assert want(1) == 24 + 2048 + 32 + 4 + 64 and want(2 ** 31 - 1) < 53 * 2 ** 31
    for n in (2 ** 31, -1):
        assert lib.epi_cx_smooth_scratch_bytes(n, C.byref(out)) == _lib.EPI_ERR_ARG and out.value == 0
    assert lib.epi_cx_smooth_scratch_bytes(1, None) == _lib.EPI_ERR_ARG


def test_fails_loudly_without_gpu():
    if _has_gpu():
        pytest.skip("GPU present")
    host = ea.Report(S.MERGE_KAT, ["chr1", "chr2"])
    t = H.templates_from_xm(["Z.z.Z.z", "z.Z.z.Z"], [1, 1], [1, 1])
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"], None)
    for call in (lambda: ea.mergeCpgStrands(host), lambda: ea.smoothCytosineReport(host), lambda: ea.generateSmoothedReport(bam)):
        with pytest.raises(ea.EpihipError) as ei:
            call()
        assert ei.value.code == 5 and "no CPU fallback" in str(ei.value)


# ---- the host function ---------------------------------------------------------------------------------------------------

def _host_window(pos, meth, unmeth, i, H_, degree):
    lib = _lib.load()
    p, m, u = (np.ascontiguousarray(x, np.int32) for x in (pos, meth, unmeth))
    sm, used, w = C.c_double(-1), C.c_int32(-9), C.c_double(-1)
    rc = lib.epi_smooth_window(C.c_void_p(p.ctypes.data), C.c_void_p(m.ctypes.data), C.c_void_p(u.ctypes.data), p.size, i, H_, degree,
                               C.byref(sm), C.byref(used), C.byref(w))
    return rc, sm.value, used.value, w.value


def test_host_window_arguments():
    lib = _lib.load()
    pos, meth, unmeth = np.asarray([5, 9, 20]), np.asarray([1, 0, 3]), np.asarray([1, 0, 0])
    assert _host_window(pos, meth, unmeth, 1, 100, 2)[0] == _lib.EPI_OK
    for i, H_, degree, word in ((3, 100, 2, b"site"), (-1, 100, 2, b"site"), (1, 0, 2, b"halfwidth"), (1, 100, 3, b"degree"), (1, 100, -1, b"degree")):
        assert _host_window(pos, meth, unmeth, i, H_, degree)[0] == _lib.EPI_ERR_ARG and word in lib.epi_last_error()
    assert _host_window(pos, np.asarray([1, -1, 3]), unmeth, 1, 100, 2)[0] == _lib.EPI_ERR_ARG
    x = C.c_double()
    assert lib.epi_smooth_window(None, None, None, 1, 0, 1, 0, C.byref(x), None, C.byref(x)) == _lib.EPI_ERR_ARG
    # a window of its own site: the site's beta; without coverage NaN and degree -1; a site at exactly H has weight 0
    assert _host_window(pos, meth, unmeth, 0, 4, 2)[1:] == (0.5, 0, 2.0)
    rc, sm, used, w = _host_window(pos, meth, unmeth, 1, 4, 2)
    assert rc == 0 and np.isnan(sm) and used == -1 and w == 0.0
    assert _host_window(pos, meth, unmeth, 0, 5, 1)[1:] == (0.5, 0, 2.0)       # site 9 is outside |d| < 4 + 1 only by its weight


def test_host_window_is_the_restatement_bit_for_bit():
    seen = set()
    n_windows = 0
    for seed in range(60):
        rng = np.random.default_rng(500 + seed)
        n = int(rng.integers(1, 161))
        pos, meth, unmeth = S.random_series(rng, n, S.GAP_KINDS[seed % 4], depth=int(rng.choice([1, 8, 200000])))
        degree = seed % 3
        r = S.smooth_series(pos, meth, unmeth, int(rng.choice([1, 2, 50, 1000])), int(rng.choice([1, 2, 3, 5, 20, 70])), 10 ** 8, degree)
        for i in range(n):
            rc, sm, used, w = _host_window(pos, meth, unmeth, i, int(r["halfwidth"][i]), degree)
            assert rc == 0 and used == r["degree"][i], (seed, i)
            assert np.float64(w).tobytes() == r["weight"][i].tobytes(), (seed, i)
            assert (np.isnan(sm) and np.isnan(r["smoothed"][i])) or np.float64(sm).tobytes() == r["smoothed"][i].tobytes(), (seed, i)
            seen.add((degree, used))
            n_windows += 1
    assert n_windows > 3000 and seen >= {(0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2), (2, -1)}


# ---- the restatement -----------------------------------------------------------------------------------------------------

def test_merge_restatement_on_the_hand_written_tables():
    got = S.merge_np(S.MERGE_KAT)
    assert S.rows_of(got) == S.rows_of(S.MERGE_KAT_WANT) and {k: got[k] for k in S.MERGE_KAT_COUNTS} == S.MERGE_KAT_COUNTS
    assert S.is_sorted(got) and got["pos"].size == S.MERGE_KAT["pos"].size - got["nmerged"]
    one = lambda *rows: S.rows_of(S.merge_np(S.cx_table(list(rows))))
    assert one((1, 1, 10, S.CG, 3, 1), (1, 2, 11, S.CG, 2, 4)) == [(1, 1, 10, S.CG, 5, 5)]                                    # a pair
    assert one((1, 2, 11, S.CG, 2, 4)) == [(1, 1, 10, S.CG, 2, 4)]                                                           # lone: moves
    assert one((1, 1, 10, S.CHH, 1, 1), (1, 2, 11, S.CG, 2, 4)) == [(1, 1, 10, S.CHH, 1, 1), (1, 2, 11, S.CG, 2, 4)]         # blocked by '+'
    assert one((1, 2, 10, S.CHG, 1, 1), (1, 2, 11, S.CG, 2, 4)) == [(1, 2, 10, S.CHG, 1, 1), (1, 2, 11, S.CG, 2, 4)]         # blocked by '-'
    assert one((1, 2, 1, S.CG, 2, 4)) == [(1, 2, 1, S.CG, 2, 4)]                                                             # q = 1
    assert one((1, 2, 2, S.CG, 2, 4)) == [(1, 1, 1, S.CG, 2, 4)]                                                             # q = 2
    assert one((1, 1, 9, S.CG, 1, 1), (1, 2, 11, S.CG, 2, 4)) == [(1, 1, 9, S.CG, 1, 1), (1, 1, 10, S.CG, 2, 4)]             # '+' CG two below
    assert one((1, 1, 10, S.CHG, 1, 0), (1, 2, 10, S.CHH, 0, 1), (1, 1, 11, S.CG, 0, 0)) == \
        [(1, 1, 10, S.CHG, 1, 0), (1, 2, 10, S.CHH, 0, 1), (1, 1, 11, S.CG, 0, 0)]                                           # non-CG rows, a lone '+'
    assert one((1, 1, 10, S.CG, 2 ** 31 - 2, 0), (1, 2, 11, S.CG, 1, 0)) == [(1, 1, 10, S.CG, 2 ** 31 - 1, 0)]
    with pytest.raises(ValueError, match="overflow"):
        S.merge_np(S.MERGE_OVERFLOW)
    for rows in ([(1, 1, 10, S.CG, 1, 1), (1, 1, 10, S.CG, 1, 1)], [(1, 3, 10, S.CG, 1, 1)], [(1, 1, 10, S.CG, -1, 1)]):
        with pytest.raises(ValueError, match="bad table"):
            S.merge_np(S.cx_table(rows))
    empty = S.merge_np(S.cx_table([]))
    assert empty["pos"].size == 0 and empty["nmerged"] == 0


def test_merge_restatement_on_fuzz_tables():
    for seed in range(10):
        rng = np.random.default_rng(40 + seed)
        t = S.random_cx(rng, int(rng.integers(1, 3001)))
        m = S.merge_np(t)
        assert S.is_sorted(m) and m["pos"].size == t["pos"].size - m["nmerged"]
        minus_cpg = int(((t["strand"] == 2) & (t["context"] == S.CG)).sum())
        assert m["nmerged"] + m["nmoved"] + m["nkept"] == minus_cpg
        for k in ("meth", "unmeth"):
            assert int(m[k].astype(np.int64).sum()) == int(t[k].astype(np.int64).sum())
        if t["pos"].size > 500:
            assert m["nmerged"] > 20 and m["nmoved"] > 5 and m["nkept"] > 5
        again = S.merge_np({k: m[k] for k in S.CX})
        assert again["nmerged"] == 0                                   # every pair is gone


def test_restatement_windows_by_hand():
    # five sites, unit coverage: min_sites 3 gives D = the distance to the second nearest other site
    pos, meth, unmeth = [10, 20, 40, 80, 81], [1, 0, 1, 0, 1], [0, 1, 0, 1, 0]
    r = S.smooth_series(pos, meth, unmeth, bandwidth=5, min_sites=3, max_gap=10 ** 8, degree=0)
    assert r["halfwidth"].tolist() == [30, 20, 30, 40, 41] and r["nsites"].tolist() == [2, 2, 2, 2, 2] and r["ncluster"] == 1
    assert r["halfwidth"].tolist() == [max(5, S.knn_distance(np.asarray(pos), i, 3)) for i in range(5)]
    # a gap equal to max_gap does not cut, one above it does; a cluster smaller than min_sites uses all of itself
    r = S.smooth_series(pos, meth, unmeth, bandwidth=5, min_sites=3, max_gap=40, degree=0)
    assert r["ncluster"] == 1
    r = S.smooth_series(pos, meth, unmeth, bandwidth=5, min_sites=3, max_gap=39, degree=0)
    assert r["ncluster"] == 2 and r["halfwidth"].tolist() == [30, 20, 30, 5, 5] and r["nsites"].tolist() == [2, 2, 2, 2, 2]
    # degree 0 is the weighted mean of the betas; a line through exactly linear betas extrapolates to the site's own
    pos = np.arange(0, 100, 10)
    meth, unmeth = np.arange(10) * 10, 90 - np.arange(10) * 10 + 10
    r = S.smooth_series(pos, meth, unmeth, bandwidth=35, min_sites=1, degree=1)
    assert (r["degree"] == 1).all() and np.allclose(r["smoothed"], meth / (meth + unmeth), atol=1e-14)
    # pos - H and pos + H do not decrease along a cluster
    rng = np.random.default_rng(3)
    for kind in S.GAP_KINDS:
        p, m, u = S.random_series(rng, 150, kind)
        for ms in (1, 2, 7, 70):
            r = S.smooth_series(p, m, u, 3, ms)
            assert (np.diff(p - r["halfwidth"]) >= 0).all() and (np.diff(p + r["halfwidth"]) >= 0).all()


def test_restatement_against_exact_arithmetic():
    worst, n_windows, used_seen = 0.0, 0, np.zeros(4, np.int64)
    for s in range(200):
        rng = np.random.default_rng(1000 + s)
        n = int(rng.integers(1, 161))
        pos, meth, unmeth = S.random_series(rng, n, S.GAP_KINDS[s % 4])
        min_sites, bandwidth = int(rng.choice([1, 2, 3, 5, 20, 70])), int(rng.choice([1, 2, 50, 1000]))
        degree = int(rng.integers(0, 3)) if s % 3 == 0 else 2
        r = S.smooth_series(pos, meth, unmeth, bandwidth, min_sites, 10 ** 8, degree)
        for i in range(n):
            used = int(r["degree"][i])
            used_seen[used + 1] += 1
            if used < 0:
                assert np.isnan(r["smoothed"][i]) and r["weight"][i] == 0.0
                continue
            exact = S.smooth_exact(pos, meth, unmeth, i, int(r["halfwidth"][i]), used)
            worst = max(worst, abs(float(exact - fractions.Fraction(float(r["smoothed"][i])))))
            n_windows += 1
    print("smoothed against exact rational arithmetic: %d windows, largest absolute error %.3g (bound %.3g); degree_used -1 .. 2: %s"
          % (n_windows, worst, EXACT_BOUND, used_seen.tolist()))
    assert n_windows > 14000 and (used_seen > 1000).all()
    assert worst <= EXACT_BOUND
