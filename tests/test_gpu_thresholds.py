"""The read-thresholding decision (rcpp_threshold_reads.cpp:43-70) and lMHL's out-of-context filter
(rcpp_mhl_report.cpp:177-179) at ties, limits and odd thresholds, in every place the engine makes them: the per-read kernels
(narrow and wide), the fused CX tile kernel's device-built table, and the fused lMHL kernel's keep table -- each against the
CPU oracle and against the plain numpy restatement in helpers.py, and with the path that ran asserted."""
import numpy as np
import pytest

import helpers as H
import synth_np
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

NAN = float("nan")
NAN2 = float(np.uint64(0x7FF8000000000123).view(np.float64))      # a NaN with another payload


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


def pb(ea, t):
    return ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"], t.get("levels"))


def want_pass(t, c4, mn, mb, mo):
    """The oracle's flags, after checking that the numpy restatement agrees with them."""
    w = orc.threshold_reads(t["xm"], t["off"], *c4, mn, mb, mo)
    assert np.array_equal(H.threshold_np(t["xm"], t["off"], c4, mn, mb, mo), w), ("oracle vs restatement", c4, mn, mb, mo)
    return w


def threshold_launches(ea, fn):
    """fn() with the profiler on; returns (result, per-read thresholding launches): 0 when the tile kernel decided."""
    import ctypes as C
    lib = ea._lib.load()
    lib.epi_prof_reset()
    lib.epi_prof_enable(1)
    try:
        r = fn()
    finally:
        lib.epi_prof_enable(0)
    ms, cnt = C.c_double(0), C.c_int64(0)
    lib.epi_prof_get(b"threshold", C.byref(ms), C.byref(cnt))
    return r, cnt.value


def fused(ea, bam, t, c4, mn, mb, mo, rctx, want):
    """cytosine_report_fused: pass vector and table against the reference; returns the per-read launches it made."""
    H.dirty_allocator(bam)
    (rep, gp), k = threshold_launches(ea, lambda: ea.cytosine_report_fused(bam, *c4, mn, mb, mo, rctx, return_pass=True))
    assert np.array_equal(gp.astype(np.int32), want), ("fused pass", c4, mn, mb, mo, rctx)
    H.assert_reports_equal(dict(rep), orc.cx_report(t["xm"], t["off"], t["rname"], t["strand"], t["start"], want, rctx))
    return k


# thresholding context -> (report context equal to it: fused tile kernel when the batch allows, a different one: per-read first)
REPORTS = {"CG": ("Z", "ZXH"), "CHG": ("X", "Z"), "CX": ("ZXH", "Z")}


def check_grid(ea, t, grid=H.THRESHOLD_GRID, expect_fused=None):
    bam = pb(ea, t)
    try:
        for ctx, rctxs in REPORTS.items():
            c4 = H.cls4(ctx)
            for mn, mb, mo in grid:
                want = want_pass(t, c4, mn, mb, mo)
                got = ea.rcpp_threshold_reads(bam, *c4, mn, mb, mo)
                assert np.array_equal(got.astype(np.int32), want), ("threshold", ctx, mn, mb, mo)
                for rctx in rctxs:
                    k = fused(ea, bam, t, c4, mn, mb, mo, rctx, want)
                    if expect_fused is not None and bam.n:
                        assert k == (0 if (expect_fused and rctx == c4[0] and ctx != "CX") else 1), (ctx, rctx, k)
    finally:
        bam.close()


def test_tie_batch_grid(ea):
    t = H.tie_batch()
    check_grid(ea, t, expect_fused=True)
    bam = pb(ea, t)
    try:
        for mn, mb, mo in H.THRESHOLD_GRID:                          # the R-level keywords reach the decision
            for tctx, rctx in (("CG", "CG"), ("CHG", "CX")):
                want = want_pass(t, H.cls4(tctx), mn, mb, mo)
                rep = ea.generateCytosineReport(bam, threshold_context=tctx, report_context=rctx, min_context_sites=mn,
                                                min_context_beta=mb, max_outofcontext_beta=mo)
                H.assert_reports_equal(dict(rep), orc.cx_report(t["xm"], t["off"], t["rname"], t["strand"], t["start"], want,
                                                                H.CONTEXT_TO_BASES[rctx]["ctx_meth"]))
    finally:
        bam.close()


@pytest.mark.parametrize("kind", ["ragged", "pileup", "long_tail", "capture"])
def test_other_batches_grid(ea, kind):
    rng = np.random.default_rng(len(kind))
    if kind == "ragged":
        t = synth_np.random_templates(rng, 3000, 0, 400, 3, 20000, alphabet="..zZZzxXhH")
    elif kind == "pileup":
        t = synth_np.random_templates(rng, 5000, 100, 400, 1, 40, alphabet="..zZZzxXhH")
    elif kind == "long_tail":
        t = synth_np.with_long_tail(synth_np.random_templates(rng, 6000, 100, 310, 2, 60000, alphabet="..zZZzxXhH"), 97, 2500, first=5)
    else:
        t = H.bam("capture.bam")
    check_grid(ea, t)


def test_table_cache_follows_every_threshold(ea):
    """Successive fused calls on one batch where one threshold moves by one ulp (or min_n by one): the device table is
    rebuilt and the tie rows flip; a NaN with another payload changes nothing."""
    t = H.tie_batch(seed=3)
    c4 = H.cls4("CG")
    steps = [((2, 0.3, 0.1), None), ((2, 0.3, np.nextafter(0.1, 0)), True), ((2, 0.3, 0.1), True),
             ((2, np.nextafter(0.3, 1), 0.1), True), ((2, 0.3, 0.1), True), ((3, 0.3, 0.1), True), ((2, 0.3, 0.1), True),
             ((2, NAN, 0.1), True), ((2, NAN2, 0.1), False), ((2, 0.3, NAN), True), ((2, 0.3, NAN2), False)]
    bam = pb(ea, t)
    try:
        prev = None
        for (mn, mb, mo), flips in steps:
            want = want_pass(t, c4, mn, mb, mo)
            if flips is not None:
                assert (not np.array_equal(want, prev)) == flips, (mn, mb, mo)
            assert fused(ea, bam, t, c4, mn, mb, mo, "Z", want) == 0          # the tile kernel decided (the cached table)
            prev = want
    finally:
        bam.close()


def test_mhl_keep_table_cache(ea):
    """The fused lMHL kernel's keep table follows max_oo by one ulp, both ways; NaN payloads keep every read."""
    t = H.tie_batch(seed=4)
    bam = pb(ea, t)
    try:
        prev = None
        for moo, flips in ((0.1, None), (np.nextafter(0.1, 0), True), (0.1, True), (NAN, True), (NAN2, False), (0.1, True)):
            got = dict(ea.rcpp_mhl_report(bam, "Zz", 0, 0, moo))
            want = mhl_want(t, "Zz", 0, 0, moo)
            H.assert_reports_equal(got, want, float_cols=("length", "lmhl"))
            if flips is not None:
                assert (not (got["coverage"].size == prev["coverage"].size and np.array_equal(got["coverage"], prev["coverage"]))) == flips, moo
            prev = got
    finally:
        bam.close()


def mhl_want(t, ctx, hmax, hmin, moo):
    """The oracle's lMHL report, after checking it against the oracle's unfiltered report of the reads mhl_keep_np keeps."""
    want = orc.mhl_report(t["xm"], t["off"], t["rname"], t["strand"], t["start"], ctx, hmax, hmin, moo)
    s = H.subset(t, H.mhl_keep_np(t["xm"], t["off"], ctx, hmin, moo))
    H.assert_reports_equal(orc.mhl_report(s["xm"], s["off"], s["rname"], s["strand"], s["start"], ctx, hmax, 0, NAN), want,
                           float_cols=("length", "lmhl"))
    return want


@pytest.mark.parametrize("fused_mhl", ["1", "0"])
def test_mhl_out_of_context_ties(ea, hook_env, fused_mhl):
    """oo_m / oo_all exactly at 0.1 (1/10, 3/30, 7/70), one below and one above; max_oo 0, 0.1, NaN, -0.5; hmin equal to
    the haplotype length of some rows -- on the fused lMHL kernel and on the two-kernel path."""
    hook_env("EPIHIP_MHL_FUSED", fused_mhl)
    t = H.tie_batch(seed=5)
    bam = pb(ea, t)
    try:
        for ctx in ("Zz", "Xx"):
            for moo in (0.0, 0.1, NAN, -0.5):
                for hmax, hmin in ((0, 0), (0, 10), (3, 30), (0, 70)):
                    got = ea.rcpp_mhl_report(bam, ctx, hmax, hmin, moo)
                    H.assert_reports_equal(dict(got), mhl_want(t, ctx, hmax, hmin, moo), float_cols=("length", "lmhl"))
    finally:
        bam.close()


# ---- 16-bit and path limits --------------------------------------------------------------------------------------

def limit_batch(rng, long_rows, n_short):
    """n_short short random rows and the given long rows (strings of in-context / out-of-context letters), at random starts."""
    xs = ["".join(rng.choice(list("..zZZzxXh"), int(rng.integers(20, 150)))) for _ in range(n_short)]
    xs += long_rows
    n = len(xs)
    return H.templates_from_xm(xs, [int(v) for v in rng.integers(1, 200000, n)], [int(v) for v in rng.integers(1, 3, n)])


def shuffled(rng, counts):
    s = np.concatenate([np.full(k, ord(ch), np.uint8) for ch, k in counts])
    rng.shuffle(s)
    return s.tobytes().decode("latin1")


def test_fused_table_last_entry(ea):
    """A row of 64 999 in-context bytes among 300 rows: fused, and n_all indexes the table's last entry; n_m one below, at
    and one above the least passing count.  At 65 000 bytes, or with 1 % + 1 long rows, the batch falls back."""
    rng = np.random.default_rng(7)
    L = 64999
    k = 32500
    mb_tie = k / L
    longs = [shuffled(rng, (("Z", m), ("z", L - m))) for m in (k - 1, k, k + 1)]
    o_long = shuffled(rng, (("Z", 1), ("X", 6499), ("x", L - 1 - 6499)))             # o_all = 64 998 at 0.1 exactly ~ 6499.8
    c4 = H.cls4("CG")
    grid = ((2, mb_tie, 0.1), (2, np.nextafter(mb_tie, 1), 0.1), (2, 0.5, 0.1), (L, 0.0, 1.0), (L + 1, 0.0, 1.0),
            (1, 0.0, 6499 / (L - 1)), (1, 0.0, np.nextafter(6499 / (L - 1), 0)), (70000, 0.5, 0.1))
    cases = [(longs, 297, True),                                     # 3 of 300 long: 1 %
             ([s + "z" for s in longs], 297, False),                 # 65 000 bytes
             (longs + [o_long], 296, False)]                         # 4 of 300
    for rows, n_short, is_fused in cases:
        t = limit_batch(rng, rows, n_short)
        bam = pb(ea, t)
        try:
            for mn, mb, mo in grid:
                want = want_pass(t, c4, mn, mb, mo)
                got = ea.rcpp_threshold_reads(bam, *c4, mn, mb, mo)
                assert np.array_equal(got.astype(np.int32), want), (mn, mb, mo)
                assert fused(ea, bam, t, c4, mn, mb, mo, "Z", want) == (0 if is_fused else 1), (len(rows), is_fused)
        finally:
            bam.close()
    # the tie rows really sit on the boundary
    t = limit_batch(rng, longs, 0)
    assert sorted(want_pass(t, c4, 2, mb_tie, 0.1).tolist()) == [0, 1, 1]
    assert sorted(want_pass(t, c4, 2, np.nextafter(mb_tie, 1), 0.1).tolist()) == [0, 0, 1]


@pytest.mark.parametrize("wide", ["1", "0"])
def test_per_read_kernel_16_bit_limits(ea, hook_env, wide):
    """Rows of 65 535 bytes (the wide kernel carries n_m / n_u and o_m / o_u as 16-bit halves) and 65 536 bytes (the batch
    takes the narrow kernel): n_m = 65 535, n_u = 65 534, o_m = 65 535, o_u = 65 534 against thresholds at the tie."""
    hook_env("EPIHIP_PR_WIDE", wide)
    rng = np.random.default_rng(8)
    for L in (65535, 65536):
        rows = ["Z" * L,                                               # n_m = L (o_m = L under ooctx "ZX")
                shuffled(rng, (("z", L - 1), ("Z", 1))),               # n_u = L - 1
                shuffled(rng, (("Z", 32768), ("z", L - 32768))),
                shuffled(rng, (("Z", 1), ("X", L - 1))),               # o_m = L - 1
                shuffled(rng, (("Z", L - 1), ("x", 1))),               # o_m (ooctx "ZX") = L - 1, o_u = 1
                "z" * L]
        t = limit_batch(rng, rows, 40)
        bam = pb(ea, t)
        try:
            for c4 in (H.cls4("CG"), ("Z", "z", "ZX", "x")):
                for mn, mb, mo in ((L, 0.0, 1.0), (L + 1, 0.0, 1.0), (1, 1 / (L - 1), 1.0), (1, 1 / L, 1.0), (1, np.nextafter(1 / L, 1), 1.0),
                                   (1, 0.0, (L - 1) / L), (1, 0.0, np.nextafter((L - 1) / L, 0)), (1, 32768 / L, 0.1), (2, 0.5, 0.1)):
                    want = want_pass(t, c4, mn, mb, mo)
                    got = ea.rcpp_threshold_reads(bam, *c4, mn, mb, mo)
                    assert np.array_equal(got.astype(np.int32), want), (L, c4, mn, mb, mo)
                gb = ea.rcpp_get_xm_beta(bam, c4[0], c4[1])
                assert np.array_equal(gb.view(np.uint64), orc.get_xm_beta(t["xm"], t["off"], c4[0], c4[1]).view(np.uint64))
            want = want_pass(t, H.cls4("CG"), 2, 0.5, 0.1)
            assert fused(ea, bam, t, H.cls4("CG"), 2, 0.5, 0.1, "Z", want) == 1        # rows of 65 000 bytes and more: per-read first
        finally:
            bam.close()
