"""compareCytosineGroups on the GPU: epi_cx_groups_dev against the numpy restatement (tests/cx_groups_np.py) on seeded
random tables for every test, group size and minimum; one sample a side with the Fisher test against rcpp_cx_compare on
the fixture BAMs; the degenerate cases; every error, each writing nothing; ownership; and composition with adjustReport,
rcpp_cx_compare_regions, writeReport and the cytosine reports the tables came from.  test_gpu_cx_groups_seams.py has the
row counts at the workgroup, scan and sort tiles and the key's ends.

Integer columns, the betas, means, variances, phi, df and Welch's stat are compared bit for bit.  G (stat of lrt and
lrt_mn) and p go through the device's log / exp / lgamma / erfc and are compared within 8 times the largest
device-host relative difference measured on an MI355X (cx_groups_np.DEV_HOST_MEASURED; every comparison prints its
own figure); the Fisher p within test_gpu_cx_compare.py's bound."""
import ctypes as C
import os

import numpy as np
import pytest

import cx_compare_np as X
import cx_groups_np as G
import helpers as H

pytestmark = pytest.mark.gpu

FISHER_RTOL = 8 * 1.405e-14          # test_gpu_cx_compare.py: the device Fisher test against the host's, measured
LEVELS = ("chrA", "chrB", "chrC")
BITWISE = ("beta_a", "beta_b", "delta_beta", "mean_beta_a", "mean_beta_b", "var_a", "var_b", "phi", "df")


@pytest.fixture(scope="module")
def ea():
    import epialleler_amd
    return epialleler_amd


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def dev_report(ea, t, levels=LEVELS):
    import torch
    return ea.Report({k: torch.from_numpy(np.ascontiguousarray(t[k])).cuda() for k in X.CX}, levels)


def gpu_groups(ea, a, b, min_coverage=1, min_a=None, min_b=None, test="lrt"):
    rep = ea.rcpp_cx_compare_groups([dev_report(ea, t) for t in a], [dev_report(ea, t) for t in b], min_coverage, min_a, min_b, test)
    assert list(rep) == list(G.GROUP_COLUMNS) and rep.levels["rname"] == LEVELS
    return rep


def assert_groups_equal(got, want, test, what=""):
    assert got.nsites == want["nsites"]
    for k in G.GROUP_INT:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), k
    for k in BITWISE:
        assert got[k].dtype == np.float64 and np.array_equal(bits(got[k]), bits(want[k])), k
    cells = np.stack([want[k] for k in ("meth_a", "unmeth_a", "meth_b", "unmeth_b")], 1).reshape(-1, 4)
    if test == "fisher":
        assert np.isnan(got["stat"]).all()
        rel_stat, rel_p = 0.0, X.compare_p(got["p"], want["p"], cells, FISHER_RTOL) if cells.size else 0.0
    else:
        if test == "welch":                                     # one sqrt and one division of bitwise-equal operands
            assert np.array_equal(bits(got["stat"]), bits(want["stat"]))
        rel_stat, rel_p = G.rel_diff(got["stat"], want["stat"]), G.rel_diff(got["p"], want["p"])
        print("  %s %s: %d rows, device-host relative difference stat %.3e, p %.3e" % (what, test, want["pos"].size, rel_stat, rel_p))
        assert rel_stat <= G.DEV_HOST_RTOL and rel_p <= G.DEV_HOST_RTOL, (rel_stat, rel_p)
    return rel_stat, rel_p


# ---- one sample a side -------------------------------------------------------------------------------------------------

def _fixture_report(ea, name):
    return ea.generateCytosineReport(os.path.join(H.GOLDEN, "bam", name), threshold_reads=False, as_device=True)


@pytest.mark.parametrize("names", [("amplicon000meth.bam", "amplicon010meth.bam"), ("amplicon010meth.bam", "amplicon100meth.bam"),
                                   ("amplicon100meth.bam", "amplicon000meth.bam"), ("capture.bam", "capture.bam")])
def test_fisher_with_one_sample_a_side_is_rcpp_cx_compare(ea, names):
    ra, rb = _fixture_report(ea, names[0]), _fixture_report(ea, names[1])
    for min_coverage in (1, 10):
        two = ea.rcpp_cx_compare(ra, rb, min_coverage)
        grp = ea.rcpp_cx_compare_groups([ra], [rb], min_coverage, test="fisher")
        assert two.nrow > (50 if min_coverage == 1 else 0) and grp.nrow == two.nrow and grp.nsites >= grp.nrow and grp.levels == two.levels
        for k in X.CMP_INT:
            assert np.array_equal(grp[k], two[k]), k
        for k in X.CMP_FLOAT:                                   # p too: the same device function of the same table
            assert np.array_equal(bits(grp[k]), bits(two[k])), k
        assert np.all(grp["nsamples_a"] == 1) and np.all(grp["nsamples_b"] == 1) and np.isnan(grp["var_a"]).all()
        assert np.array_equal(bits(grp["mean_beta_a"]), bits(grp["beta_a"])) and np.array_equal(bits(grp["mean_beta_b"]), bits(grp["beta_b"]))


# ---- against the restatement -------------------------------------------------------------------------------------------

SHAPES = {"1+1": (1, 1, 300, 400), "2+1": (2, 1, 300, 400), "3+3": (3, 3, 300, 400), "32+32": (32, 32, 85, 90)}


@pytest.fixture(scope="module")
def tables():
    rng = np.random.default_rng(2024)
    out = {k: G.random_groups(rng, *v) for k, v in SHAPES.items()}
    out["3+3 disjoint"] = G.random_groups(rng, 3, 3, 100, 150, disjoint=True)
    return out


@pytest.mark.parametrize("test", ["fisher", "lrt", "lrt_mn", "welch"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_random_tables(ea, tables, shape, test):
    a, b = tables[shape]
    mins = {(1, 1), (len(a), len(b)), (max(len(a) // 2, 1), max(len(b) * 3 // 4, 1))}
    for min_a, min_b in sorted(mins):
        want = G.groups_np(a, b, 3, min_a, min_b, test)
        got = gpu_groups(ea, a, b, 3, min_a, min_b, test)
        assert_groups_equal(got, want, test, "%s min %d+%d" % (shape, min_a, min_b))
        assert want["nsites"] >= want["pos"].size > (5 if (min_a, min_b) == (1, 1) else -1)
    # None means every sample of the group; min_coverage 0 is 1
    got = gpu_groups(ea, a, b, 0, None, None, test)
    assert_groups_equal(got, G.groups_np(a, b, 1, len(a), len(b), test), test, shape + " all")


@pytest.mark.parametrize("test", ["fisher", "lrt", "lrt_mn", "welch"])
def test_disjoint_position_sets(ea, tables, test):
    """No site is shared: one group never counts anywhere, which gives 0 rows with the right nsites."""
    a, b = tables["3+3 disjoint"]
    want = G.groups_np(a, b, 1, 1, 1, test)
    got = gpu_groups(ea, a, b, 1, 1, 1, test)
    assert want["pos"].size == 0 and want["nsites"] > 400 and got.nrow == 0 and got.nsites == want["nsites"]
    assert list(got) == list(G.GROUP_COLUMNS) and got["p"].dtype == np.float64 and got["pos"].dtype == np.int32
    # b is empty altogether; then everything is
    empty = X.cx_table([])
    got = gpu_groups(ea, a, [empty], 1, 1, 1, test)
    assert got.nrow == 0 and got.nsites == G.groups_np(a, [empty], 1, 1, 1, test)["nsites"] > 100
    got = gpu_groups(ea, [empty, empty], [empty], 1, None, None, test)
    assert got.nrow == 0 and got.nsites == 0


def test_degenerate_statistics(ea):
    """n = 2 with lrt_mn; zero variance; pooled betas of 0 and 1; a group's variance undefined."""
    a = [X.cx_table([(1, 1, 10, 7, 5, 5), (1, 1, 20, 7, 10, 0), (1, 1, 30, 7, 0, 8), (1, 1, 40, 7, 2, 6), (1, 1, 50, 7, 9, 0), (1, 2, 60, 7, 4, 4)]),
         X.cx_table([(1, 1, 10, 7, 5, 5), (1, 1, 20, 7, 7, 0), (1, 1, 30, 7, 0, 3), (1, 1, 40, 7, 3, 9), (1, 1, 50, 7, 0, 9)])]
    b = [X.cx_table([(1, 1, 10, 7, 1, 9), (1, 1, 20, 7, 4, 0), (1, 1, 30, 7, 0, 5), (1, 1, 40, 7, 6, 2), (1, 1, 50, 7, 8, 0), (1, 2, 60, 7, 1, 7)]),
         X.cx_table([(1, 1, 10, 7, 2, 18), (1, 1, 20, 7, 6, 0), (1, 1, 30, 7, 0, 6), (1, 1, 40, 7, 9, 3), (1, 1, 50, 7, 0, 8)])]
    for test in ("fisher", "lrt", "lrt_mn", "welch"):
        for min_a, min_b in ((2, 2), (1, 1)):
            want = G.groups_np(a, b, 1, min_a, min_b, test)
            assert_groups_equal(gpu_groups(ea, a, b, 1, min_a, min_b, test), want, test, "degenerate")
        one = gpu_groups(ea, a[:1], b[:1], 1, 1, 1, test)
        assert_groups_equal(one, G.groups_np(a[:1], b[:1], 1, 1, 1, test), test, "n = 2")
    mn = gpu_groups(ea, a[:1], b[:1], 1, 1, 1, "lrt_mn")                # n = 2: df = 0 and no statistic
    assert mn.nrow == 6 and np.all(mn["df"] == 0) and np.isnan(mn["stat"]).all() and np.isnan(mn["phi"]).all() and np.isnan(mn["p"]).all()
    lrt, w = gpu_groups(ea, a, b, 1, 1, 1, "lrt"), gpu_groups(ea, a, b, 1, 1, 1, "welch")
    assert lrt["pos"].tolist() == [10, 20, 30, 40, 50, 60]
    assert lrt["stat"][1] == 0.0 and lrt["p"][1] == 1.0 and lrt["beta_a"][1] == 1.0        # all methylated
    assert lrt["stat"][2] == 0.0 and lrt["p"][2] == 1.0 and lrt["beta_b"][2] == 0.0        # none
    assert w["var_a"][0] == 0.0 and w["var_b"][0] == 0.0 and np.isnan(w["p"][0]) and np.isnan(w["stat"][0])      # s2 == 0
    assert w["var_a"][4] == 0.5 and not np.isnan(w["p"][4])                                 # sample betas 1 and 0
    assert np.isnan(w["var_a"][5]) and np.isnan(w["p"][5]) and w["nsamples_a"][5] == 1


# ---- errors and ownership ------------------------------------------------------------------------------------------------

def allocations(ea):
    live, nbytes = C.c_int64(-1), C.c_int64(-1)
    ea._lib.check(ea._lib.load().epi_device_allocations(C.byref(live), C.byref(nbytes)))
    return live.value, nbytes.value


def raw_groups(ea, a, b, cap, min_coverage=1, min_a=1, min_b=1, test=1, n_a=None, n_b=None):
    """epi_cx_groups_dev itself, into columns filled with a mark: (rc, nsite, nrow, columns, message)."""
    import torch
    from epialleler_amd import _lib, api
    lib = _lib.load()
    reps = [dev_report(ea, t) for t in list(a) + list(b)]
    cols = [r[k] for r in reps for k in X.CX]
    nrows = [t["pos"].size for t in list(a) + list(b)]
    icols = list(torch.full((10, max(cap, 1)), -7, dtype=torch.int32, device="cuda").unbind(0))
    dcols = list(torch.full((11, max(cap, 1)), -7.0, dtype=torch.float64, device="cuda").unbind(0))
    nsite, nrow = C.c_int64(-1), C.c_int64(-1)
    rc = lib.epi_cx_groups_dev(api._engine(0), api._ptr_array(cols), (C.c_int64 * len(nrows))(*nrows), len(a) if n_a is None else n_a,
                               len(b) if n_b is None else n_b, min_coverage, min_a, min_b, test, api._ptr_array(icols), api._ptr_array(dcols), cap,
                               api._stream(0), C.byref(nsite), C.byref(nrow))
    torch.cuda.synchronize()
    return rc, nsite.value, nrow.value, [c.cpu().numpy() for c in icols + dcols], lib.epi_last_error()


def _untouched(cols):
    return all(np.all(c == -7) for c in cols)


def test_errors_write_nothing_and_keep_nothing(ea):
    from epialleler_amd import _lib
    gpu_groups(ea, G.KAT_A, G.KAT_B)                                    # (the engine and its buffers exist from here on)
    before = allocations(ea)
    ok = G.KAT_A[0]
    swapped = {k: v[[0, 2, 1, 3, 4, 5]] for k, v in ok.items()}
    twice = X.cx_table([(1, 1, 10, 7, 1, 1), (1, 1, 10, 7, 1, 1)])
    strands = X.cx_table([(1, 2, 10, 7, 1, 1), (1, 1, 10, 7, 1, 1)])
    for a, b, which in (([swapped], [ok], b"table 0"), ([ok, ok], [ok, swapped], b"table 3"), ([ok], [twice], b"table 1"), ([strands], [ok], b"table 0")):
        rc, nsite, nrow, cols, msg = raw_groups(ea, a, b, 64)
        assert rc == _lib.EPI_ERR_ARG and which in msg and b"ascending" in msg and (nsite, nrow) == (0, 0) and _untouched(cols)
    # capacity: one too small returns the count needed
    want = G.groups_np(G.KAT_A, G.KAT_B, 1, 1, 1, "lrt")
    need = want["pos"].size
    assert need == 6
    rc, nsite, nrow, cols, msg = raw_groups(ea, G.KAT_A, G.KAT_B, need - 1)
    assert rc == _lib.EPI_ERR_ARG and nrow == need and nsite == want["nsites"] and b"6 rows to write, room for 5" in msg and _untouched(cols)
    rc, nsite, nrow, cols, msg = raw_groups(ea, G.KAT_A, G.KAT_B, need)
    assert rc == _lib.EPI_OK and (nsite, nrow) == (want["nsites"], need)
    for k, c in zip(G.GROUP_INT, cols):
        assert np.array_equal(c, want[k]), k
    # pooled coverage above 2^31 - 1 at a reported site; at a site that is not reported it is no error
    big = X.cx_table([(1, 1, 10, 7, 2 ** 30, 0), (1, 1, 20, 7, 1, 1)])
    small = X.cx_table([(1, 1, 20, 7, 1, 1)])
    rc, nsite, nrow, cols, msg = raw_groups(ea, [big, big], [big], 8)
    assert rc == _lib.EPI_ERR_ARG and b"2^31 - 1" in msg and _untouched(cols)
    rc, nsite, nrow, cols, msg = raw_groups(ea, [big, big], [small], 8)
    assert rc == _lib.EPI_OK and (nsite, nrow) == (2, 1) and cols[2][0] == 20
    rc, nsite, nrow, cols, msg = raw_groups(ea, [X.cx_table([(1, 1, 10, 7, 2 ** 31 - 1, 0)])], [big], 8, test=0)
    assert rc == _lib.EPI_OK and nrow == 1 and cols[4][0] == 2 ** 31 - 1 and cols[6][0] == 2 ** 30      # the largest pool that fits
    # a field outside the key's ranges
    for row in ((G.MAX_RNAME + 1, 1, 10, 7, 1, 1), (-1, 1, 10, 7, 1, 1), (1, 1, -5, 7, 1, 1), (1, 3, 10, 7, 1, 1), (1, 0, 10, 7, 1, 1),
                (1, 1, 10, 8, 1, 1), (1, 1, 10, -1, 1, 1), (1, 1, 10, 7, -1, 5), (1, 1, 10, 7, 5, -2 ** 31)):
        rc, nsite, nrow, cols, msg = raw_groups(ea, [ok], [X.cx_table([row])], 64)
        assert rc == _lib.EPI_ERR_ARG and b"rname code outside 0 .. 2097151" in msg and (nsite, nrow) == (0, 0) and _untouched(cols), row
    # arguments
    thirty_three = [small] * 33
    for kw, text in ((dict(a=thirty_three, b=[ok]), b"33 and 1 samples"), (dict(a=[ok], b=thirty_three), b"1 and 33 samples"),
                     (dict(a=[ok], b=[ok], n_a=0), b"0 and 1 samples"), (dict(a=[ok], b=[ok], min_a=2), b"min_samples_a = 2"),
                     (dict(a=[ok], b=[ok, ok], min_b=0), b"min_samples_b = 0"), (dict(a=[ok], b=[ok], test=4), b"test = 4"),
                     (dict(a=[ok], b=[ok], test=-1), b"test = -1"), (dict(a=[ok], b=[ok], cap=-1), b"negative capacity")):
        kw.setdefault("cap", 64)
        rc, nsite, nrow, cols, msg = raw_groups(ea, **kw)
        assert rc == _lib.EPI_ERR_ARG and text in msg and (nsite, nrow) == (0, 0) and _untouched(cols), text
    with pytest.raises(ValueError):
        gpu_groups(ea, thirty_three, [ok])
    with pytest.raises(ea.EpihipError) as ei:
        gpu_groups(ea, [swapped], [ok])
    assert ei.value.code == _lib.EPI_ERR_ARG
    assert allocations(ea) == before                                    # successful and failing calls alike


# ---- composition ---------------------------------------------------------------------------------------------------------

AMPLICONS = ("amplicon000meth.bam", "amplicon010meth.bam", "amplicon100meth.bam", "amplicon100meth.bam")


def _paths():
    p = [os.path.join(H.GOLDEN, "bam", n) for n in AMPLICONS]
    return p[:2], p[2:]


def _same(got, want):
    assert list(got) == list(want) and got.nrow == want.nrow
    for k in want:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k]), equal_nan=True), k


def _block_tables():
    """3 + 3 samples over 60 positions, coverage 20: beta about 0.2 everywhere in a, and in b 0.8 at positions 20 .. 39."""
    rng = np.random.default_rng(8)
    tabs = []
    for k in range(6):
        pos = np.arange(60)
        meth = np.where((k >= 3) & (pos >= 20) & (pos < 40), 16, 4) + rng.integers(-2, 3, 60)
        tabs.append(X.cx_table(np.stack([np.ones(60, np.int64), 1 + (pos & 1), 100 + pos, np.full(60, 7), meth, 20 - meth], 1)))
    return tabs[:3], tabs[3:]


@pytest.mark.parametrize("test", ["fisher", "lrt", "lrt_mn", "welch"])
def test_table_composes_with_adjust_and_regions(ea, test):
    a, b = _block_tables()
    dev = ea.rcpp_cx_compare_groups([dev_report(ea, t) for t in a], [dev_report(ea, t) for t in b], 3, None, None, test, as_device=True)
    assert dev.nrow == 60 and dev.nsites == 60
    adj = ea.adjustReport(dev, "BH")
    assert list(adj) == list(G.GROUP_COLUMNS) + ["q"] and adj.nsites == dev.nsites
    q = adj["q"].cpu().numpy()
    assert np.array_equal(q, ea.adjustPValues(dev["p"].cpu().numpy(), "BH"), equal_nan=True) and np.all(q[20:40] < 0.05)
    got = ea.rcpp_cx_compare_regions(adj, 0.05, 0.3, 5, 3, significance="q")
    # the same rows as a plain comparison table gives: the regions read the twelve columns they know, whatever else is there
    plain = ea.Report({k: adj[k] for k in ea.api.CX_COMPARE_COLUMNS + ("q",)}, LEVELS)
    _same(got, ea.rcpp_cx_compare_regions(plain, 0.05, 0.3, 5, 3, significance="q"))
    assert (got["start"].tolist(), got["end"].tolist(), got["nsites"].tolist(), got["direction"].tolist()) == ([120], [139], [20], [1])


def test_end_to_end_on_the_fixture_bams(ea, tmp_path):
    """generateGroupDmrReport equals its steps run one by one; compareCytosineGroups equals the join of the samples' own
    reports; files are written; the cytosine reports are afterwards what they were (the call is stateless)."""
    pa, pb = _paths()
    kw = dict(threshold_reads=False, min_coverage=5, min_samples=(1, 2), test="lrt_mn")
    bams = [ea.preprocessBam(p) for p in pa + pb]
    before = [ea.generateCytosineReport(x, threshold_reads=False) for x in bams]
    reps = [ea.generateCytosineReport(x, threshold_reads=False, as_device=True) for x in bams]
    step = ea.rcpp_cx_compare_groups(reps[:2], reps[2:], 5, 1, 2, "lrt_mn", as_device=True)
    host_tabs = [{k: r[k] for k in X.CX} for r in before]
    want = G.groups_np(host_tabs[:2], host_tabs[2:], 5, 1, 2, "lrt_mn")
    got = ea.compareCytosineGroups(pa, pb, **kw)
    assert got.nrow > 50 and got.levels == before[0].levels
    assert_groups_equal(got, want, "lrt_mn", "amplicons")
    _same(got, ea.api._table_to_host(step, False))
    _same(ea.compareCytosineGroups(bams[:2], bams[2:], **kw), got)      # preprocessBam results instead of paths
    region_kw = dict(max_q=0.05, min_delta_beta=0.2, max_gap=100, min_sites=2, p_adjust="BH")
    regions = ea.generateGroupDmrReport(pa, pb, **kw, **region_kw)
    by_hand = ea.adjustReport(ea.rcpp_cx_compare_regions(ea.adjustReport(step, "BH"), 0.05, 0.2, 100, 2, as_device=True, significance="q"), "BH")
    _same(regions, ea.api._table_to_host(by_hand, False))
    assert regions.nrow >= 1 and regions.nsites == got.nsites and list(regions) == list(ea.api.DMR_COLUMNS) + ["q"]
    # files
    assert ea.compareCytosineGroups(pa, pb, report_file=str(tmp_path / "grp.tsv"), **kw) is None
    assert ea.generateGroupDmrReport(pa, pb, report_file=str(tmp_path / "dmr.tsv.gz"), gzip=True, **kw, **region_kw) is None
    with open(tmp_path / "grp.tsv") as f:
        lines = f.read().split("\n")
    assert lines[0].split("\t") == list(G.GROUP_COLUMNS) and len(lines) == got.nrow + 2
    first = lines[1].split("\t")
    assert first[0] == got.levels["rname"][got["rname"][0] - 1] and first[1] in "+-" and first[2] == str(got["pos"][0]) and first[3] in ("CG", "CHG", "CHH")
    assert float(first[-1]) == pytest.approx(got["p"][0], rel=1e-14)
    import gzip
    assert gzip.open(tmp_path / "dmr.tsv.gz", "rt").readline().rstrip("\n").split("\t") == list(regions)
    # nothing changed on the batches
    for x, cx in zip(bams, before):
        H.assert_reports_equal(ea.generateCytosineReport(x, threshold_reads=False), cx)
