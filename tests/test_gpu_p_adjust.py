"""adjustPValues, adjustReport, the regions on q and generateAdjustedDmrReport against the numpy restatement of
tests/padjust_np.py (include/epihip.h: epi_p_adjust_dev).  Nothing in the restatement reads a GPU result.  q and order compare
bit for bit: every term is one IEEE division and / or multiplication, minimum and maximum are exact, and the order is the
stable one, so neither a launch shape nor the order among ties can show.

The sizes sit on the edges of a wave (64), a workgroup (256), a sorting tile and the u32 scan's block (4096), make the
[digit][workgroup] table larger than one scan block (65 537: 17 tiles x 256 digits) and take the scan of doubles through
several rounds of its carry kernel (300 001: 293 blocks of 1024 terms, 256 per round).  The contents choose which digit passes
run: all eight, only the lowest, only the exponent's, none.

The regions' pooled p compares with the host Fisher test as in test_gpu_cx_compare.py, with its tolerance."""
import ctypes as C

import numpy as np
import pytest

import cx_compare_np as X
import helpers as H
import padjust_np as P

pytestmark = pytest.mark.gpu

RTOL = 8 * 1.405e-14                   # test_gpu_cx_compare.py: device against host Fisher p
SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 65537, 300001)
LEVELS = ("chrA", "chrB", "chrC")


@pytest.fixture(scope="module")
def ea():
    import epialleler_amd
    return epialleler_amd


@pytest.fixture(scope="module")
def fisher_p(ea):
    """Real Fisher p-values: fisherExact on random small tables (many exact 1.0, many ties)."""
    rng = np.random.default_rng(99)
    t = rng.integers(0, 12, (max(SIZES), 4))
    p = ea.fisherExact(t[:, 0], t[:, 1], t[:, 2], t[:, 3])
    assert np.mean(p == 1.0) > 0.1 and not np.isnan(p).any()
    p.setflags(write=False)
    return p


def contents(n, fisher_p):
    rng = np.random.default_rng(1000 + n)
    u = rng.random(n)
    tiny = rng.random(n) ** 8
    tiny[::7] *= 1e-310                                                        # subnormals and zeros
    low = ((np.full(n, 0.3).view(np.uint64) & ~np.uint64(0xFF)) | rng.integers(0, 256, n).astype(np.uint64)).view(np.float64)
    edges = u.copy()
    for v in (0.0, -0.0, 1.0):
        edges[rng.random(n) < 0.1] = v
    if n >= 3:
        edges[[0, n // 2, n - 1]] = (1.0, -0.0, 0.0)
    return {"uniform": u, "pow8": tiny, "low_byte": low, "exponent": 2.0 ** -rng.integers(0, 1000, n).astype(np.float64),
            "equal": np.full(n, 0.37), "ties": np.round(rng.random(n), 2), "fisher": fisher_p[:n].copy(), "edges": edges,
            "nan10": np.where(rng.random(n) < 0.1, np.nan, u), "all_nan": np.full(n, np.nan)}


def raw(ea, p, method, n_tests=0, in_place=False, with_order=True, mark=-7.0):
    """epi_p_adjust_dev itself, into columns filled with a mark: (rc, m, q, order, message)."""
    import torch
    from epialleler_amd import _lib, api
    lib = _lib.load()
    n = int(np.size(p))
    dp = torch.from_numpy(np.ascontiguousarray(p, np.float64)).cuda()
    dq = dp if in_place else torch.full((max(n, 1),), mark, dtype=torch.float64, device="cuda")
    do = torch.full((max(n, 1),), -7, dtype=torch.int32, device="cuda")
    m = C.c_int64(-1)
    rc = lib.epi_p_adjust_dev(api._engine(0), C.c_void_p(dp.data_ptr()), n, P.CODES[method], n_tests, C.c_void_p(dq.data_ptr()),
                              C.c_void_p(do.data_ptr()) if with_order else None, api._stream(0), C.byref(m))
    torch.cuda.synchronize()
    return rc, m.value, dq.cpu().numpy()[:max(n, 1)], do.cpu().numpy(), lib.epi_last_error()


@pytest.mark.parametrize("n", SIZES)
def test_against_the_restatement(ea, fisher_p, n):
    from epialleler_amd import _lib
    for name, p in contents(n, fisher_p).items():
        want_order = P.order_np(p).astype(np.int32)
        for method in P.METHODS:
            want_q, _, want_m = P.adjust_np(p, method)
            rc, m, q, order, msg = raw(ea, p, method)
            assert rc == _lib.EPI_OK, (name, method, msg)
            assert m == want_m, (name, method)
            np.testing.assert_array_equal(q[:n], want_q, err_msg="%s %s q" % (name, method))
            np.testing.assert_array_equal(order[:n], want_order, err_msg="%s %s order" % (name, method))
            assert not np.signbit(q[:n][q[:n] == 0.0]).any()
        if n >= 257:                                                           # the passes this content is here for
            passes = P.digit_passes(p)
            assert {"equal": passes == 0, "all_nan": passes == 0, "low_byte": passes == 1, "exponent": passes == 2,
                    "uniform": passes >= 7}.get(name, True), (name, passes)


@pytest.mark.parametrize("method", P.METHODS)
def test_python_interface(ea, method):
    import torch
    rng = np.random.default_rng(3)
    p = np.where(rng.random(5000) < 0.05, np.nan, np.round(rng.random(5000), 3))
    want = P.adjust_np(p, method)[0]
    got = ea.adjustPValues(p, method)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(ea.adjustPValues(p.tolist(), method), want)
    dev = torch.from_numpy(p).cuda()
    before = dev.clone()
    out = ea.adjustPValues(dev, method, as_device=True)
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float64 and out.device == dev.device
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    assert torch.equal(dev.view(torch.int64), before.view(torch.int64))       # the input is left alone
    # float32 input: the values as doubles
    p32 = p.astype(np.float32)
    np.testing.assert_array_equal(ea.adjustPValues(torch.from_numpy(p32).cuda(), method), P.adjust_np(p32.astype(np.float64), method)[0])
    if method == "BH":
        np.testing.assert_array_equal(ea.adjustPValues(p, "fdr"), want)
        assert ea.adjustPValues([], method).shape == (0,)
        np.testing.assert_allclose(ea.adjustPValues([.01, .02, .03, .04, .05], "holm"), [.05, .08, .09, .09, .09], rtol=1e-15)


@pytest.mark.parametrize("method", P.METHODS)
def test_n_tests(ea, method):
    from epialleler_amd import _lib
    rng = np.random.default_rng(4)
    p = np.where(rng.random(1000) < 0.1, np.nan, rng.random(1000) ** 3)
    m = int((~np.isnan(p)).sum())
    for n_tests in (m, m + 1, 5000, 2 ** 31 - 1 if method != "BY" else 100000):
        np.testing.assert_array_equal(ea.adjustPValues(p, method, n_tests=n_tests), P.adjust_np(p, method, n_tests)[0])
    rc, got_m, q, order, msg = raw(ea, p, method, n_tests=m - 1)
    assert rc == _lib.EPI_ERR_ARG and got_m == m and b"n_tests" in msg
    assert np.all(q == -7.0) and np.all(order == -7)
    with pytest.raises(ea.EpihipError) as ei:
        ea.adjustPValues(p, method, n_tests=m - 1)
    assert ei.value.code == _lib.EPI_ERR_ARG


@pytest.mark.parametrize("bad", [1.5, -1e-9, np.inf, -np.inf, 1.0000000000000002, -5e-324])
def test_values_outside_the_unit_interval_are_refused(ea, bad):
    from epialleler_amd import _lib
    rng = np.random.default_rng(5)
    for n, at in ((1, 0), (300, 299), (5000, 4097)):
        p = rng.random(n)
        p[at] = bad
        for in_place in (False, True):
            rc, m, q, order, msg = raw(ea, p, "BH", in_place=in_place)
            assert rc == _lib.EPI_ERR_ARG and m == 0 and b"[0, 1]" in msg
            assert np.all(order == -7)
            np.testing.assert_array_equal(q, p if in_place else np.full(n, -7.0))   # nothing was written
    with pytest.raises(ea.EpihipError):
        ea.adjustPValues([0.5, bad])


@pytest.mark.parametrize("method", P.METHODS)
def test_in_place_and_without_order(ea, method):
    from epialleler_amd import _lib
    rng = np.random.default_rng(6)
    p = np.where(rng.random(9000) < 0.1, np.nan, np.round(rng.random(9000), 2))
    want_q, want_order, want_m = P.adjust_np(p, method)
    rc, m, q, order, _ = raw(ea, p, method, in_place=True)
    assert rc == _lib.EPI_OK and m == want_m
    np.testing.assert_array_equal(q, want_q)
    np.testing.assert_array_equal(order, want_order)
    rc, m, q, order, _ = raw(ea, p, method, with_order=False)
    assert rc == _lib.EPI_OK and m == want_m and np.all(order == -7)
    np.testing.assert_array_equal(q, want_q)


def test_on_a_side_stream(ea):
    import torch
    p = np.random.default_rng(8).random(70000)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dev = torch.from_numpy(p).cuda()
        got = ea.adjustPValues(dev, "BY", as_device=True)
    s.synchronize()
    np.testing.assert_array_equal(got.cpu().numpy(), P.adjust_np(p, "BY")[0])


# ---- tables ----------------------------------------------------------------------------------------------------------------

def dev_report(ea, t, names, levels=LEVELS):
    import torch
    return ea.Report({k: torch.from_numpy(np.ascontiguousarray(t[k])).cuda() for k in names}, levels)


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def test_adjust_report(ea):
    import torch
    table = X.random_comparison(np.random.default_rng(5), 1000)
    names = X.CMP_INT + X.CMP_FLOAT
    want = P.adjust_np(table["p"], "BH")[0]
    assert np.isnan(want).any()
    dev = dev_report(ea, table, names)
    dev.ncommon = 1234
    host = ea.Report({k: table[k].copy() for k in names}, LEVELS)
    host.ncommon = 1234
    for rep, on_device in ((dev, True), (host, False)):
        out = ea.adjustReport(rep, "BH")
        assert list(out) == list(names) + ["q"] and list(rep) == list(names) and out.ncommon == 1234 and out.levels == rep.levels
        assert (isinstance(out["q"], torch.Tensor) and out["q"].is_cuda) if on_device else isinstance(out["q"], np.ndarray)
        np.testing.assert_array_equal(out["q"].cpu().numpy() if on_device else out["q"], want)
        for k in names:
            assert out[k] is rep[k]
            np.testing.assert_array_equal(out[k].cpu().numpy() if on_device else out[k], table[k])
        again = ea.adjustReport(out, "holm", column="p", name="q_holm", n_tests=5000)
        assert list(again) == list(names) + ["q", "q_holm"]
        np.testing.assert_array_equal(again["q_holm"].cpu().numpy() if on_device else again["q_holm"], P.adjust_np(table["p"], "holm", 5000)[0])
    # other columns: the two strands' p-values of a VCF report
    vcf = ea.Report({"FEp+": np.asarray([0.01, np.nan, 0.5, 0.01]), "FEp-": np.asarray([1.0, 0.2, np.nan, 0.0])}, None)
    out = ea.adjustReport(ea.adjustReport(vcf, "BY", column="FEp+", name="q+"), "bonferroni", column="FEp-", name="q-")
    np.testing.assert_array_equal(out["q+"], P.adjust_np(vcf["FEp+"], "BY")[0])
    np.testing.assert_array_equal(out["q-"], P.adjust_np(vcf["FEp-"], "bonferroni")[0])


def assert_regions_equal(got, want):
    for k in X.DMR_INT:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), k
    for k in ("beta_a", "beta_b", "delta_beta", "mean_delta_beta"):
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    X.compare_p(got["p"], want["p"], want["cells"], RTOL)


@pytest.mark.parametrize("method,args", [("BH", (0.05, 0.1, 300, 1)), ("BH", (0.1, 0.1, 300, 1)), ("BH", (0.2, 0.1, 40, 3)),
                                         ("holm", (1.0, 0.0, 2 ** 31 - 1, 2)), ("BY", (0.8, 0.5, 100, 1)), ("none", (0.05, 0.1, 300, 1))])
def test_regions_on_q(ea, method, args):
    """The table of test_gpu_cx_compare.py::test_regions_random.  Its small p-values are uniform on (0, 0.05) in two rows of
    three, so BH lifts nearly all of them to about 0.076: at 0.05 one region is left of the 68 that p gives, at 0.1 all."""
    table = X.random_comparison(np.random.default_rng(5), 1000)
    rep = ea.adjustReport(dev_report(ea, table, X.CMP_INT + X.CMP_FLOAT), method)
    got = ea.rcpp_cx_compare_regions(rep, *args, significance="q")
    assert list(got) == list(X.DMR_INT + X.DMR_FLOAT)
    copy = dict(table)
    copy["p"] = P.adjust_np(table["p"], method)[0]
    want = X.regions_np(copy, *args)
    assert want["rname"].size == (1 if (method, args[0]) == ("BH", 0.05) else want["rname"].size) and want["rname"].size >= 1
    assert_regions_equal(got, want)
    on_p = ea.rcpp_cx_compare_regions(rep, *args)                               # the default still reads p
    assert_regions_equal(on_p, X.regions_np(table, *args))
    assert on_p.nrow > 60
    with pytest.raises(TypeError):
        ea.rcpp_cx_compare_regions(dev_report(ea, table, X.CMP_INT + X.CMP_FLOAT), *args, significance="q")   # no q column


# ---- end to end ------------------------------------------------------------------------------------------------------------

def _sample(seed, raised):
    """The two-sample fixture of test_gpu_cx_compare.py::test_end_to_end: 300 templates of 80 bases on two sequences and
    both strands, a CpG every 6 bases and a few CHH calls; methylation 0.3, in 300 .. 520 of the first sequence 0.15, or
    0.95 when `raised`."""
    rng = np.random.default_rng(seed)
    xms, starts, strands, rnames = [], [], [], []
    for _ in range(300):
        st, rn = int(rng.integers(1, 800)), int(rng.integers(1, 3))
        s = []
        for pos in range(st, st + 80):
            level = (0.95 if raised else 0.15) if rn == 1 and 300 <= pos <= 520 else 0.3
            if pos % 6 == 0:
                s.append("Z" if rng.random() < level else "z")
            elif pos % 17 == 0:
                s.append("H" if rng.random() < 0.03 else "h")
            else:
                s.append(".")
        xms.append("".join(s)); starts.append(st); strands.append(int(rng.integers(1, 3))); rnames.append(rn)
    return H.templates_from_xm(xms, starts, strands, rnames)


@pytest.fixture(scope="module")
def samples(ea):
    ta, tb = _sample(11, False), _sample(12, True)
    mk = lambda t: ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"], LEVELS[:2])
    return mk(ta), mk(tb)


def _read_tsv(path):
    with open(path) as f:
        rows = [ln.rstrip("\n").split("\t") for ln in f]
    return rows[0], rows[1:]


@pytest.mark.parametrize("p_adjust,max_q", [("BH", 0.05), ("BY", 0.2)])
def test_end_to_end(ea, samples, tmp_path, p_adjust, max_q):
    """(with the host Fisher test the restatement finds 6 regions for BH at 0.05 and 2 for BY at 0.2 in these samples; Holm,
    Hochberg and Bonferroni leave fewer than three neighbouring cytosines at any limit up to 0.2)"""
    import torch
    a, b = samples
    kw = dict(threshold_reads=False, min_coverage=4)
    region_kw = dict(min_delta_beta=0.2, max_gap=30, min_sites=3)
    before = [ea.generateCytosineReport(x, threshold_reads=False) for x in (a, b)]
    got = ea.generateAdjustedDmrReport(a, b, **kw, max_q=max_q, p_adjust=p_adjust, **region_kw)
    assert list(got) == list(X.DMR_INT + X.DMR_FLOAT) + ["q"] and got.levels["rname"] == LEVELS[:2]
    # the staged calls
    cmp_ = ea.compareCytosineReports(a, b, as_device=True, **kw)
    table = ea.adjustReport(cmp_, p_adjust)
    staged = ea.adjustReport(ea.rcpp_cx_compare_regions(table, max_q, 0.2, 30, 3, as_device=True, significance="q"), p_adjust)
    assert got.ncommon == cmp_.ncommon and got.nrow == staged.nrow
    for k in got:
        assert isinstance(got[k], np.ndarray) and np.array_equal(got[k], staged[k].cpu().numpy(), equal_nan=True), k
    # ... and the restatements on the device table's p
    host = {k: v.cpu().numpy() for k, v in table.items()}
    np.testing.assert_array_equal(host["q"], P.adjust_np(host["p"], p_adjust)[0])
    copy = dict(host)
    copy["p"] = host["q"]
    want = X.regions_np(copy, max_q, 0.2, 30, 3)
    print("rows %d, significant on p %d, on q %d, regions %d" % (host["p"].size, int(np.sum(host["p"] <= max_q)), int(np.sum(host["q"] <= max_q)),
                                                                  want["rname"].size))
    assert want["rname"].size >= 1 and np.any((want["rname"] == 1) & (want["direction"] == 1) & (want["start"] >= 300) & (want["end"] <= 520))
    assert_regions_equal(got, want)
    np.testing.assert_array_equal(got["q"], P.adjust_np(got["p"], p_adjust)[0])
    assert np.all(got["q"] >= got["p"])
    # device columns and files on request
    dev = ea.generateAdjustedDmrReport(a, b, as_device=True, **kw, max_q=max_q, p_adjust=p_adjust, **region_kw)
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in dev.values()) and dev.ncommon == got.ncommon
    for k in got:
        assert np.array_equal(dev[k].cpu().numpy(), got[k], equal_nan=True)
    path = str(tmp_path / "dmr_q.tsv")
    assert ea.generateAdjustedDmrReport(a, b, report_file=path, **kw, max_q=max_q, p_adjust=p_adjust, **region_kw) is None
    head, rows = _read_tsv(path)
    assert head == list(got) and len(rows) == got.nrow
    for j, k in enumerate(head):
        col = [r[j] for r in rows]
        if k in X.DMR_FLOAT + ("q",):
            np.testing.assert_allclose(np.asarray([float(v) if v else np.nan for v in col]), got[k], rtol=1e-14, atol=0, equal_nan=True)
        elif k == "rname":
            assert col == [LEVELS[v - 1] for v in got[k].tolist()]
        else:
            assert col == [str(v) for v in got[k].tolist()]
    # no adjustment, the same limit: generateDmrReport
    plain = ea.generateDmrReport(a, b, **kw, max_p=0.05, **region_kw)
    none = ea.generateAdjustedDmrReport(a, b, **kw, max_q=0.05, p_adjust="none", **region_kw)
    assert list(none)[:10] == list(plain) and none.nrow == plain.nrow and none.ncommon == plain.ncommon
    for k in plain:
        assert np.array_equal(none[k], plain[k], equal_nan=True) and none[k].dtype == plain[k].dtype, k
    np.testing.assert_array_equal(none["q"], none["p"])
    # nothing was left behind on either batch
    for x, cx in zip((a, b), before):
        H.assert_reports_equal(ea.generateCytosineReport(x, threshold_reads=False), cx)
