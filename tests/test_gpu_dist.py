"""epi_dist_tail_dev, chisqPValues and tTestPValues on the GPU: the device kernel against the host function, which shares
its arithmetic (csrc/dist_math.hpp) and which test_dist_host.py holds against 50-digit arithmetic, on that test's grid
and random points; the domain's edges; the Python entry points' conventions; and the p-value that compareHeterogeneity's g
and df were missing."""
import numpy as np
import pytest

import cx_groups_np as G
import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ea():
    import epialleler_amd
    return epialleler_amd


def dev_tail(ea, kind, x, df):
    import ctypes as C
    import torch
    from epialleler_amd import _lib, api
    x, df = [torch.from_numpy(np.ascontiguousarray(v, np.float64)).cuda() for v in (x, np.broadcast_to(np.asarray(df, np.float64), np.shape(x)))]
    p = torch.full_like(x, -7.0)
    _lib.check(_lib.load().epi_dist_tail_dev(api._engine(0), kind, C.c_void_p(x.data_ptr()), C.c_void_p(df.data_ptr()), x.numel(),
                                             C.c_void_p(p.data_ptr()), api._stream(0)))
    torch.cuda.synchronize()
    return p.cpu().numpy()


def test_device_against_the_host_on_the_grid(ea):
    """Measured on an MI355X: the figures this prints; cx_groups_np.DEV_HOST_MEASURED is the largest of them and of
    test_gpu_cx_groups.py's.  The bound is 8 times it."""
    kind, x, df = G.dist_points()
    worst = 0.0
    for k in (G.CHISQ, G.T2, G.F1):
        m = kind == k
        got, want = dev_tail(ea, k, x[m], df[m]), G.host_dist_tail(k, x[m], df[m])
        assert np.all((got >= 0) & (got <= 1))
        rel = G.rel_diff(got, want)
        print("  kind %d: largest device-host relative difference %.3e" % (k, rel))
        worst = max(worst, rel)
    assert worst <= G.DEV_HOST_RTOL, worst


def test_edges_and_out_of_domain_on_the_device(ea):
    inf, nan = float("inf"), float("nan")
    x = [0.0, 0.0, inf, inf, 1.0, 1.0, 1.0, 1.0, 1.0, nan, 1e300, 1.0, 1.0]
    df = [1.0, 1e4, 1.0, 1e4, 0.0, -1.0, 1e4 + 1, inf, nan, 3.0, 5.0, 1e-3, 1e4]
    for k in (G.CHISQ, G.T2, G.F1):
        got, want = dev_tail(ea, k, x, df), G.host_dist_tail(k, x, df)
        assert got[:4].tolist() == [1.0, 1.0, 0.0, 0.0] and np.isnan(got[4:10]).all() and not np.isnan(got[10:]).any()
        assert np.array_equal(np.isnan(got), np.isnan(want)) and G.rel_diff(got, want) <= G.DEV_HOST_RTOL
    for k in (G.CHISQ, G.F1):
        assert np.isnan(dev_tail(ea, k, [-1.0, -inf], [3.0])).all()
    t = dev_tail(ea, G.T2, [-2.5, 2.5, -inf], [7.0])
    assert t[0] == t[1] and t[2] == 0.0
    assert dev_tail(ea, G.CHISQ, np.zeros(0), np.zeros(0)).size == 0


def test_python_entry_points(ea):
    import torch
    stat, df = np.asarray([0.0, 3.84, 10.0, 50.0]), np.asarray([1.0, 1.0, 4.0, 30.0])
    want = G.host_dist_tail(G.CHISQ, stat, df)
    got = ea.chisqPValues(stat, df)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and G.rel_diff(got, want) <= G.DEV_HOST_RTOL and got[0] == 1.0
    # one df for all; integers; lists; device tensors in, device tensor out
    assert np.array_equal(ea.chisqPValues([1, 2, 3], 2), dev_tail(ea, G.CHISQ, [1.0, 2.0, 3.0], 2.0))
    d = ea.chisqPValues(torch.from_numpy(stat).cuda(), torch.from_numpy(df.astype(np.int32)).cuda(), as_device=True)
    assert isinstance(d, torch.Tensor) and d.is_cuda and d.dtype == torch.float64 and np.array_equal(d.cpu().numpy(), got)
    t = np.asarray([-3.0, 0.0, 2.0, 2.0])
    tp = ea.tTestPValues(t, [5.0, 5.0, 10.0, 1e4])
    assert G.rel_diff(tp, G.host_dist_tail(G.T2, t, [5.0, 5.0, 10.0, 1e4])) <= G.DEV_HOST_RTOL and tp[1] == 1.0
    assert tp[2] == pytest.approx(0.0733880347707404, rel=1e-12)          # 2 * pt(-2, 10)
    assert ea.chisqPValues([], 3).size == 0 and np.isnan(ea.chisqPValues([-1.0, 1.0], [2.0, 0.0])).all()


def test_p_value_of_compare_heterogeneity(ea):
    """chisqPValues(g, df) on a compareHeterogeneity table: equal to the host function on the fetched columns, and the
    table itself is what it was (compareHeterogeneity is unchanged)."""
    import os
    a, b = [ea.preprocessBam(os.path.join(H.GOLDEN, "bam", n)) for n in ("amplicon010meth.bam", "amplicon100meth.bam")]
    rep = ea.compareHeterogeneity(a, b, window_sites=3, as_device=True)
    assert rep.nrow > 10 and "p" not in rep
    p = ea.chisqPValues(rep["g"], rep["df"])
    g, df = rep["g"].cpu().numpy(), rep["df"].cpu().numpy()
    want = G.host_dist_tail(G.CHISQ, g, df)
    rel = G.rel_diff(p, want)
    print("  compareHeterogeneity: %d windows, largest device-host relative difference %.3e" % (g.size, rel))
    ok = df > 0                                                         # (a window with one pattern in all has df = 0: NaN)
    assert rel <= G.DEV_HOST_RTOL and ok.sum() > 10 and np.all((p[ok] >= 0) & (p[ok] <= 1)) and np.isnan(p[~ok]).all()
