"""epi_dist_tail, the host side of the distribution tails (csrc/dist_math.hpp): against 50-digit arithmetic on the grid and the
random points the GPU test shares (tests/cx_groups_np.py, dist_points), the domain's edges, every out-of-domain input, the
identities that make one incomplete beta function serve Student's t and F(1, df), and scipy.  No device is needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cx_groups_np as G
from epialleler_amd import _lib


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def test_host_against_50_digit_arithmetic(lib):
    """Measured on the CPU: largest relative error 6.4e-13 (EPI_DIST_T2 at t = 2, df = 1e4: the direct continued fraction
    just below the swap); EPI_DIST_CHISQ 1.1e-13 at p = 3.7e-249, EPI_DIST_F1 5.2e-13 at F = 3.84, df = 1e4.  Nothing on
    the grid is above 1e-12.  The bound is 8 times the measured figure."""
    kind, x, df = G.dist_points()
    assert kind.size == 3 * (len(G.GRID_X) * len(G.GRID_DF) + 200)
    got = np.concatenate([G.host_dist_tail(k, x[kind == k], df[kind == k]) for k in (G.CHISQ, G.T2, G.F1)])
    assert not np.isnan(got).any() and np.all((got >= 0) & (got <= 1))
    rel, tiny_ok = G.dist_errors(got, G.dist_exact(kind, x, df))
    assert tiny_ok
    compared = ~np.isnan(rel)
    assert compared.sum() > 900 and (~compared).sum() > 10            # both sides of 1e-300 are exercised
    for k in (G.CHISQ, G.T2, G.F1):
        m = compared & (kind == k)
        i = np.flatnonzero(m)[np.argmax(rel[m])]
        print("  kind %d: largest relative error %.3e at x = %g, df = %g, p = %.3e" % (k, rel[i], x[i], df[i], got[i]))
    assert np.nanmax(rel) <= 1e-12                                    # (the issue's line between a figure and a finding)
    assert np.nanmax(rel) <= G.DIST_HOST_RTOL, np.nanmax(rel)


def test_edges_and_out_of_domain(lib):
    inf, nan = float("inf"), float("nan")
    for k in (G.CHISQ, G.T2, G.F1):
        assert G.host_dist_tail(k, [0.0, 0.0, 0.0, inf, inf], [1.0, 0.3, 1e4, 1.0, 1e4]).tolist() == [1.0, 1.0, 1.0, 0.0, 0.0]
        bad_df = G.host_dist_tail(k, [1.0] * 6, [0.0, -1.0, 1e4 + 1, inf, -inf, nan])
        assert np.isnan(bad_df).all()
        assert np.isnan(G.host_dist_tail(k, [nan], [3.0])).all()
        assert not np.isnan(G.host_dist_tail(k, [1.0, 1.0], [1e4, 1e-3])).any()
    for k in (G.CHISQ, G.F1):
        assert np.isnan(G.host_dist_tail(k, [-1.0, -1e-300, -inf], [3.0])).all()
    # a t statistic has a sign: the tail is two-sided
    assert G.host_dist_tail(G.T2, [-2.5, -inf], [7.0]).tolist() == [G.host_dist_tail(G.T2, [2.5], [7.0])[0], 0.0]
    # huge finite arguments: no overflow on the way, 0 or a tiny tail
    assert G.host_dist_tail(G.CHISQ, [1e300], [5.0])[0] == 0.0 and G.host_dist_tail(G.F1, [1e308], [1e4])[0] == 0.0
    assert 0 < G.host_dist_tail(G.F1, [1.7e308], [1.0])[0] < 1e-150       # Cauchy tails are fat: 2 / (pi sqrt(F))


def test_bad_arguments_of_the_library(lib):
    p = np.zeros(1)
    ptr = C.c_void_p(p.ctypes.data)
    assert lib.epi_dist_tail(3, ptr, ptr, 1, ptr) == _lib.EPI_ERR_ARG and b"kind" in lib.epi_last_error()
    assert lib.epi_dist_tail(-1, ptr, ptr, 1, ptr) == _lib.EPI_ERR_ARG
    assert lib.epi_dist_tail(0, None, ptr, 1, ptr) == _lib.EPI_ERR_ARG
    assert lib.epi_dist_tail(0, ptr, ptr, -1, ptr) == _lib.EPI_ERR_ARG
    assert lib.epi_dist_tail(0, None, None, 0, None) == _lib.EPI_OK
    assert lib.epi_dist_tail_dev(None, 0, None, None, 0, None, None) == _lib.EPI_ERR_ARG


def test_identities_and_scipy(lib):
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(3)
    x = np.exp(rng.uniform(np.log(1e-3), np.log(300), 400))
    df = np.exp(rng.uniform(np.log(0.5), np.log(1e4), 400))
    for got, want in ((G.host_dist_tail(G.CHISQ, x, df), stats.chi2.sf(x, df)), (G.host_dist_tail(G.T2, np.sqrt(x), df), 2 * stats.t.sf(np.sqrt(x), df)),
                      (G.host_dist_tail(G.F1, x, df), stats.f.sf(x, 1, df))):
        ok = want > 1e-290
        assert ok.sum() > 300 and np.max(np.abs(got[ok] - want[ok]) / want[ok]) < 1e-9       # (scipy is the looser side)
    # t^2 is F(1, df): the same function of the same argument, bit for bit
    t = np.sqrt(x)
    assert np.array_equal(G.host_dist_tail(G.T2, t, df), G.host_dist_tail(G.F1, t * t, df))
    # df = 1 and df = 2 in closed form
    assert G.host_dist_tail(G.CHISQ, [3.84], [2.0])[0] == pytest.approx(np.exp(-1.92), rel=1e-14)
    assert G.host_dist_tail(G.T2, [1.0], [1.0])[0] == pytest.approx(0.5, rel=1e-14)


def test_one_copy_of_the_arithmetic():
    """dist.cpp and cx_groups.hip both take the tails from dist_math.hpp; every loop there has a written bound."""
    src = {}
    for name in ("dist.cpp", "cx_groups.hip", "dist_math.hpp"):
        with open(os.path.join(_lib.CSRC, name)) as f:
            src[name] = f.read()
    for fn in ("chisq_upper", "beta_tail", "beta_cf", "pois_term", "tail_of"):
        assert len(re.findall(r"double %s\(" % fn, src["dist_math.hpp"])) == 1
        assert not re.search(r"double %s\(" % fn, src["dist.cpp"] + src["cx_groups.hip"])
    for name in ("dist.cpp", "cx_groups.hip"):
        assert '#include "dist_math.hpp"' in src[name]
    code = re.sub(r"//.*|#define.*", "", src["dist_math.hpp"])
    assert "while" not in code
    loops = re.findall(r"for \(int \w+ = 1; \w+ <= (\w+); \w+\+\+\)", code)
    assert sorted(loops) == ["kBetaCfMax", "kGammaCfMax", "kSeriesMax"]
    assert code.count("for (") == 4 and "for (int k = 0; k < kBetaShift; k++)" in code            # (the fourth has no exit but its bound)
    with open(os.path.join(_lib.CSRC, "Makefile")) as f:
        mk = f.read()
    assert re.search(r"^HOST_SRCS := .*\bdist\.cpp\b", mk, flags=re.M) and re.search(r"^SRCS := .*\bcx_groups\.hip\b", mk, flags=re.M)
    assert re.search(r"^fisher\.o dist\.o: HOST_FPFLAGS := -fno-fast-math -ffp-contract=off$", mk, flags=re.M)
