"""The smoother and the segmentation at the seams of the step they share into series order (cx_series.hpp): tables of 1 and 2 rows,
of a workgroup's 256 threads, the segmentation's workgroup range of 2048 sites and the scan's and the sort's 4096-row block, each
with a row less and a row more, and 8193 rows.  A table holds two (strand, context) classes on one rname, interleaved row by row -- the later
class first in series order, so the stable pass moves every row -- with sites 1 to 40 apart inside a class and one gap above
max_gap in each.  Nothing new is asserted: the comparisons are test_gpu_smooth.py's and test_gpu_segment.py's own, exact against
tests/smooth_np.py and tests/segment_np.py."""
import numpy as np
import pytest

import segment_np as G
import smooth_np as S
from test_gpu_segment import check_segment
from test_gpu_smooth import check_smooth, ea  # noqa: F401  (ea: the module fixture)

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 8193)
MAX_GAP = 300


def interleaved(n):
    """n rows: even rows are '-' CG, odd rows '+' CHH (the class that comes first in series order)"""
    rng = np.random.default_rng(1000 + n)
    gaps = rng.integers(1, 21, n)                                   # two of them between the neighbours of a class: 2 to 40
    if n >= 2:
        gaps[n // 2] = MAX_GAP + 1                                  # between a row of each class: one cut in both
    pos = np.cumsum(gaps)
    cov = rng.integers(0, 9, n)
    meth = rng.binomial(cov, np.where((np.arange(n) // 75) % 2 == 0, 0.15, 0.85))
    even, odd = slice(0, n, 2), slice(1, n, 2)
    t = S.series_table([(1, 2, S.CG, pos[even], meth[even], (cov - meth)[even]), (1, 1, S.CHH, pos[odd], meth[odd], (cov - meth)[odd])])
    assert t["pos"].size == n and (n < 2 or t["strand"][:2].tolist() == [2, 1])
    return t


@pytest.mark.parametrize("n", SIZES)
def test_smooth(ea, n):  # noqa: F811
    got = check_smooth(ea, interleaved(n), n, bandwidth=50, min_sites=5, max_gap=MAX_GAP, degree=1)
    assert got.ncluster == (4 if n >= 4 else n)


@pytest.mark.parametrize("n", SIZES)
def test_segment(ea, n):  # noqa: F811
    t = interleaved(n)
    for K in (2, 3, 4):
        got = check_segment(ea, t, G.start_model((0.1, 0.5, 0.9, 0.7)[:K], 0.9), (n, K), max_gap=MAX_GAP, max_iter=2)
        assert got.nchain == (4 if n >= 4 else n)
