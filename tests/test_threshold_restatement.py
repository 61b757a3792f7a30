"""The plain numpy restatements of the per-read decisions (helpers.threshold_np, helpers.mhl_keep_np) against the CPU oracle,
on random data and on the tie batch at every threshold of the grid.  The GPU tests compare the kernels with both, so a
mistake shared by the oracle and the kernels still shows."""
import numpy as np
import pytest

import helpers as H
import synth_np
from oracle import oracle as orc

NAN2 = float(np.uint64(0x7FF8000000000123).view(np.float64))      # a NaN with another payload


def batches():
    rng = np.random.default_rng(101)
    yield H.tie_batch()
    yield synth_np.random_templates(rng, 3000, 0, 300, 3, 20000)
    yield synth_np.random_templates(rng, 500, 0, 200, 2, 800, p_garbage=0.3)
    yield H.templates_from_xm([], [], [])


@pytest.mark.parametrize("ctx", ["CG", "CHG", "CHH", "CxG", "CX"])
def test_threshold_np_matches_oracle(ctx):
    grid = H.THRESHOLD_GRID + ((2, 0.5, 0.1), (2, NAN2, 0.1), (0, 0.0, 0.0), (2, np.nextafter(0.3, 1), np.nextafter(0.1, 0)))
    for t in batches():
        for mn, mb, mo in grid:
            want = orc.threshold_reads(t["xm"], t["off"], *H.cls4(ctx), mn, mb, mo)
            got = H.threshold_np(t["xm"], t["off"], H.cls4(ctx), mn, mb, mo)
            assert np.array_equal(got, want), (ctx, mn, mb, mo)
    # repeated letters count twice; empty out-of-context classes
    t = next(batches())
    for c4 in (("ZZ", "z", "XH", "xh"), ("Zz", "zZ", "", ""), ("Z", "z", "ZX", "x")):
        assert np.array_equal(H.threshold_np(t["xm"], t["off"], c4, 3, 0.4, 0.3), orc.threshold_reads(t["xm"], t["off"], *c4, 3, 0.4, 0.3))


def test_tie_batch_has_ties():
    """The tie rows flip when a threshold moves by one ulp: the batch exercises what the GPU tests need it for."""
    t = H.tie_batch()
    f = lambda mn, mb, mo: H.threshold_np(t["xm"], t["off"], H.cls4("CG"), mn, mb, mo)
    base = f(2, 0.3, 0.1)
    assert base.sum() > 0
    assert not np.array_equal(base, f(2, np.nextafter(0.3, 1), 0.1))
    assert not np.array_equal(base, f(2, 0.3, np.nextafter(0.1, 0)))
    assert not np.array_equal(base, f(3, 0.3, 0.1))
    assert np.array_equal(f(2, float("nan"), 0.1), f(2, NAN2, 0.1))


@pytest.mark.parametrize("ctx", ["Zz", "Xx", "ZzXx", "Hh"])
def test_mhl_keep_np_matches_oracle(ctx):
    """The oracle's lMHL report with its read filter equals its report, unfiltered, of the reads mhl_keep_np keeps."""
    for t in batches():
        if t["start"].size == 0:
            continue
        for hmin, moo in ((0, 0.1), (0, 0.0), (0, float("nan")), (0, -0.5), (10, 0.1), (3, 1.0)):
            keep = H.mhl_keep_np(t["xm"], t["off"], ctx, hmin, moo)
            want = orc.mhl_report(t["xm"], t["off"], t["rname"], t["strand"], t["start"], ctx, 0, hmin, moo)
            s = H.subset(t, keep)
            got = orc.mhl_report(s["xm"], s["off"], s["rname"], s["strand"], s["start"], ctx, 0, 0, float("nan"))
            H.assert_reports_equal(got, want, float_cols=("length", "lmhl"))
