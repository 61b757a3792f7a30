"""A fixed set of randomized batches over many shapes -- short ragged rows, pile-ups, long reads, rows around the lane-width
and single-block limits, positions near tile multiples and 2^31, the benchmark's two generators, tails of long templates --
each through thresholding (per-read and fused), beta, CX and lMHL against the CPU oracle, with thresholds drawn from a grid
that includes ties, NaN and the extremes.  Bounded by a list of seeds, not by time; a failure names its seed."""
import numpy as np
import pytest

import helpers as H
import synth_np
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ALPHABETS = [None, "......hhxzzZZZHXuU-", "zZ", "zZ.", "zzzzZ....", "ZZZZZZZZz.", "hHxXzZuU.+-", "....-----zZ", "..zZZzxX"]
MN = (0, 1, 2, 3, 5)
MB = (0.0, 0.3, 1 / 3, 0.5, 0.9, 1.0, float("nan"))
MO = (0.0, 0.1, 1.0, float("nan"))
SEEDS = list(range(1000, 1150))
GROUPS = 10


@pytest.fixture(scope="module")
def ea():
    import epialleler_amd
    return epialleler_amd


def make_batch(rng, seed):
    alpha = lambda: ALPHABETS[int(rng.integers(0, len(ALPHABETS)))]
    kind = int(rng.integers(0, 6))
    if kind == 0:      # short ragged
        t = synth_np.random_templates(rng, int(rng.integers(1, 4000)), 0, int(rng.integers(1, 700)), int(rng.integers(1, 6)),
                                      int(rng.integers(10, 20000)), p_garbage=float(rng.choice([0, 0, 0.05, 0.3])), alphabet=alpha())
    elif kind == 1:    # pile-up
        t = synth_np.random_templates(rng, int(rng.integers(100, 8000)), 20, int(rng.integers(40, 500)), int(rng.integers(1, 3)),
                                      int(rng.integers(2, 300)), alphabet=alpha())
    elif kind == 2:    # long reads (multi-block lMHL pass 1, slice-by-slice CX rows)
        t = synth_np.random_templates(rng, int(rng.integers(1, 120)), int(rng.integers(0, 3000)), int(rng.integers(3000, 20000)),
                                      int(rng.integers(1, 4)), int(rng.integers(100, 60000)), alphabet=alpha())
    elif kind == 3:    # medium reads around the single-block limit of the lMHL row kernel (2 KiB) and lane-width switches
        top = int(rng.choice([200, 240, 250, 370, 380, 500, 760, 1000, 1010, 2030, 2040, 2050, 3000]))
        t = synth_np.random_templates(rng, int(rng.integers(1, 1500)), max(top - 40, 0), top, int(rng.integers(1, 4)),
                                      int(rng.integers(100, 30000)), alphabet=alpha())
    elif kind == 4:    # positions near tile multiples and large coordinates
        t = synth_np.random_templates(rng, int(rng.integers(1, 2000)), 1, int(rng.integers(2, 400)), int(rng.integers(1, 3)), 3000)
        base = int(rng.choice([1, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 10 ** 6, 2 ** 31 - 4000]))
        t["start"] = (t["start"].astype(np.int64) + base - 1).astype(np.int32)
    elif seed % 2:     # ragged, gapped templates at uniform-random starts (the benchmark's cfg2u model), small
        t = synth_np.generate_uniform(seed=seed, n_total=int(rng.integers(1000, 15000)))
    else:              # the benchmark generator's model, small
        L = int(rng.choice([100, 300, 301, 2000]))
        t = synth_np.generate(seed=seed, n_total=int(rng.integers(1000, 15000 if L < 2000 else 3000)), read_len=L)
    if kind in (0, 1, 3, 5) and rng.random() < 0.4 and t["off"].size > 2:      # a tail of long templates
        every = int(rng.choice([3, 17, 97, 501, 4001]))
        t = synth_np.with_long_tail(t, every, int(rng.choice([330, 400, 650, 1000, 1100, 2500, 4000, 9000])), first=int(rng.integers(0, every)))
    return kind, t


def run_seed(ea, seed):
    rng = np.random.default_rng(seed)
    kind, t = make_batch(rng, seed)
    n = t["off"].size - 1
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"])
    try:
        ctxn = str(rng.choice(["CG", "CHG", "CHH", "CxG", "CX"]))
        c4 = H.cls4(ctxn)
        mn, mb, mo = int(rng.choice(MN)), float(rng.choice(MB)), float(rng.choice(MO))
        want = orc.threshold_reads(t["xm"], t["off"], *c4, mn, mb, mo)
        assert np.array_equal(H.threshold_np(t["xm"], t["off"], c4, mn, mb, mo), want), "oracle vs restatement"
        got = ea.rcpp_threshold_reads(bam, *c4, mn, mb, mo)
        assert np.array_equal(got.astype(np.int32), want), ("threshold", ctxn, mn, mb, mo)
        gb = ea.rcpp_get_xm_beta(bam, c4[0], c4[1])
        assert np.array_equal(gb.view(np.uint64), orc.get_xm_beta(t["xm"], t["off"], c4[0], c4[1]).view(np.uint64)), "beta"
        p = want if rng.random() < 0.6 else None
        rctx = str(rng.choice(["Z", "X", "H", "ZX", "ZXH"]))
        H.assert_reports_equal(dict(ea.rcpp_cx_report(bam, p, rctx)),
                               orc.cx_report(t["xm"], t["off"], t["rname"], t["strand"], t["start"], p, rctx))
        if n:                                              # thresholding inside the tile kernel; the report's context is the
            rctx2 = c4[0] if rng.random() < 0.5 else str(rng.choice(["Z", "X", "H", "ZX", "ZXH"]))   # thresholding one half the time
            H.dirty_allocator(bam)
            rep2, p2 = ea.cytosine_report_fused(bam, *c4, mn, mb, mo, rctx2, return_pass=True)
            assert np.array_equal(p2.astype(np.int32), want), ("fused pass", ctxn, rctx2, mn, mb, mo)
            H.assert_reports_equal(dict(rep2), orc.cx_report(t["xm"], t["off"], t["rname"], t["strand"], t["start"], want, rctx2))
        hctx = str(rng.choice(["Zz", "Xx", "Hh", "ZzXx", "ZzXxHh"]))
        hmax, hmin = int(rng.choice([0, 0, 1, 3, 50])), int(rng.choice([0, 0, 2, 5]))
        moo = float(rng.choice([0.1, 0.0, 1.0, float("nan"), -0.5]))
        H.assert_reports_equal(dict(ea.rcpp_mhl_report(bam, hctx, hmax, hmin, moo)),
                               orc.mhl_report(t["xm"], t["off"], t["rname"], t["strand"], t["start"], hctx, hmax, hmin, moo),
                               float_cols=("length", "lmhl"))
    except AssertionError as e:
        raise AssertionError("seed %d (kind %d, %d rows): %s" % (seed, kind, n, e)) from e
    finally:
        bam.close()


@pytest.mark.parametrize("group", range(GROUPS))
def test_fuzz_seeds(ea, group):
    for seed in SEEDS[group::GROUPS]:
        run_seed(ea, seed)
