"""generateFdrpReport on the batches of test_gpu_fuzz_reports.py (the fuzz generator's and the deliberate ones: garbage
bytes, rows of length 0, strand codes outside 1 / 2, positions up to 2^31 - 1, piles under which the CX report runs its
general kernel, contexts mixed at one position, rows of 4000 bytes) against the loop restatement (fdrp_np.restate_indexed;
test_fdrp_host.py shows it equal to fdrp_np.restate), all ten columns bit for bit.  The batch of a seed is
test_gpu_fuzz_reports.plan(seed)["t"], untouched; FDRP's arguments come from a generator of their own, so that no draw of
that module moves.  Context and row filter lean the way test_gpu_fuzz_reports.draw_het leans (they read the input bytes
only), min_overlap leans towards small values: most calls then compare tables with discordant pairs and not two empty
ones.  On the deliberate batches the arguments are fixed; they hold both ends of flank_sites and max_reads.  What the seed
list reaches is checked without a GPU in test_fdrp_host.py.  A failure names its seed, kind and row count."""
import time

import numpy as np
import pytest

import fdrp_np
import test_gpu_fdrp as TF
import test_gpu_fuzz_reports as R

pytestmark = pytest.mark.gpu

SEEDS = R.SEEDS
MAX_DISTANCE = (0, 3, 10, 40)
# What a call costs the restatement, in pairs of rows compared: per site C(min(coverage, max_reads), 2) pairs -- the coverage
# from the site table's meth + unmeth, an upper bound that needs no restatement -- plus 32 for the site's own bookkeeping.
# A call above COST_CAP is skipped.  Measured on one CPU core the restatement takes about 0.6 us per unit: 3.5 s for the
# 8.5e6 of seed 1024, 2.8 s for the 117 000 shallow sites (4.5e6) of seed 1032, 11.9 s for the 1.6e7 of seed 1021 (9655 sites
# under a pile of 662 rows at max_reads = 58), the one call of the list that is skipped.  The plain product sites x rows does
# not follow the time: 3.1e8 (seed 1031, the largest) takes 3.5 s, the 2.9e7 of seed 1021 four times as long.
COST_CAP = 10_000_000
# (context, flank_sites, max_reads, min_overlap, max_distance, max_ooctx_meth_frac, min_reads)
FIXED = {"top": [("CG", 31, 64, 1, 0, 1.0, 2), ("CG", 0, 2, 1, 3, 1.0, 0)],
         "below_top": [("CG", 8, 40, 2, 40, 1.0, 3), ("CG", 31, 2, 5, 0, 1.0, 2)],
         "pile": [("CG", 8, 64, 1, 0, 1.0, 2)],
         "deep_pile": [("CG", 0, 64, 1, 0, 1.0, 5), ("CX", 31, 40, 3, 10, 1.0, 2)]}


def draw_fdrp(rng, t):
    name, _, mo, _, _ = R.draw_het(rng, t)
    W = int(rng.integers(0, 32))
    min_overlap = 1 if rng.random() < 0.5 else int(rng.integers(1, min(2 * W + 1, 6) + 1))
    return (name, W, int(rng.integers(2, 65)), min_overlap, int(rng.choice(MAX_DISTANCE)), mo, int(rng.integers(0, 6)))


def plan(seed):
    """(kind, the seed's batch, its FDRP calls)"""
    p = R.plan(seed)
    rng = np.random.default_rng([seed, 2])
    return p["kind"], p["t"], FIXED.get(p["kind"]) or [draw_fdrp(rng, p["t"])]


def cost(t, call):
    s = fdrp_np.site_table(t, call[0])
    c = np.minimum(s["meth"].astype(np.int64) + s["unmeth"], call[2])
    return int((c * (c - 1) // 2).sum()) + 32 * int(c.size)


def fdrp_want(t, call):
    """The restatement's table, or None where the call's cost passes COST_CAP"""
    if cost(t, call) > COST_CAP:
        return None
    ctx, W, m, min_overlap, max_distance, max_oo, min_reads = call
    return fdrp_np.restate_indexed(t, ctx, W, m, min_overlap, max_distance, max_oo, min_reads)


# Groups of at most about five seconds, set from the seeds' measured times (the restatement is most of it; seed 1021 costs its
# plan alone).  The per-seed times that the test prints are there for the next regrouping.
SEED_GROUPS = ([1024], [1031], [1020, 1032], [1000, 1039, 9002], [1015, 1016, 1018, 1049], [1014, 1037, 1047, 1050, 1052],
               [1003, 1005, 1006, 1013, 1019, 1038, 9001],
               [1002, 1008, 1022, 1023, 1028, 1029, 1030, 1033, 1034, 1036, 1046, 1051, 1054, 9003, 9005],
               [1004, 1007, 1009, 1010, 1011, 1012, 1021, 1025, 1026, 1027, 1035, 1040, 1042, 1043, 1044, 1045, 1048, 1053, 9004])
assert sorted(s for g in SEED_GROUPS for s in g) == sorted(SEEDS)


@pytest.fixture(scope="module")
def ea():
    import epialleler_amd
    return epialleler_amd


def run_seed(ea, seed):
    """-> (calls skipped for size, calls)"""
    kind, t, calls = plan(seed)
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"])
    skipped = 0
    try:
        for call in calls:
            want = fdrp_want(t, call)
            if want is None:
                skipped += 1
                continue
            ctx, W, m, min_overlap, max_distance, max_oo, min_reads = call
            got = TF.gpu_report(ea, bam, ctx, W=W, m=m, min_overlap=min_overlap, max_distance=max_distance, max_oo=max_oo, min_reads=min_reads)
            TF.assert_same(got, want, ("fdrp",) + tuple(call))
    except AssertionError as e:
        raise AssertionError("seed %d (kind %s, %d rows): %s" % (seed, kind, t["start"].size, e)) from e
    finally:
        bam.close()
    return skipped, len(calls)


def timed(ea, seed):
    t0 = time.perf_counter()
    out = run_seed(ea, seed)
    print("seed %d: %.2f s" % (seed, time.perf_counter() - t0))
    return out


@pytest.mark.parametrize("group", range(len(SEED_GROUPS)))
def test_fuzz_fdrp_seeds(ea, group):
    ran = [timed(ea, seed) for seed in SEED_GROUPS[group]]
    print("group %d: %d seeds, %d of %d calls skipped for size" % (group, len(ran), sum(r[0] for r in ran), sum(r[1] for r in ran)))
