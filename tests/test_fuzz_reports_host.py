"""What the seeds of test_gpu_fuzz_reports.py reach, from the restatements and the CPU oracle alone: a fuzz that compares
empty tables proves nothing.  One test for the five older reports, one for the linkage calls, their blocks and the
comparisons with the sibling: pairs with a defined r2 and beyond the adjacent ones, blocks, every D, the top of int32, deep
pairs and windows, long rows and the mean row length that switches the counting kernels, partial and empty common
tables.  Runs without a GPU."""
import numpy as np

import test_gpu_fuzz_reports as R
import test_gpu_heterogeneity_compare as HC
import test_gpu_sequences as SQ

TOP = 2 ** 31 - 1


def test_fuzz_report_inputs_cover_the_shapes():
    calls = skipped = multi = deep = high = long_row = three = both = 0
    ks, npat, repeated, halves = set(), 0, 0, 0
    for seed in R.SEEDS:
        p = R.plan(seed)
        t = p["t"]
        if p["kind"] == "pile":
            assert SQ.deep(t) and np.unique(t["rname"]).size == 3
        if p["kind"] == "top":
            assert int((t["start"].astype(np.int64) + np.diff(t["off"])).max()) == TOP
        for call in p["het"]:
            calls += 1
            ks.add(call[1])
            want = R.het_want(t, call)
            if want is None:
                skipped += 1
                continue
            nwin = want["pos"].size
            multi += bool(np.any(want["npatterns"] > 1))
            deep += bool(nwin and want["nreads"].max() >= 256)
            high += bool(nwin and want["pos"].max() > TOP - 1000)
            long_row += bool(np.diff(t["off"]).max() > 4000)
            three += np.unique(t["rname"]).size >= 3
            both += set(np.unique(want["sites"]["strand"]).tolist()) >= {1, 2}
        want = R.freqs_want(t, p["freqs"])[2]
        halves += bool(want[:, :10].sum() > 0 and want[:, 10:].sum() > 0)
        for tab, summ in R.pattern_wants(t, p["patterns"]):
            npat += len(tab["pattern"])
            repeated += bool(summ is not None and summ["count"].max() > 1)
    print("heterogeneity calls %d: %d with several patterns in a window, %d with a window of 256 reads or more, %d with a site above "
          "2^31 - 1000, %d on a batch with a row above 4000 bytes, %d on three sequences or more, %d with sites on both strands, "
          "%d skipped for size, k drawn %s; %d patterns, %d summaries with a count above 1, %d of %d base-frequency batches with "
          "counts in both halves" % (calls, multi, deep, high, long_row, three, both, skipped, sorted(ks), npat, repeated, halves,
                                     len(R.SEEDS)))
    assert 3 * multi >= 2 * calls
    assert deep >= 2 and high >= 2 and long_row >= 1 and three >= 1 and both >= 1   # (two calls of a deliberate batch each: losing one shows)
    assert ks == {2, 3, 4, 5, 6}
    assert 20 * skipped <= calls
    assert npat > 2000
    assert repeated >= 10
    assert 4 * halves >= len(R.SEEDS)                       # two of the five kinds of pass vector always give both (expected: 2 in 5)


def test_fuzz_linkage_and_compare_inputs_cover_the_shapes():
    """The linkage calls, their block calls and the comparisons with the sibling, as the seeds' tests run them."""
    lk = dict.fromkeys(("calls", "skipped", "r2", "far", "far_asked", "both", "blocks", "high", "deep", "long_row", "wide", "three_both"), 0)
    cm = dict.fromkeys(("calls", "skipped", "exercise", "partial", "high", "deep", "none_common"), 0)
    Ds = set()
    for seed in R.SEEDS:
        p = R.plan(seed)
        t = p["t"]
        L = np.diff(t["off"])
        for call, bcall in p["link"]:
            lk["calls"] += 1
            Ds.add(call[1])
            want = R.link_want(t, call)
            if want is None:
                lk["skipped"] += 1
                continue
            npair = want["pos"].size
            lk["r2"] += bool(np.any(~np.isnan(want["r2"])))
            lk["far_asked"] += call[1] > 1
            lk["far"] += bool(call[1] > 1 and np.any(want["neighbour"] > 1))
            lk["both"] += bool(np.any(~np.isnan(want["r2"])) and (call[1] == 1 or np.any(want["neighbour"] > 1)))
            lk["blocks"] += R.blocks_want(want, bcall)["start"].size > 0
            lk["high"] += bool(npair and want["pos2"].max() > TOP - 1000)
            lk["deep"] += bool(npair and want["nreads"].max() >= 256)
            lk["long_row"] += bool(L.max() > 4000)
            lk["wide"] += bool(int(t["off"][-1]) > 512 * L.size)          # site_count_blocks: a whole wave takes a row
            lk["three_both"] += bool(np.unique(t["rname"]).size >= 3 and set(np.unique(want["sites"]["strand"]).tolist()) >= {1, 2})
        ta, tb = t, p["sibling"]
        for call in p["cmp"]:
            for x, y in ((ta, tb), (tb, ta)):
                cm["calls"] += 1
                want = R.cmp_want(x, y, call)
                if want is None:
                    cm["skipped"] += 1
                    continue
                nwin = want["pos"].size
                cm["exercise"] += HC.exercises(want)
                cm["partial"] += 0 < want["ncommon"] < min(want["sites_a"]["pos"].size, want["sites_b"]["pos"].size)
                cm["high"] += bool(nwin and want["end"].max() > TOP - 1000)
                cm["deep"] += bool(nwin and max(want["nreads_a"].max(), want["nreads_b"].max()) >= 256)
                cm["none_common"] += want["ncommon"] == 0
    print("linkage calls %(calls)d: %(r2)d with a defined r2, %(far)d of %(far_asked)d with D > 1 have a pair beyond the adjacent ones (%(both)d calls with both), "
          "%(blocks)d with a block, %(high)d with pos2 above 2^31 - 1000, %(deep)d with a pair of 256 reads or more, %(long_row)d on a "
          "batch with a row above 4000 bytes, %(wide)d on a batch with a mean row above 512 bytes, %(three_both)d on three sequences with "
          "sites on both strands, %(skipped)d skipped for size" % lk, "D drawn %s" % sorted(Ds))
    print("comparisons %(calls)d (both orders): %(exercise)d exercise, %(partial)d with a partial common table, %(high)d with a window end "
          "above 2^31 - 1000, %(deep)d with a window of 256 reads or more, %(none_common)d without a common site, %(skipped)d skipped "
          "for size" % cm)
    assert 20 * lk["skipped"] <= lk["calls"]
    assert 3 * lk["both"] >= 2 * lk["calls"]                    # a defined r2 and, where D > 1, a pair beyond the adjacent ones
    assert 2 * lk["blocks"] >= lk["calls"]
    assert Ds == set(R.LINK_D)
    assert lk["high"] >= 2 and lk["deep"] >= 1 and lk["long_row"] >= 1 and lk["wide"] >= 1 and lk["three_both"] >= 1
    assert 20 * cm["skipped"] <= cm["calls"]
    assert 2 * cm["exercise"] >= cm["calls"]
    assert 4 * cm["partial"] >= 3 * cm["calls"]
    assert cm["high"] >= 2 and cm["deep"] >= 1 and cm["none_common"] >= 1
