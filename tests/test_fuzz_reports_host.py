"""What the seeds of test_gpu_fuzz_reports.py reach, from the restatements and the CPU oracle alone: a fuzz that compares
empty tables proves nothing.  Runs without a GPU."""
import numpy as np

import test_gpu_fuzz_reports as R
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
