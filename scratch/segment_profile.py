"""segmentCytosineReport's kernels on a destranded genome's worth of CpGs in one process -- kernel time of every phase of one
decode from epi_prof (prof_begin / prof_end: device events around each launch), median and range of the repeats after a
warm-up, the bytes each phase reads and writes with its share of the HBM rate, and the time of a refit iteration: the driver of
profiles/segment_report.txt.
    python scratch/segment_profile.py [n_sites] [repeats]      default 28 000 000 sites, 5 repeats
The table: n_sites CpGs over 24 rnames, geometric gaps of mean 100, strand '+' (seeded; made on the device); methylation in
blocks of 400 sites that alternate between the levels 0.1 and 0.85 with every tenth block at 0.5, Poisson(8) coverage.  K = 3,
segmentCytosineReport's default model.
Before anything is timed, three windows of 3000 rows are segmented as tables of their own and compared with the restatement
(tests/segment_np.py): states, segments, fit and score; and the whole table's states and score are compared with the library's
own plain loop (epi_segment_chain_host over every chain, from epi_segment_quantise's tables).
Bytes: what a phase must move, from the shapes (BYTES below), not counters: n sites, nb = workgroups of the scans.  The share is
bytes over kernel time over 6.29 TB/s, the rate a float4 copy reaches on this part (8.0 TB/s on the data sheet)."""
import ctypes as C
import math
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import segment_np as G  # noqa: E402
import smooth_np as S  # noqa: E402
import epialleler_amd as ea  # noqa: E402

lib = ea._lib.load()
HBM_COPY_RATE = 6.29e12
N_RNAME = 24
K = 3
MODEL = G.start_model()
MAX_GAP, MAX_COVERAGE = 5000, 1000
LABELS = ("segment_sort", "segment_gather", "segment_fwd_agg", "segment_fwd_carry", "segment_fwd_walk", "segment_bwd_agg", "segment_bwd_carry",
          "segment_bwd_walk", "segment_runs", "segment_emit", "segment_counts")
# bytes a phase reads + writes: n sites, nb workgroups, g segments (each row 7 * 4 + 3 * 8 = 52 bytes)
BYTES = {
    "segment_sort": lambda n, nb, g: 24 * n + 12 * n + 8 * n + 12 * n + 12 * n,      # key: six columns in, pair out; histogram; scatter
    "segment_gather": lambda n, nb, g: (4 + 8 + 16) * n + 4 * n,                       # order, class, four columns by row; the site word
    "segment_fwd_agg": lambda n, nb, g: 4 * n + nb * (8 * K * K + 8),
    "segment_fwd_carry": lambda n, nb, g: 2 * nb * (8 * K * K + 8) + nb * 8 * K,
    "segment_fwd_walk": lambda n, nb, g: 4 * n + nb * 8 * K + n,
    "segment_bwd_agg": lambda n, nb, g: n + nb,
    "segment_bwd_carry": lambda n, nb, g: 3 * nb,
    "segment_bwd_walk": lambda n, nb, g: n + nb + n,
    "segment_runs": lambda n, nb, g: 5 * n + 4 * n + 8 * n,                            # flags out; the scan reads them and writes offsets
    "segment_emit": lambda n, nb, g: (4 + 1 + 4 + 4) * n + 4 * n + (4 + 4 + 8) * n + (52 + 20 + 20) * g,   # sites: order, state, flag, offset in, state
                                                                                      # out; sums: order, flag, the raw counts; rows: zeroed, summed, written
    "segment_counts": lambda n, nb, g: 5 * n,
}


def make_table(n, seed=42):
    g = torch.Generator(device="cuda").manual_seed(seed)
    per = (n + N_RNAME - 1) // N_RNAME
    idx = torch.arange(n, device="cuda")
    u = torch.rand(n, generator=g, device="cuda", dtype=torch.float64)
    gaps = (torch.log1p(-u) / np.log1p(-0.01)).floor().to(torch.int64) + 1          # geometric, mean 100
    rname = (idx // per).to(torch.int32) + 1
    pos = torch.cumsum(gaps, 0)
    first = idx // per * per
    pos = (pos - pos[first] + gaps[first]).to(torch.int32)                           # restart per rname
    cdf = np.cumsum([math.exp(-8.0 + k * math.log(8.0) - math.lgamma(k + 1.0)) for k in range(80)])     # Poisson(8) by inversion
    cov = torch.searchsorted(torch.from_numpy(cdf).cuda(), torch.rand(n, generator=g, device="cuda", dtype=torch.float64)).to(torch.int32)
    block = idx // 400
    level = torch.where(block % 10 == 9, 0.5, torch.where(block % 2 == 0, 0.1, 0.85)).double()
    meth = torch.zeros(n, dtype=torch.int32, device="cuda")
    for k in range(int(cov.max())):                                                  # binomial(cov, level) as a sum of Bernoulli draws
        meth += ((torch.rand(n, generator=g, device="cuda", dtype=torch.float64) < level) & (cov > k)).to(torch.int32)
    cols = dict(rname=rname, strand=torch.ones(n, dtype=torch.int32, device="cuda"), pos=pos,
                context=torch.full((n,), S.CG, dtype=torch.int32, device="cuda"), meth=meth, unmeth=cov - meth)
    return ea.Report(cols, ["chr%d" % (k + 1) for k in range(N_RNAME)])


def prof_run(fn):
    lib.epi_prof_reset(); lib.epi_prof_enable(1)
    try:
        fn()
    finally:
        lib.epi_prof_enable(0)
    out = {}
    for label in LABELS:
        ms, k = C.c_double(0), C.c_int64(0)
        lib.epi_prof_get(label.encode(), C.byref(ms), C.byref(k))
        out[label] = ms.value
    return out


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def host_loop(rep, state):
    """states and score of the whole table by epi_segment_chain_host over its chains (one class: series order = row order)"""
    cols = {k: rep[k].cpu().numpy() for k in S.CX}
    n = cols["pos"].size
    cut = np.flatnonzero((cols["rname"][1:] != cols["rname"][:-1]) | (cols["pos"][1:].astype(np.int64) - cols["pos"][:-1] > MAX_GAP)) + 1
    starts = [0] + cut.tolist() + [n]
    tabs = np.zeros(3 * K + K * K, np.int32)
    p, trans, init = (np.ascontiguousarray(np.asarray(x, np.float64).reshape(-1)) for x in MODEL)
    ea._lib.check(lib.epi_segment_quantise(K, p.ctypes.data, trans.ctypes.data, init.ctypes.data, tabs.ctypes.data))
    total, want = 0, np.zeros(n, np.int32)
    for lo, hi in zip(starts, starts[1:]):
        m, u = np.ascontiguousarray(cols["meth"][lo:hi]), np.ascontiguousarray(cols["unmeth"][lo:hi])
        st, sc = np.zeros(hi - lo, np.int32), C.c_int64(0)
        ea._lib.check(lib.epi_segment_chain_host(K, tabs.ctypes.data, m.ctypes.data, u.ctypes.data, hi - lo, MAX_COVERAGE, st.ctypes.data, C.byref(sc)))
        want[lo:hi] = st
        total += sc.value
    return len(starts) - 1, total, bool(np.array_equal(want, state.cpu().numpy()))


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 28_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    rep = make_table(n)
    per = (n + N_RNAME - 1) // N_RNAME
    nb = (n + lib.epi_segment_block_sites() - 1) // lib.epi_segment_block_sites()
    print("library %s; %d sites over %d rnames, mean gap %.1f, mean coverage %.2f, K = %d, %d sites per workgroup, %d per thread" % (
        os.path.basename(ea._lib.LIB_PATH), n, N_RNAME, float(rep["pos"][per - 1]) / per, float((rep["meth"] + rep["unmeth"]).double().mean()), K,
        lib.epi_segment_block_sites(), lib.epi_segment_thread_sites()))
    # correctness first
    for a in (0, per - 1500, n - 3000):
        a = max(a, 0)
        sub = {k: v[a:a + 3000].cpu().numpy() for k, v in rep.items()}
        for max_iter in (1, 5):
            got = ea.rcpp_cx_segment(ea.Report({k: torch.from_numpy(v).cuda() for k, v in sub.items()}, rep.levels["rname"]), *MODEL, max_iter=max_iter)
            want = G.segment_np(sub, *MODEL, max_iter=max_iter)
            assert np.array_equal(got["state"], want["state"]) and (got.nchain, got.nsegment) == (want["nchain"], want["nsegment"])
            G.same_segments(got.segments, want["segments"], "rows %d.." % a)
            G.same_fit(got.fit, want["fit"], "rows %d.." % a)
    print("  equal to the restatement on 3 windows of 3000 rows, max_iter 1 and 5: states, segments, fit and score")
    decode = lambda: ea.rcpp_cx_segment(rep, *MODEL, max_iter=1, as_device=True)
    out = decode()                                                       # warm-up
    nchain, score, same = host_loop(rep, out["state"])
    assert same and score == out.fit["score"] and nchain == out.nchain
    g = out.nsegment
    print("  whole table, one decode: %d chains, %d segments, score %d; states and score equal the host loop's over every chain" % (nchain, g, score))
    del out
    ts = [prof_run(decode) for _ in range(reps)]
    total = 0.0
    for label in LABELS[:-1]:
        v = [t[label] for t in ts]
        med = statistics.median(v)
        total += med
        b = BYTES[label](n, nb, g)
        print("    %-18s %8.3f ms [%.3f, %.3f]   %7.1f MB   %5.1f %% of the copy rate" % (label, med, min(v), max(v), b / 1e6, 100 * b / (med * 1e-3) / HBM_COPY_RATE))
    print("    sum of the medians %.3f ms = %.2f G sites/s; forward + backward %.3f ms" % (
        total, n / total / 1e6, sum(statistics.median([t[x] for t in ts]) for x in LABELS[2:8])))
    walls = [wall(decode)[0] for _ in range(reps)]
    print("  the call, host clock, max_iter 1: %.2f ms [%.2f, %.2f]" % (1e3 * statistics.median(walls), 1e3 * min(walls), 1e3 * max(walls)))
    # the refit: the whole call at max_iter 6 against the pure decode
    refit = lambda: ea.rcpp_cx_segment(rep, *MODEL, max_iter=6, as_device=True)
    t_refit, out = wall(refit)
    its = out.fit["iterations"]
    tr = [prof_run(refit) for _ in range(reps)]
    walls6 = [wall(refit)[0] for _ in range(reps)]
    cnt = statistics.median([t["segment_counts"] for t in tr]) / max(its if out.fit["converged"] else its - 1, 1)   # (a launch behind every decode but a last one at max_iter)
    print("  refit, max_iter 6: %d decodes, converged %d, p = %s, %d segments" % (its, out.fit["converged"], np.round(out.fit["p"], 4).tolist(), out.nsegment))
    print("    the call %.2f ms [%.2f, %.2f]; per iteration beyond the first %.2f ms (a decode, the counts kernel %.3f ms a launch [%.1f MB], one read of the counters, "
          "the host's re-estimate)" % (1e3 * statistics.median(walls6), 1e3 * min(walls6), 1e3 * max(walls6),
                                       1e3 * (statistics.median(walls6) - statistics.median(walls)) / max(its - 1, 1), cnt, BYTES["segment_counts"](n, nb, g) / 1e6))
    sys.stdout.flush()


main()
