"""compareHeterogeneity timed on two pairs of batches, next to the two generateHeterogeneityReport calls a user runs
without it -- the driver of profiles/heterogeneity_compare.txt.
    python scratch/heterogeneity_compare_profile.py cfg2 [rows]   two batches like bench.py's cfg2 (uniform starts, L = 300) on
                                                                  one site grid: the same content seed, other row starts
    python scratch/heterogeneity_compare_profile.py deep          two deep targets of heterogeneity_profile.py on the same 25
                                                                  sites, each with 200 XM strings of its own
Each: the whole call (median [min, max] of 9 repeats after one untimed call, stream synchronised, as_device), k = 4, CG; the
kernels of the comparison (epi_prof "hetcmp_intersect": match + scan, "hetcmp_compact": compaction + the common per-strand
table, "hetcmp_count_a", "hetcmp_count_b", "hetcmp_keep": keep + scan, "hetcmp_emit": the fetch's kernel) and the counting
and emit kernels of the two single reports ("het_count", "het_emit", summed over both)."""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.argv, argv = [sys.argv[0], "none"], sys.argv           # (heterogeneity_profile runs a mode when imported with one; it prints the library's name)
sys.path[:0] = [HERE]
from heterogeneity_profile import ea, kernel_ms, lib, np, synth, timed, torch  # noqa: E402

sys.argv = argv


def cfg2_like(rows, start_seed, content_seed=5):
    """synth.generate_device_uniform(ragged=False, gap_every=0) with the row starts of one seed and the content of another:
    the contexts are a function of (content seed, sequence, position), so two such batches share their site grid."""
    dev = "cuda:%d" % torch.cuda.current_device()
    rname, start, lens = synth.uniform_layout(rows, 300, 4, 30, start_seed, 0, rows, dev, False, None)
    off = torch.zeros(rows + 1, dtype=torch.int64, device=dev)
    torch.cumsum(lens, 0, out=off[1:])
    nbytes = int(off[-1].item())
    xm = torch.empty((nbytes + 15) // 16 * 16 + 64, dtype=torch.uint8, device=dev)
    xm[nbytes:] = 0xFB
    strand = torch.empty(rows, dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ea._lib.check(lib.epi_synth_fill_dev(content_seed, 0, rows, C.c_void_p(off.data_ptr()), C.c_void_p(rname.data_ptr()),
                                         C.c_void_p(start.data_ptr()), nbytes, 0, 50, C.c_void_p(xm.data_ptr()),
                                         C.c_void_p(strand.data_ptr()), stream))
    levels = tuple("chrS%d" % (i + 1) for i in range(4))
    return ea.ProcessedBam.from_device(xm, nbytes, off, rname.contiguous(), strand, start.contiguous(), levels)


def deep_target(pat_seed, n=10 ** 6, npat=200, L=250):
    """heterogeneity_profile.deep_bam with the 25 sites of seed 1 and the XM strings of pat_seed."""
    sites = np.sort(np.random.default_rng(1).choice(L, 25, replace=False))
    rng = np.random.default_rng(pat_seed)
    pats = np.full((npat, L), ord("."), np.uint8)
    seen = set()
    k = 0
    while k < npat:
        m = rng.integers(0, 2, size=25)
        if m.tobytes() in seen:
            continue
        seen.add(m.tobytes())
        pats[k, sites] = np.where(m == 1, ord("Z"), ord("z"))
        k += 1
    body = np.concatenate([np.zeros(int(n * 0.55), np.int64), rng.integers(1, npat, size=n - int(n * 0.55))])
    rng.shuffle(body)
    xm = pats[body].reshape(-1).astype(np.int64)
    packed = ((1 << 4) | (((xm + 2) >> 2) & 15)).astype(np.uint8)
    off = np.arange(n + 1, dtype=np.int64) * L
    return ea.ProcessedBam.from_arrays(packed, off, np.ones(n, np.int32), np.ones(n, np.int32), np.full(n, 1000, np.int32), levels=("chrA",))


def run(name, a, b, reps=9):
    print(name)
    het = lambda x: ea.generateHeterogeneityReport(x, window_context="CG", window_sites=4, as_device=True)
    state = {"flip": False}

    def both():                                              # what a user runs today, in alternating order
        state["flip"] = not state["flip"]
        first, second = (a, b) if state["flip"] else (b, a)
        return het(first).nrow + het(second).nrow
    cmp_ = lambda: ea.compareHeterogeneity(a, b, window_context="CG", window_sites=4, as_device=True)
    nsingle, t_both = timed(both, reps)
    rep, t_cmp = timed(cmp_, reps)
    print("  rows %d and %d, common sites %d, windows reported %d (the two single reports: %d)" % (a.n, b.n, rep.ncommon, rep.nrow, nsingle))
    print("  two generateHeterogeneityReport(k=4) calls   %s" % t_both)
    print("  ... their counting kernels (het_count, sum)  %s" % kernel_ms(both, "het_count", reps))
    print("  ... their emit kernels (het_emit, sum)       %s" % kernel_ms(both, "het_emit", reps))
    print("  compareHeterogeneity(k=4)                    %s" % t_cmp)
    for label in ("hetcmp_intersect", "hetcmp_compact", "hetcmp_count_a", "hetcmp_count_b", "hetcmp_keep", "hetcmp_emit"):
        print("  ... %-41s%s" % (label, kernel_ms(cmp_, label, reps)))
    sys.stdout.flush()


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "cfg2":
        rows = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
        a, b = cfg2_like(rows, 5), cfg2_like(rows, 6)
        a.batch(); b.batch()
        run("cfg2-like pair: 2 x %d rows of 300 bytes, uniform starts, depth 30, one site grid" % rows, a, b)
    else:
        a, b = deep_target(1), deep_target(2)
        a.batch(); b.batch()
        run("deep-target pair: 2 x 10^6 rows of 250 bytes on the same 25 CpGs, 200 XM strings each, one on 55 % of the rows", a, b)
