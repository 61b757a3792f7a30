"""generateMbiasReport's kernels beside epi_batch_threshold_reads_dev on the same resident batch in one process -- kernel time
from epi_prof (prof_begin / prof_end), median and range of 9 repeats after a warm-up, and the byte-stream bound nbytes / 8 TB/s:
the driver of profiles/mbias_report.txt.
    python scratch/mbias_profile.py cfg2 [max_offset]     10 M PE150 templates (300 bytes), the bench's cfg2 stream
    python scratch/mbias_profile.py cfg5 [max_offset]     500 000 long reads of 10 kb, the bench's cfg5 stream at a tenth of its rows
With EPIHIP_LIB=epialleler_amd/csrc/libepihip_tmbias.so (`make -C epialleler_amd/csrc timing-mbias`) the M-bias kernel is the
shape the shipped one replaced (a wave per row, a lane per byte, LDS atomics).  The threshold kernel reads the same bytes and
is the same in both libraries: the yardstick.  Before anything is timed the table is compared with the restatement
(tests/mbias_np.py) on three row windows of the resident batch, and its totals with a byte histogram of the whole batch."""
import ctypes as C
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import mbias_np as MB  # noqa: E402
import epialleler_amd as ea  # noqa: E402
from epialleler_amd import synth  # noqa: E402

lib = ea._lib.load()
SHAPES = {"cfg2": dict(n_total=10_000_000, mean_len=300), "cfg5": dict(n_total=500_000, mean_len=10_000)}
WINDOW = {"cfg2": 2000, "cfg5": 60}
HBM_PEAK = 8.0e12


def prof(fn, label):
    lib.epi_prof_reset(); lib.epi_prof_enable(1)
    try:
        fn()
    finally:
        lib.epi_prof_enable(0)
    ms, n = C.c_double(0), C.c_int64(0)
    lib.epi_prof_get(label.encode(), C.byref(ms), C.byref(n))
    return ms.value


def repeats(fn, label, reps=9):
    fn()
    ts = [prof(fn, label) for _ in range(reps)]
    return statistics.median(ts), min(ts), max(ts)


def window(bam, a, b):
    """Rows [a, b) of a resident batch as a batch of their own and as host arrays"""
    d = bam.dev
    o0, o1 = int(d["off"][a]), int(d["off"][b])
    xm = torch.zeros(((o1 - o0 + 15) // 16 * 16 + 64,), dtype=torch.uint8, device=d["xm"].device)
    xm[:o1 - o0] = d["xm"][o0:o1]
    off = (d["off"][a:b + 1] - o0).contiguous()
    cols = [d[k][a:b].contiguous() for k in ("rname", "strand", "start")]
    sub = ea.ProcessedBam.from_device(xm, o1 - o0, off, *cols, bam.levels)
    t = dict(xm=xm[:o1 - o0].cpu().numpy(), off=off.cpu().numpy(), strand=cols[1].cpu().numpy())
    return sub, t


def main():
    shape = sys.argv[1]
    M = int(sys.argv[2]) if len(sys.argv) > 2 else 150
    bam = synth.generate_device_uniform(seed=42, n_chr=4, ragged=False, gap_every=0, device=0, **SHAPES[shape])
    bam.batch()
    n, nbytes = bam.n, bam.nbytes
    print("library %s; %s: %d rows, %d bytes, max_offset %d" % (os.path.basename(ea._lib.LIB_PATH), shape, n, nbytes, M))
    # correctness first
    w = WINDOW[shape]
    for a in (0, n // 2 - w // 2, n - w):
        sub, t = window(bam, a, a + w)
        got = ea.rcpp_mbias_report(sub, M)
        want, want_tot = MB.restate(t, M)
        MB.same({k: np.asarray(v) for k, v in got.items()}, want, "rows %d.." % a)
        MB.same(dict(got.totals), want_tot, "totals of rows %d.." % a)
        sub.close()
    rep = ea.rcpp_mbias_report(bam, M)
    hist = torch.zeros(16, dtype=torch.int64, device="cuda:0")
    step = 1 << 28
    for o in range(0, nbytes, step):
        hist += torch.bincount((bam.dev["xm"][o:min(o + step, nbytes)] & 15).to(torch.int32), minlength=16)
    hist = hist.cpu().numpy()
    for code, (k, state) in MB.CLASS.items():
        both = int(rep.totals["unmeth" if state else "meth"][rep.totals["context"] == MB.CODES[k]].sum())
        assert both == int(hist[code]), (code, both, int(hist[code]))
    again = ea.rcpp_mbias_report(bam, M)
    MB.same({k: np.asarray(v) for k, v in again.items()}, {k: np.asarray(v) for k, v in rep.items()}, "second call")
    print("  table equal to the restatement on 3 windows of %d rows; totals equal to the batch's byte histogram; second call identical" % w)
    print("  classed bytes %d of %d; table cells filled %d of %d" % (int(rep.totals["meth"].sum() + rep.totals["unmeth"].sum()), nbytes,
                                                                   int(((rep["meth"] + rep["unmeth"]) > 0).sum()), rep.nrow))
    # timing
    bound = nbytes / HBM_PEAK * 1e3
    for label, what, fn in (("mbias_report", "epi_batch_mbias_report_dev (both kernels)", lambda: ea.rcpp_mbias_report(bam, M, as_device=True)),
                            ("threshold", "epi_batch_threshold_reads_dev", lambda: ea.rcpp_threshold_reads(bam, "Z", "z", "XH", "xh", 2, 0.5, 0.1, as_device=True))):
        med, lo, hi = repeats(fn, label)
        print("  %-44s %8.3f ms [%.3f, %.3f]   %5.2f TB/s   %4.1fx the bound of %.3f ms" % (what, med, lo, hi, nbytes / med / 1e9, med / bound, bound))
    sys.stdout.flush()


main()
