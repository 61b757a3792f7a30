"""generateVcfReport's kernel next to the CX step on the config-2 batch (10 M PE150 templates, uniform starts, depth 30):
one VCF site per ~100 bp, jittered, every 20th duplicated (multi-ALT).  Run under rocprofv3 --kernel-trace --stats;
also prints HIP-event times (epi_prof) and the algorithmic bytes of the base-frequency kernel."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import epialleler_amd as ea  # noqa: E402
from epialleler_amd import _lib, synth  # noqa: E402

ROWS, L, NCHR, DEPTH = 10_000_000, 300, 4, 30
bam = synth.generate_device_uniform(ROWS, mean_len=L, n_chr=NCHR, depth=DEPTH, ragged=False, gap_every=0)
bam.batch()
torch.cuda.synchronize()
glen = ROWS * L // DEPTH // NCHR
rng = np.random.default_rng(1)
chr_, pos = [], []
for c in range(1, NCHR + 1):
    p = np.arange(50, glen, 100) + rng.integers(-40, 40, (glen - 50 + 99) // 100)
    p = np.sort(np.concatenate([p, p[::20]]))
    chr_.append(np.full(p.size, c, np.int32))
    pos.append(p.astype(np.int32))
chr_, pos = np.concatenate(chr_), np.concatenate(pos)
m = chr_.size
lib = _lib.load()
c = ea.CONTEXT_TO_BASES["CG"]
pass_ = ea.rcpp_threshold_reads(bam, c["ctx_meth"], c["ctx_unmeth"], c["ooctx_meth"], c["ooctx_unmeth"], 2, 0.5, 0.1, as_device=True)
d_c, d_p = torch.from_numpy(chr_).cuda(), torch.from_numpy(pos).cuda()
cnt = torch.empty(20 * m, dtype=torch.int32, device="cuda:0")
lib.epi_prof_enable(1)
for it in range(6):
    if it == 1:
        torch.cuda.synchronize()
        lib.epi_prof_reset()
    ea.generateCytosineReport(bam, as_device=True)
    _lib.check(lib.epi_batch_base_freqs_dev(bam.batch(), C.c_void_p(pass_.data_ptr()), C.c_void_p(d_c.data_ptr()),
                                            C.c_void_p(d_p.data_ptr()), m, C.c_void_p(cnt.data_ptr()), None))
torch.cuda.synchronize()
res = {}
for k in ("cx_tiles", "base_freqs"):
    ms, n = C.c_double(), C.c_int64()
    lib.epi_prof_get(k.encode(), C.byref(ms), C.byref(n))
    res[k] = ms.value / max(n.value, 1)
tot = cnt.view(20, m).sum().item()
# algorithmic bytes: off 8 + len 4 + rname 4 + strand 4 + start 4 + pass 4 per row, 8 B per site (twice: window staging is
# per workgroup, counted once), one byte per (row, site) pair, 80 B of counters per site (memset + atomics)
alg = ROWS * 28 + m * 8 + tot + m * 80 * 2
print("sites %d pairs %d  cx_tiles %.3f ms  base_freqs %.3f ms  alg bytes %.3g -> %.2f TB/s = %.3f of 8 TB/s" %
      (m, tot, res["cx_tiles"], res["base_freqs"], alg, alg / res["base_freqs"] / 1e9, alg / res["base_freqs"] / 1e9 / 8))
