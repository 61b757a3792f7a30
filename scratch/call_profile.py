"""callMethylation end to end on a seeded synthetic input: a random genome (2 x 8 Mb, CpG-enriched) and 1 M paired
150 bp bwa-meth-style records (YD tags, name-sorted pairs, bisulfite-converted reads).  Prints records/s and the
library's phase split (EPIHIP_BAM_TIMING=1 on stderr).  Kernel times come from a rocprofv3 run of the same script:

  python scratch/call_profile.py make DIR            # writes DIR/genome.fa, DIR/in.bam
  python scratch/call_profile.py run DIR [NTHREADS]  # calls, prints one JSON line
"""
import json
import os
import struct
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SEED = 20261015
CONTIGS = (("chr1", 8_000_000), ("chr2", 8_000_000))
NPAIR = 500_000
L = 150


def make(d):
    import epialleler_amd as ea
    from epialleler_amd import _lib
    rng = np.random.default_rng(SEED)
    os.makedirs(d, exist_ok=True)
    seqs = {}
    with open(os.path.join(d, "genome.fa"), "w") as f:
        for name, ln in CONTIGS:
            s = rng.choice(np.frombuffer(b"ACGT", np.uint8), ln)
            cg = rng.integers(0, ln - 1, ln // 50)                      # CpG-rich: ~2 % of the positions start a CG
            s[cg], s[cg + 1] = ord("C"), ord("G")
            seqs[name] = s
            f.write(">%s\n" % name)
            b = s.tobytes().decode()
            f.write("\n".join(b[i:i + 60] for i in range(0, ln, 60)) + "\n")
    text = "@HD\tVN:1.0\tSO:queryname\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in CONTIGS)
    hdr = bytearray(b"BAM\1") + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(CONTIGS))
    for name, ln in CONTIGS:
        hdr += struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<i", ln)
    rec = np.dtype([("bs", "<i4"), ("tid", "<i4"), ("pos", "<i4"), ("lrn", "u1"), ("mapq", "u1"), ("bin", "<u2"),
                    ("ncig", "<u2"), ("flag", "<u2"), ("lseq", "<i4"), ("mtid", "<i4"), ("mpos", "<i4"), ("isize", "<i4"),
                    ("qname", "S9"), ("cigar", "<u4"), ("seq", "u1", (L // 2,)), ("qual", "u1", (L,)), ("yd", "S5")])
    n = 2 * NPAIR
    r = np.zeros(n, rec)
    r["bs"] = rec.itemsize - 4
    tid = rng.integers(0, len(CONTIGS), NPAIR)
    p1 = rng.integers(2, CONTIGS[0][1] - 400, NPAIR)
    ins = rng.integers(160, 350, NPAIR)
    p2 = p1 + ins - L
    r["tid"] = np.repeat(tid, 2)
    r["pos"] = np.stack([p1, p2], 1).ravel()
    r["lrn"], r["mapq"], r["bin"], r["ncig"], r["lseq"] = 9, 60, 4680, 1, L
    r["flag"] = np.tile(np.array([99, 147], np.uint16), NPAIR)
    r["mtid"] = r["tid"]
    r["mpos"] = np.stack([p2, p1], 1).ravel()
    r["isize"] = np.stack([ins, -ins], 1).ravel()
    r["qname"] = np.repeat(np.array(["p%07d" % i for i in range(NPAIR)], "S8"), 2)
    r["cigar"] = (L << 4) | 0
    r["qual"] = 37
    strand = rng.integers(0, 2, NPAIR)
    r["yd"] = np.where(np.repeat(strand, 2) == 0, b"YDZf", b"YDZr")
    code = np.zeros(256, np.uint8)
    code[[ord("A"), ord("C"), ord("G"), ord("T")]] = [1, 2, 4, 8]
    for k0 in range(0, n, 100_000):                                      # bases: the genome, bisulfite-converted
        k1 = min(n, k0 + 100_000)
        b = np.empty((k1 - k0, L), np.uint8)
        for t, (name, _) in enumerate(CONTIGS):
            m = r["tid"][k0:k1] == t
            idx = r["pos"][k0:k1][m][:, None] + np.arange(L)[None, :]
            b[m] = seqs[name][idx]
        rev = np.repeat(strand, 2)[k0:k1][:, None] == 1
        conv = rng.random(b.shape) < 0.7
        b = np.where(~rev & (b == ord("C")) & conv, ord("T"), b)
        b = np.where(rev & (b == ord("G")) & conv, ord("A"), b)
        nib = code[b]
        r["seq"][k0:k1] = (nib[:, 0::2] << 4) | nib[:, 1::2]
    body = bytes(hdr) + r.tobytes()
    buf = np.frombuffer(body, np.uint8)
    _lib.check(_lib.load().epi_bgzf_write_file(os.path.join(d, "in.bam").encode(), buf.ctypes.data, buf.size,
                                                min(16, os.cpu_count() or 1)))
    print("wrote %d records, %d inflated bytes" % (n, len(body)))
    del ea


def run(d, nthreads):
    import epialleler_amd as ea
    g = ea.preprocessGenome(os.path.join(d, "genome.fa"), nthreads=nthreads, verbose=False)
    ea.callMethylation(os.path.join(d, "in.bam"), os.path.join(d, "out.bam"), g, nthreads=nthreads, verbose=False)  # warm-up
    t0 = time.time()
    res = ea.callMethylation(os.path.join(d, "in.bam"), os.path.join(d, "out.bam"), g, nthreads=nthreads, verbose=False)
    dt = time.time() - t0
    res.update(seconds=round(dt, 3), records_per_s=round(res["nrecs"] / dt), nthreads=nthreads,
               kernel_bytes=int(res["ncalled"] * (L * 4.5 + 48)))
    print(json.dumps(res))


if __name__ == "__main__":
    if sys.argv[1] == "make":
        make(sys.argv[2])
    else:
        run(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else min(16, os.cpu_count() or 1))
