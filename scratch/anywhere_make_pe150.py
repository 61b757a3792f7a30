"""Generated PE150 file for the mates="anywhere" measurement: N pairs (2N records), coordinate-sorted, plus its G(F)
twin (the same records grouped by QNAME, READ1 first).  Fixed-size records, built with numpy; BGZF by a process pool."""
import multiprocessing as mp
import struct
import sys
import zlib

import numpy as np

L = 150
QN = 11                      # "r%09d\0"
REC = 4 + 32 + QN + 4 + L // 2 + L + 6 + (3 + L + 1)


def build(npairs, seed=1):
    rng = np.random.default_rng(seed)
    ncontig, clen = 24, 10_000_000
    n = 2 * npairs
    pid = np.repeat(np.arange(npairs), 2)
    mate = np.tile([0, 1], npairs)
    tid = np.repeat(rng.integers(0, ncontig, npairs), 2).astype(np.int32)
    p1 = rng.integers(0, clen - 1000, npairs)
    ins = rng.integers(180, 500, npairs)
    p2 = p1 + ins - L
    pos = np.where(mate == 0, np.repeat(p1, 2), np.repeat(p2, 2)).astype(np.int32)
    mpos = np.where(mate == 0, np.repeat(p2, 2), np.repeat(p1, 2)).astype(np.int32)
    lo = np.minimum(p1, p2); hi = np.maximum(p1, p2) + L
    w = np.repeat(hi - lo, 2)
    isize = np.where(pos <= mpos, w, -w).astype(np.int32)
    rev = np.repeat(rng.random(npairs) < 0.5, 2)
    flag = np.where(mate == 0, np.where(rev, 83, 99), np.where(rev, 163, 147)).astype(np.uint16)
    r = np.zeros((n, REC), np.uint8)
    r[:, 0:4] = np.frombuffer(np.int32(REC - 4).tobytes(), np.uint8)
    core = np.zeros(n, dtype=[("tid", "<i4"), ("pos", "<i4"), ("lq", "u1"), ("mapq", "u1"), ("bin", "<u2"), ("nc", "<u2"),
                              ("flag", "<u2"), ("ls", "<i4"), ("mtid", "<i4"), ("mpos", "<i4"), ("isize", "<i4")])
    core["tid"] = tid; core["pos"] = pos; core["lq"] = QN; core["mapq"] = 60; core["bin"] = 4680; core["nc"] = 1
    core["flag"] = flag; core["ls"] = L; core["mtid"] = tid; core["mpos"] = mpos; core["isize"] = isize
    r[:, 4:36] = core.view(np.uint8).reshape(n, 32)
    o = 36
    r[:, o] = ord("r")
    d = pid.copy()
    for k in range(9):
        r[:, o + 9 - k] = ord("0") + d % 10
        d //= 10
    o += QN
    r[:, o:o + 4] = np.frombuffer(np.uint32(L << 4).tobytes(), np.uint8)
    o += 4
    nt = rng.choice(np.array([1, 2, 4, 8], np.uint8), size=(n, L))
    r[:, o:o + L // 2] = (nt[:, 0::2] << 4) | nt[:, 1::2]
    o += L // 2
    r[:, o:o + L] = rng.integers(2, 42, size=(n, L), dtype=np.uint8)
    o += L
    xg = np.where(np.repeat(rng.random(npairs) < 0.5, 2)[:, None], np.frombuffer(b"XGZCT\0", np.uint8), np.frombuffer(b"XGZGA\0", np.uint8))
    r[:, o:o + 6] = xg
    o += 6
    r[:, o:o + 3] = np.frombuffer(b"XMZ", np.uint8)
    letters = np.frombuffer(b"..........zZxXhHhh", np.uint8)
    r[:, o + 3:o + 3 + L] = letters[rng.integers(0, len(letters), size=(n, L))]
    r[:, o + 3 + L] = 0
    assert o + 4 + L == REC
    order_f = np.lexsort((np.arange(n), pos, tid))
    # G(F): groups in the order of their first record in F, READ1 then READ2
    first = np.full(npairs, n, np.int64)
    np.minimum.at(first, pid[order_f], np.arange(n))
    order_g = np.lexsort((mate, pid, first[pid]))
    return ncontig, clen, r, order_f, order_g


def bgzf(data):
    co = zlib.compressobj(1, zlib.DEFLATED, -15)
    comp = co.compress(data) + co.flush()
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(comp) + 25) + comp +
            struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def write(path, hdr, body, pool):
    chunks = [body[i:i + 65280] for i in range(0, len(body), 65280)]
    with open(path, "wb") as f:
        f.write(bgzf(hdr))
        for b in pool.imap(bgzf, chunks, chunksize=64):
            f.write(b)
        f.write(bgzf(b""))


if __name__ == "__main__":
    npairs, out = int(sys.argv[1]), sys.argv[2]
    ncontig, clen, r, of, og = build(npairs)
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:chr%d\tLN:%d\n" % (i + 1, clen) for i in range(ncontig))
    hdr = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", ncontig)
    for i in range(ncontig):
        nm = ("chr%d" % (i + 1)).encode() + b"\0"
        hdr += struct.pack("<i", len(nm)) + nm + struct.pack("<i", clen)
    with mp.Pool(16) as pool:
        write(out + "-coord.bam", hdr, r[of].tobytes(), pool)
        write(out + "-G.bam", hdr, r[og].tobytes(), pool)
    print("wrote %d records (%d bytes each) x2" % (2 * npairs, REC))
