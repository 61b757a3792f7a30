"""Seeded crafted BAM files for the reader's differential and sanitizer runs: records whose aux region is random fields
with, in half of them, one malformed field placed before or after XG / XM; XG or XM typed as integer or array; MM + ML
with an ML count past the record; unknown CIGAR operations; l_seq disagreeing with the CIGAR; single records and pairs.
File k is a function of k alone (scratch/bam_refactor_diff.py, tests/test_bam_host_sanitized.py)."""
import os
import random
import struct

from test_preprocess_bam import _raw_bam


def os_bytes(rng, n):
    return bytes(rng.randrange(256) for _ in range(n))


def aux_field(rng, tag=None):
    tag = tag or bytes(rng.choice(b"ABNXYZM") for _ in range(2))
    ty = rng.choice("AcCsSiIfZHB")
    if ty in "AcC":
        return tag + ty.encode() + bytes([rng.randrange(256)])
    if ty in "sS":
        return tag + ty.encode() + os_bytes(rng, 2)
    if ty in "iIf":
        return tag + ty.encode() + os_bytes(rng, 4)
    if ty in "ZH":
        return tag + ty.encode() + bytes(rng.choice(b"zZxXhH.CTGA0123") for _ in range(rng.randrange(0, 12))) + b"\0"
    sub = rng.choice("cCsSiIf")
    n = rng.randrange(0, 6)
    return tag + b"B" + sub.encode() + struct.pack("<I", n) + os_bytes(rng, n * {"c": 1, "C": 1, "s": 2, "S": 2}.get(sub, 4))


def malformed_field(rng, kind):
    tag = bytes(rng.choice(b"ABNXYZ") for _ in range(2))
    if kind == "z_open":                                             # a string without its terminator
        return tag + b"Z" + b"abc"
    if kind == "b_long":                                             # an array whose count runs past the record
        return tag + b"B" + rng.choice((b"c", b"S", b"i")) + struct.pack("<I", rng.choice((7, 1000, 0x7FFFFFFF, 0xFFFFFFFF))) + os_bytes(rng, 3)
    if kind == "b_cut":                                              # an array header cut short
        return tag + b"B" + b"c" + b"\1"
    return tag + bytes([rng.choice(b"?qZ!")]).replace(b"Z", b"k") + os_bytes(rng, rng.randrange(0, 4))   # unknown type


def crafted_record(rng, i, l_seq, pe):
    xm = bytes(rng.choice(b"zZxXhH.") for _ in range(l_seq))
    methyl = [b"XGZ" + rng.choice((b"CT", b"GA")) + b"\0", b"XMZ" + xm + b"\0"]
    r = rng.random()
    if r < 0.15:
        methyl[rng.randrange(2)] = rng.choice((b"XG", b"XM")) + rng.choice((b"i" + os_bytes(rng, 4), b"C\7", b"Bc" + struct.pack("<I", 2) + b"ab"))
    elif r < 0.25:
        methyl = [rng.choice((b"YDZf\0", b"ZSZ+-\0", b"XGZCT\0"))]   # to be called with a genome
    elif r < 0.30:
        methyl.append(b"MMZC+m,1,0;\0")
        methyl.append(b"MLBC" + struct.pack("<I", rng.choice((2, 2, 900))) + b"\x80\xf0")
    fields = [aux_field(rng) for _ in range(rng.randrange(0, 5))]
    for m in methyl:
        fields.insert(rng.randrange(len(fields) + 1), m)
    if rng.random() < 0.5:
        bad = malformed_field(rng, rng.choice(("z_open", "b_long", "b_cut", "unknown")))
        fields.insert(rng.randrange(len(fields) + 1), bad)          # XG / XM land before or after it
    cigar = [(0, l_seq)]
    c = rng.random()
    if c < 0.12:
        cigar = [(0, l_seq // 2), (rng.choice((10, 11, 15)), 3), (0, l_seq - l_seq // 2)]   # an unknown operation
    elif c < 0.24:
        cigar = [(0, l_seq + rng.choice((-2, -1, 1, 5)))]            # l_seq disagrees with the CIGAR
    elif c < 0.5:
        cigar = [(4, 1), (0, l_seq - 3), (2, 2), (1, 1), (3, 4), (0, 1)]
    flag, mpos, tlen = (rng.choice((0, 16)), -1, 0) if not pe else ((99, 150, 40) if i % 2 == 0 else (147, 100, -40))
    qname = (b"q%d" % (i // 2 if pe else i)) + b"\0"
    core = struct.pack("<iiBBHHHiiii", 0, 100 + (i % 2) * 50, len(qname), 60, 4680, len(cigar), flag, l_seq, 0 if pe else -1, mpos, tlen)
    cg = b"".join(struct.pack("<I", (ln << 4) | op) for op, ln in cigar)
    return core + qname + cg + bytes([0x12] * ((l_seq + 1) // 2)) + bytes([40] * l_seq) + b"".join(fields)


def crafted_files(d, n=600):
    paths = []
    for k in range(n):
        rng = random.Random(k)
        pe = k % 3 == 0
        recs = [crafted_record(rng, i, rng.randrange(4, 24), pe) for i in range(2 if pe or rng.random() < 0.5 else 1)]
        paths.append(_raw_bam(os.path.join(d, "crafted_%03d.bam" % k), recs))
    return paths
