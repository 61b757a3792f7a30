"""preprocessBam(mates="anywhere"): paired-end input whose mates lie anywhere in the file.

The contract (include/epihip.h, epi_preprocess_bam_anyorder) is
    preprocessBam(F, mates="anywhere", **opts)  ==  preprocessBam(G(F), **opts)
for xm, off, rname, strand, start, levels, paired and nrecs, where G(F) is F with its records regrouped by QNAME: groups
in the order of their first kept record, READ1 before READ2 inside a group (flag & 0xC0, ties in file order).  Both
helpers are here: a raw-record rewriter (read_records / write_records: the records of a BAM, written back byte for byte in
any order) and regroup() = G.  The default mode on G(F) is the CPU-checked reader, so every comparison below is against
an independent path; the kernel (assemble_templates.hip) runs on the GPU."""
import gzip
import os
import random
import struct
import zlib

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

BAM = os.path.join(H.GOLDEN, "bam")
SKIP_DEFAULTS = dict(skip_duplicates=False, skip_secondary=True, skip_qcfail=True, skip_supplementary=True)


@pytest.fixture(scope="module")
def ea():
    import epialleler_amd
    return epialleler_amd


# ---- the raw-record rewriter ------------------------------------------------------------------------------------------

def read_records(path):
    """-> (header bytes, [raw record bytes including block_size])"""
    with open(path, "rb") as f:
        data = gzip.decompress(f.read())
    assert data[:4] == b"BAM\1"
    p = 8 + struct.unpack_from("<i", data, 4)[0]
    n_ref = struct.unpack_from("<i", data, p)[0]
    p += 4
    for _ in range(n_ref):
        p += 4 + struct.unpack_from("<i", data, p)[0] + 4
    hdr, recs = data[:p], []
    while p < len(data):
        bs = struct.unpack_from("<i", data, p)[0]
        recs.append(data[p:p + 4 + bs])
        p += 4 + bs
    return hdr, recs


def write_records(path, hdr, recs, block=4000):
    """header + records as BGZF, in blocks of `block` uncompressed bytes (records straddle blocks and windows)"""
    body = bytes(hdr) + b"".join(recs)

    def bgzf(data):
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        comp = co.compress(data) + co.flush()
        return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(comp) + 25) + comp +
                struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))

    with open(path, "wb") as f:
        for i in range(0, len(body), block):
            f.write(bgzf(body[i:i + block]))
        f.write(bgzf(b""))
    return path


def fields(rec):
    """(qname, flag, mapq, tid, pos, has usable XG and XM) of a raw record; None for a record that does not parse"""
    try:
        tid, pos, l_qname, mapq, _, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHi", rec, 4)
        qname = rec[36:36 + l_qname - 1]
        p = 36 + l_qname + 4 * n_cig + (l_seq + 1) // 2 + l_seq
        if p > len(rec):
            return None
        z = {}
        while p + 3 <= len(rec):
            tag, ty = rec[p:p + 2], chr(rec[p + 2])
            p += 3
            if ty in "AcC":
                p += 1
            elif ty in "sS":
                p += 2
            elif ty in "iIf":
                p += 4
            elif ty in "ZH":
                e = rec.index(b"\0", p)
                if ty == "Z":
                    z.setdefault(tag, rec[p:e])
                p = e + 1
            elif ty == "B":
                sub, cnt = chr(rec[p]), struct.unpack_from("<i", rec, p + 1)[0]
                p += 5 + cnt * (1 if sub in "cC" else 2 if sub in "sS" else 4)
            else:
                break
        return qname, flag, mapq, tid, pos, (b"XG" in z and b"XM" in z)
    except (struct.error, ValueError):
        return None


def kept(f, min_mapq=0, skip_duplicates=False, skip_secondary=True, skip_qcfail=True, skip_supplementary=True, **_):
    """what the paired-end packer uses (pack_pe)"""
    if f is None:
        return False
    _, flag, mapq, _, _, usable = f
    skip = 4 | 8 | (256 if skip_secondary else 0) | (512 if skip_qcfail else 0) | \
        (1024 if skip_duplicates else 0) | (2048 if skip_supplementary else 0)
    return not (flag & skip) and bool(flag & 2) and mapq >= min_mapq and usable


def regroup(recs, **opts):
    """G(F): records grouped by QNAME, groups in the order of their first kept record (groups without one last),
    READ1 before READ2 inside a group, ties in file order"""
    fs = [fields(r) for r in recs]
    first, seen = {}, {}
    for i, f in enumerate(fs):
        q = f[0] if f else ("?%d" % i).encode()
        seen.setdefault(q, i)
        if kept(f, **opts):
            first.setdefault(q, i)
    big = len(recs)

    def key(i):
        q = fs[i][0] if fs[i] else ("?%d" % i).encode()
        return (first.get(q, big), seen[q], (fs[i][1] & 0xC0) if fs[i] else 0, i)
    return [recs[i] for i in sorted(range(len(recs)), key=key)]


def coordinate_sorted(recs):
    def key(i):
        f = fields(recs[i])
        tid = f[3] if f and f[3] >= 0 else 1 << 40
        return (tid, f[4] if f else 0, i)
    return [recs[i] for i in sorted(range(len(recs)), key=key)]


def shuffled(recs, seed=11):
    out = list(recs)
    random.Random(seed).shuffle(out)
    return out


def same(a, b):
    for k in ("xm", "off", "rname", "strand", "start"):
        assert np.array_equal(a.host[k], b.host[k]), k
    assert (a.n, a.nbytes, a.nrecs, a.paired, a.levels) == (b.n, b.nbytes, b.nrecs, b.paired, b.levels)


def check_contract(ea, tmp_path, hdr, recs, name, **opts):
    """anyorder(F) == preprocessBam(G(F)) for F = recs as given, on these options"""
    f = write_records(str(tmp_path / (name + ".bam")), hdr, recs)
    g = write_records(str(tmp_path / (name + "-G.bam")), hdr, regroup(recs, **opts))
    a = ea.preprocessBam(f, mates="anywhere", **opts)
    same(a, ea.preprocessBam(g, **opts))
    return a


# ---- the reference's fixture ------------------------------------------------------------------------------------------

def test_reference_unsorted_fixture(ea):
    a = ea.preprocessBam(os.path.join(BAM, "dragen-pe-unsort-xg-xm.bam"), mates="anywhere")
    b = ea.preprocessBam(os.path.join(BAM, "dragen-pe-namesort-xg-xm.bam"))
    assert a.n == b.n == 100 and a.nrecs == b.nrecs == 200 and a.paired and a.levels == b.levels

    def rows(x):
        h = x.host
        r = [(int(h["rname"][i]), int(h["start"][i]), int(h["strand"][i]), bytes(h["xm"][h["off"][i]:h["off"][i + 1]]))
             for i in range(x.n)]
        return sorted(r)
    assert rows(a) == rows(b)
    sp = H.expected()["survey_probe"]["dragen-pe-namesort-xg-xm"]
    r = ea.generateCytosineReport(a, threshold_reads=False, report_context="CX")
    assert [r["pos"].size, int(r["meth"].sum()), int(r["unmeth"].sum())] == sp["cx_nothr"] == [3827, 435, 5214]
    assert [int((r["context"] == k).sum()) for k in (2, 6, 7)] == sp["cx_ctx_rows"]
    H.assert_reports_equal(ea.generateCytosineReport(a), ea.generateCytosineReport(b))
    H.assert_reports_equal(ea.generateMhlReport(a), ea.generateMhlReport(b), float_cols=("lMHL",))
    # through **preprocess_args, from the file itself
    H.assert_reports_equal(ea.generateCytosineReport(os.path.join(BAM, "dragen-pe-unsort-xg-xm.bam"), mates="anywhere"),
                           ea.generateCytosineReport(b))
    # the default mode still refuses the file
    with pytest.raises(ValueError) as ei:
        ea.preprocessBam(os.path.join(BAM, "dragen-pe-unsort-xg-xm.bam"))
    assert "not sorted by name" in str(ei.value)


# ---- the contract on the fixtures -------------------------------------------------------------------------------------

GRID = [
    {},
    {"nthreads": 8, "window_kib": 1},
    {"min_mapq": 20, "min_baseq": 25, "trim": (4, 1)},
    {"skip_duplicates": True, "skip_secondary": False, "skip_supplementary": False},
]


@pytest.mark.parametrize("name", ["dragen-pe-namesort-xg-xm", "dragen-pe-unsort-xg-xm", "amplicon010meth", "capture"])
@pytest.mark.parametrize("order", ["shipped", "coordinate", "shuffled"])
def test_contract_on_fixtures(ea, tmp_path, name, order):
    hdr, recs = read_records(os.path.join(BAM, name + ".bam"))
    recs = {"shipped": recs, "coordinate": coordinate_sorted(recs), "shuffled": shuffled(recs)}[order]
    for k, opts in enumerate(GRID):
        a = check_contract(ea, tmp_path, hdr, recs, "%s-%d" % (name, k), **opts)
        assert a.n > 0 and a.nrecs == len(recs)


# ---- synthetic paired-end files ---------------------------------------------------------------------------------------

NT16 = {c: i for i, c in enumerate("=ACMGRSVTWYHKDBN")}


def encode(r):
    seq, n = r["seq"], len(r["seq"])
    qname = r["qname"].encode() + b"\0"
    packed = bytearray((n + 1) // 2)
    for i, ch in enumerate(seq):
        packed[i >> 1] |= NT16[ch] << (4 if (i & 1) == 0 else 0)
    aux = b"".join(t.encode() + b"Z" + v.encode() + b"\0" for t, v in r["tags"].items())
    core = struct.pack("<iiBBHHHiiii", r["tid"], r["pos"] - 1, len(qname), r["mapq"], 4680, len(r["cigar"]), r["flag"], n,
                       r["tid"], r["mpos"] - 1, r["isize"])
    rec = core + qname + b"".join(struct.pack("<I", (ln << 4) | op) for op, ln in r["cigar"]) + bytes(packed) + \
        bytes(r["qual"]) + aux
    return struct.pack("<i", len(rec)) + rec


def header(contigs):
    text = "@HD\tVN:1.0\tSO:unknown\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in contigs)
    h = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(contigs))
    for name, ln in contigs:
        h += struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<i", ln)
    return h


def span(cigar):
    return sum(ln for op, ln in cigar if op in (0, 2, 3, 7, 8))


def random_cigar(rng, ln):
    """a CIGAR over ln query bases with I / D / N / S / = / X ops, sometimes ending in D"""
    if rng.random() < 0.5:
        return [(0, ln)]
    ops, q = [], 0
    if rng.random() < 0.3:
        s = rng.randint(1, 5)
        ops.append((4, s))
        q += s
    while q < ln:
        k = min(ln - q, rng.randint(5, 40))
        ops.append((rng.choice((0, 0, 7, 8)), k))
        q += k
        if q < ln and rng.random() < 0.5:
            op = rng.choice((1, 2, 3))
            if op == 1:
                k = min(ln - q, rng.randint(1, 4))
                ops.append((1, k))
                q += k
            else:
                ops.append((op, rng.randint(1, 6) if op == 2 else rng.randint(20, 200)))
    if rng.random() < 0.2:
        ops.append((2, rng.randint(1, 5)))                                      # D at the record's end
    return ops


def synth_pairs(rng, n, ncontigs=3, clen=200000, wide=True):
    """Paired-end templates (XG and XM on every record): overlapping mates with equal qualities and disagreeing bytes,
    dovetails, every CIGAR op, orphans whose mate falls to mapq or the duplicate flag, a third record (secondary /
    supplementary) on some QNAMEs, mates in either order, and (wide) a 10 kb pair."""
    contigs = [("c%03d" % i, clen) for i in range(ncontigs)]
    recs = []
    for k in range(n):
        tid = rng.randrange(ncontigs)
        big = wide and k == n // 3
        l1, l2 = (100, 100) if big else (rng.randint(30, 150), rng.randint(30, 150))
        p1 = rng.randint(1, clen - 12000)
        kind = k % 6
        if big:
            p2 = p1 + 9900
        elif kind == 0:                                                          # full overlap, equal qualities
            p2, l2 = p1, l1
        elif kind == 1:                                                          # dovetail: the mate starts first
            p2 = max(1, p1 - rng.randint(1, 40))
        else:
            p2 = p1 + rng.randint(0, 300)
        c1 = [(0, l1)] if big or kind == 0 else random_cigar(rng, l1)
        c2 = [(0, l2)] if big or kind == 0 else random_cigar(rng, l2)
        lo, hi = min(p1, p2), max(p1 + span(c1), p2 + span(c2))
        rev = rng.random() < 0.5
        dup = 1024 if k % 17 == 3 else 0
        xg = "CT" if rng.random() < 0.5 else "GA"
        qeq = bytes([30]) * max(l1, l2) if kind == 0 else None
        mates = []
        for m, (p, c, ln) in enumerate(((p1, c1, l1), (p2, c2, l2))):
            other = p2 if m == 0 else p1
            flag = 1 | 2 | (64 if m == 0 else 128) | dup | ((16 if m == 0 else 32) if rev else (32 if m == 0 else 16))
            r = {"qname": "pair%06d" % k, "tid": tid, "pos": p, "mpos": other, "cigar": c, "flag": flag,
                 "isize": (hi - lo) if p <= other else -(hi - lo),
                 "seq": "".join(rng.choice("ACGTN" if rng.random() < 0.1 else "ACGT") for _ in range(ln)),
                 "qual": qeq[:ln] if qeq else bytes(rng.randint(2, 41) for _ in range(ln)),
                 "mapq": 5 if k % 19 == 4 and m == 1 else 60}
            r["tags"] = {"XG": xg, "XM": "".join(rng.choice("zZxXhH.") for _ in range(ln)), "NM": "0"}
            mates.append(r)
        if k % 23 == 7:                                                          # a third record of the QNAME
            extra = dict(mates[rng.randrange(2)])
            extra["flag"] |= rng.choice((256, 2048))
            extra["tags"] = {"XG": xg, "XM": "".join(rng.choice("zZxXhH.") for _ in extra["seq"]), "NM": "0"}
            mates.append(extra)
        if rng.random() < 0.5:
            mates.reverse()                                                      # READ2 first in the file
        recs.extend(mates)
    return contigs, recs


SYNTH_GRID = [
    {"nthreads": 1},
    {"nthreads": 16, "window_kib": 8},
    {"nthreads": 8, "min_mapq": 20, "min_baseq": 25, "trim": (4, 1), "window_kib": 4},
    {"nthreads": 4, "skip_duplicates": True, "skip_secondary": False, "skip_supplementary": False, "window_kib": 16},
]


def split_mates(recs):
    """every READ1 first, then every READ2: mates thousands of records apart"""
    fs = [fields(r) for r in recs]
    return [r for r, f in zip(recs, fs) if not f[1] & 128] + [r for r, f in zip(recs, fs) if f[1] & 128]


@pytest.mark.parametrize("order", ["grouped", "coordinate", "shuffled", "split"])
def test_contract_synthetic(ea, tmp_path, order):
    rng = random.Random(7)
    contigs, recs = synth_pairs(rng, 3000)
    raw = [encode(r) for r in recs]
    raw = {"grouped": raw, "coordinate": coordinate_sorted(raw), "shuffled": shuffled(raw, 5), "split": split_mates(raw)}[order]
    hdr = header(contigs)
    for k, opts in enumerate(SYNTH_GRID):
        a = check_contract(ea, tmp_path, hdr, raw, "syn-%s-%d" % (order, k), **opts)
        lens = np.diff(a.host["off"])
        assert a.n > 2000 and lens.max() > 9000 > 2048       # the 10 kb pair: the kernel's global-memory path
        assert (lens <= 2048).sum() > 2000                   # and the LDS path


def test_contract_400_contigs_and_threads(ea, tmp_path):
    rng = random.Random(3)
    contigs, recs = synth_pairs(rng, 2500, ncontigs=400, clen=20000, wide=False)
    raw = coordinate_sorted([encode(r) for r in recs])
    hdr = header(contigs)
    a = check_contract(ea, tmp_path, hdr, raw, "c400", nthreads=1, window_kib=2)
    b = ea.preprocessBam(str(tmp_path / "c400.bam"), mates="anywhere", nthreads=16, window_kib=2)
    same(a, b)
    assert len(set(a.host["rname"].tolist())) > 350


def test_tie_rule_keeps_the_earlier_record(ea, tmp_path):
    """two fully overlapping mates, equal qualities, different bytes: READ1's bytes win wherever they sit in the file"""
    def pair(read2_first):
        r1 = {"qname": "tie", "tid": 0, "pos": 101, "mpos": 101, "cigar": [(0, 8)], "flag": 1 | 2 | 64 | 32, "isize": 8,
              "seq": "CCCCCCCC", "qual": bytes([30]) * 8, "mapq": 60, "tags": {"XG": "CT", "XM": "ZZZZZZZZ"}}
        r2 = dict(r1, flag=1 | 2 | 128 | 16, isize=-8, seq="TTTTTTTT", tags={"XG": "CT", "XM": "zzzzzzzz"})
        filler = []
        for k in range(600):                                  # other pairs, so that the file is detected as paired-end
            a = dict(r1, qname="f%04d" % k, pos=1001 + 10 * k, mpos=1001 + 10 * k)
            filler += [a, dict(a, flag=r2["flag"], isize=-8)]
        return [encode(x) for x in ([r2] + filler + [r1] if read2_first else [r1] + filler + [r2])]
    hdr = header([("chrT", 20000)])
    for read2_first in (False, True):
        raw = pair(read2_first)
        a = check_contract(ea, tmp_path, hdr, raw, "tie%d" % read2_first)
        row = bytes(a.host["xm"][a.host["off"][0]:a.host["off"][1]])
        assert row == bytes([(NT16["C"] << 4) | H.ctx_to_idx("Z")]) * 8


# ---- single-end and long-read files: exactly the default mode -----------------------------------------------------------

def test_single_end_is_the_default_mode(ea, tmp_path):
    f = os.path.join(BAM, "dragen-se-unsort-xg-xm.bam")
    for opts in ({}, {"nthreads": 8, "window_kib": 1, "skip_duplicates": True}):
        same(ea.preprocessBam(f, mates="anywhere", **opts), ea.preprocessBam(f, **opts))
    rng = random.Random(5)
    recs = []
    for k in range(300):
        seq = "".join(rng.choice("ACGT") for _ in range(rng.randint(20, 80)))
        recs.append({"seq": seq, "pos": rng.randint(1, 900), "flag": rng.choice((0, 16)),
                     "tags": {"MM": "C+m?,0,1;", "ML": [rng.randint(0, 255) for _ in range(2)]}})
    mm = H.write_bam(str(tmp_path / "mm.bam"), recs)
    same(ea.preprocessBam(mm, mates="anywhere"), ea.preprocessBam(mm))


# ---- errors: the default mode's message on G(F) -----------------------------------------------------------------------

def _small_pe(rng):
    contigs, recs = synth_pairs(rng, 700, ncontigs=2, clen=50000, wide=False)
    return contigs, recs


def _bad(kind, recs):
    """one bad record of each kind, in the second half of the file"""
    k = next(k for k in range(350, 700) if k % 6 >= 2 and k % 17 != 3 and k % 19 != 4 and k % 23 != 7)   # a plain pair
    i = next(i for i, x in enumerate(recs) if x["qname"] == "pair%06d" % k and x["flag"] & 64)
    r = dict(recs[i])
    if kind == "cigar":
        r["cigar"] = [(0, len(r["seq"]) + 1)]
    elif kind == "xm":
        r["tags"] = dict(r["tags"], XM=r["tags"]["XM"][:-1])
    elif kind == "tid":
        r["tid"] = 7
    elif kind == "before":                                   # READ1 gives the start; its mate starts before it
        mate = next(j for j in range(len(recs)) if recs[j]["qname"] == r["qname"] and j != i)
        r["mpos"] = r["pos"]
        recs[mate] = dict(recs[mate], pos=max(1, r["pos"] - 10))
    elif kind == "isize":
        r["isize"] = -2 ** 31
    recs[i] = r
    raw = [encode(x) for x in recs]
    if kind == "corrupt":                                    # l_seq beyond the record's end
        b = bytearray(raw[i])
        struct.pack_into("<i", b, 4 + 16, 10 ** 6)
        raw[i] = bytes(b)
    return raw


@pytest.mark.parametrize("kind", ["corrupt", "cigar", "xm", "tid", "before", "isize"])
def test_errors_match_default_mode_on_G(ea, tmp_path, kind):
    contigs, recs = _small_pe(random.Random(13))
    raw = coordinate_sorted(_bad(kind, recs))
    hdr = header(contigs)
    f = write_records(str(tmp_path / "bad.bam"), hdr, raw)
    g = write_records(str(tmp_path / "bad-G.bam"), hdr, regroup(raw))
    with pytest.raises(ValueError) as want:
        ea.preprocessBam(g)
    with pytest.raises(ValueError) as got:
        ea.preprocessBam(f, mates="anywhere")
    assert str(got.value) == str(want.value)
    assert {"corrupt": "corrupt BAM record", "cigar": "CIGAR does not match", "xm": "XM tag shorter",
            "tid": "reference id out of range", "before": "starts before its template",
            "isize": "template length"}[kind] in str(got.value)


# ---- the kernel ran -----------------------------------------------------------------------------------------------------

def test_kernel_launches_are_profiled(ea):
    from epialleler_amd import _lib
    import ctypes as C
    lib = _lib.load()

    def launches(path):
        lib.epi_prof_reset()
        lib.epi_prof_enable(1)
        try:
            ea.preprocessBam(path, mates="anywhere")
            n = C.c_int64(0)
            ms = C.c_double(0)
            _lib.check(lib.epi_prof_get(b"assemble_templates", C.byref(ms), C.byref(n)))
        finally:
            lib.epi_prof_enable(0)
        return n.value
    assert launches(os.path.join(BAM, "dragen-pe-unsort-xg-xm.bam")) >= 1
    assert launches(os.path.join(BAM, "dragen-se-unsort-xg-xm.bam")) == 0
