"""preprocessBam(genome=): methylation called on the GPU inside the reader.  The contract is the composition

    preprocessBam(in, genome=G, **opts) == preprocessBam(callMethylation(in, tmp, G); tmp, **opts)

byte for byte (xm, off, rname, strand, start, levels, paired, nrecs), errors included; `ncalled` is callMethylation's.
Checked on the reference's known answers, on every fixture over an options grid, on synthetic single- and paired-end
BAMs cut into many windows, on each of callMethylation's errors, and through the report functions."""
import ctypes as C
import os
import random
import struct
import zlib

import numpy as np
import pytest

import epialleler_amd as ea
from helpers import GOLDEN, write_bam
from test_gpu_call_methylation import CONTIGS, EXPECTED, many_contigs_input, random_read, synth_records, write_genome

pytestmark = pytest.mark.gpu

BAMS = os.path.join(GOLDEN, "bam")
FASTA = os.path.join(BAMS, "reference.fasta.gz")
FIXTURES = sorted(f for f in os.listdir(BAMS) if f.endswith(".bam"))


@pytest.fixture(scope="module")
def genome():
    return ea.preprocessGenome(FASTA, verbose=False)


@pytest.fixture(scope="module")
def synth_genome(tmp_path_factory):
    d = tmp_path_factory.mktemp("pg_genome")
    write_genome(str(d / "g.fa"), random.Random(20261016))
    return ea.preprocessGenome(str(d / "g.fa"), verbose=False)


def call_launches(fn):
    """fn() with the profiler on; returns (result, call_methylation windows launched)."""
    lib = ea._lib.load()
    lib.epi_prof_reset()
    lib.epi_prof_enable(1)
    try:
        r = fn()
    finally:
        lib.epi_prof_enable(0)
    ms, cnt = C.c_double(0), C.c_int64(0)
    lib.epi_prof_get(b"call_methylation", C.byref(ms), C.byref(cnt))
    return r, cnt.value


def outcome(fn):
    """("ok", result) or ("error", message) of fn()."""
    try:
        return "ok", fn()
    except ValueError as e:
        return "error", str(e)


def assert_same_templates(a, b):
    assert (a.n, a.nbytes, a.nrecs, a.paired, a.levels) == (b.n, b.nbytes, b.nrecs, b.paired, b.levels)
    for k in ("xm", "off", "rname", "strand", "start"):
        assert np.array_equal(np.asarray(a.host[k]), np.asarray(b.host[k])), k


def check_contract(src, g, tmp_path, opts, call_threads=2):
    """Both sides of the contract on one input; returns the direct result (None when both raised)."""
    called = str(tmp_path / "called.bam")
    if os.path.exists(called):
        os.unlink(called)
    kind, res = outcome(lambda: ea.callMethylation(src, called, g, nthreads=call_threads, verbose=False))
    if kind == "ok":
        want_kind, want = outcome(lambda: ea.preprocessBam(called, **opts))
    else:
        want_kind, want = kind, res
    before = sorted(os.listdir(tmp_path))
    got_kind, got = outcome(lambda: ea.preprocessBam(src, genome=g, **opts))
    assert sorted(os.listdir(tmp_path)) == before                   # nothing written
    assert got_kind == want_kind, (src, opts, got if got_kind == "error" else want)
    if got_kind == "error":
        assert got == want
        return None
    assert_same_templates(got, want)
    assert got.ncalled == res["ncalled"] and got.nrecs == res["nrecs"]
    assert want.ncalled == 0
    return got


def reports_equal(a, b):
    if set(a) != set(b):
        return False
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.shape != y.shape or not np.array_equal(x, y, equal_nan=x.dtype.kind == "f"):
            return False
    return True


# ---- 1. the reference's known answers (test_callMethylation.R) -----------------------------------------------------

@pytest.mark.parametrize("expr", sorted(EXPECTED["cx_identical"]))
def test_known_cx_comparisons(expr):
    case = EXPECTED["cx_identical"][expr]
    ref = ea.generateCytosineReport(os.path.join(BAMS, case["ref"]), threshold_reads=False, report_context="CX")
    got = ea.generateCytosineReport(os.path.join(BAMS, case["input"]), genome=FASTA, threshold_reads=False,
                                    report_context="CX")
    assert reports_equal(ref, got) == case["identical"]


# ---- 2. the contract on the fixtures, over an options grid -----------------------------------------------------------

GRID = [
    {},
    {"min_mapq": 30, "nthreads": 8},
    {"min_baseq": 20, "trim": (2, 5), "nthreads": 1},
    {"skip_duplicates": True, "trim": 3, "nthreads": 8, "window_kib": 1},
    {"min_mapq": 10, "min_baseq": 30, "nthreads": 1, "window_kib": 1},
]


@pytest.mark.parametrize("name", FIXTURES)
def test_contract_fixtures(name, genome, tmp_path):
    src = os.path.join(BAMS, name)
    for opts in GRID:
        got, launches = call_launches(lambda: check_contract(src, genome, tmp_path, opts))
        if got is not None and got.ncalled == 0:
            assert launches == 0, (name, opts)                      # an XG/XM file: nothing to call, no kernel
        if got is not None and got.ncalled > 0:
            assert launches >= 1


def test_fixtures_cover_every_tag(genome, tmp_path):
    """The fixture contract above is not vacuous: inputs with each strand tag are accepted and called."""
    for name in ("dragen-pe-namesort-xg.bam", "dragen-se-unsort-xg.bam", "bwameth-pe-namesort-yd.bam",
                 "bwameth-se-unsort-yd.bam", "bsmap-pe-namesort-zs.bam", "bsmap-se-unsort-zs.bam"):
        got = check_contract(os.path.join(BAMS, name), genome, tmp_path, {})
        assert got is not None and got.n > 0 and got.ncalled > 0, name
    got = check_contract(os.path.join(BAMS, "dragen-pe-namesort-xg-xm.bam"), genome, tmp_path, {})
    assert got is not None and got.n > 0 and got.ncalled == 0


# ---- 3. the contract on synthetic BAMs ----------------------------------------------------------------------------

def write_bam_pe(path, records, refs=CONTIGS, block=4000):
    """helpers.write_bam with mate fields (mtid, mpos 1-based, isize) and small BGZF blocks (many windows)."""
    nt16 = {c: i for i, c in enumerate("=ACMGRSVTWYHKDBN")}
    body = bytearray(b"BAM\1")
    text = "@HD\tVN:1.0\tSO:queryname\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
    body += struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(refs))
    for name, ln in refs:
        body += struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<i", ln)
    for r in records:
        seq, n = r["seq"], len(r["seq"])
        qname = r["qname"].encode() + b"\0"
        cigar = r["cigar"]
        packed = bytearray((n + 1) // 2)
        for i, ch in enumerate(seq):
            packed[i >> 1] |= nt16[ch] << (4 if (i & 1) == 0 else 0)
        aux = b"".join(t.encode() + b"Z" + v.encode() + b"\0" for t, v in r["tags"].items())
        core = struct.pack("<iiBBHHHiiii", r["tid"], r["pos"] - 1, len(qname), r["mapq"], 4680, len(cigar), r["flag"], n,
                           r.get("mtid", -1), r.get("mpos", 0) - 1, r.get("isize", 0))
        rec = core + qname + b"".join(struct.pack("<I", (ln << 4) | op) for op, ln in cigar) + bytes(packed) + \
            bytes(r["qual"]) + aux
        body += struct.pack("<i", len(rec)) + rec

    def bgzf(data):
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        comp = co.compress(bytes(data)) + co.flush()
        return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(comp) + 25) + comp +
                struct.pack("<II", zlib.crc32(bytes(data)) & 0xFFFFFFFF, len(data)))

    with open(path, "wb") as f:
        for i in range(0, len(body), block):
            f.write(bgzf(body[i:i + block]))
        f.write(bgzf(b""))
    return path


def _span(cigar):
    return sum(ln for op, ln in cigar if op in (0, 2, 3, 7, 8))


def _finish(r, rng):
    r["mapq"] = rng.choice((0, 5, 20, 40, 60, 60))
    r["qual"] = bytes(rng.randint(2, 41) for _ in range(len(r["seq"])))
    return r


def synth_se(rng, tag, n):
    """Single-end: synth_records' reads (every CIGAR op, contig ends, unmapped / untagged / already-called records,
    two 10 kb reads) with single-end flags, duplicates among them."""
    recs = synth_records(rng, tag, n, long_reads=True)
    for r in recs:
        r["flag"] = (r.get("flag", 0) & 4) | rng.choice((0, 16, 0, 16, 1024))
        _finish(r, rng)
    return recs


def synth_pe(rng, tag, n):
    """Name-sorted paired-end templates: two mates on one contig with mate positions and template length, some mates
    unmapped, untagged or already called, some pairs not proper, duplicates, a 10 kb pair."""
    vals = {"XG": ("CT", "GA"), "YD": ("f", "r"), "ZS": ("++", "+-", "-+", "--")}[tag]
    recs = []
    for k in range(n):
        tid = rng.randrange(len(CONTIGS))
        clen = CONTIGS[tid][1]
        big = k == n // 2
        mates = []
        for m in range(2):
            pos = end_gap = None
            if k % 13 == 0 and m == 0:
                pos = k % 2
            elif k % 13 == 1 and m == 1:
                end_gap = (k // 13) % 2
            ln = 10000 if big else rng.randint(1, 60) if clen < 100 else rng.randint(20, 150)
            p, cigar, seq = random_read(rng, CONTIGS[0][1] if big else clen, ln, pos, end_gap)
            mates.append((p, cigar, seq))
        if big:
            tid = 0
        lo = min(mates[0][0], mates[1][0])
        hi = max(p + _span(c) for p, c, _ in mates)
        rev = rng.random() < 0.5
        dup = 1024 if rng.random() < 0.05 else 0
        proper = 2 if rng.random() < 0.95 else 0
        v = vals[k % len(vals)]
        for m, (p, cigar, seq) in enumerate(mates):
            other = mates[1 - m][0]
            flag = 1 | proper | (64 if m == 0 else 128) | dup | ((16 if m == 0 else 32) if rev else (32 if m == 0 else 16))
            isize = (hi - lo) if p <= other else -(hi - lo)
            r = {"qname": "t%06d" % k, "tid": tid, "pos": p, "cigar": cigar, "seq": seq, "flag": flag, "mtid": tid,
                 "mpos": other, "isize": isize, "tags": {tag: v, "NM": "0"}}
            u = (2 * k + m) % 29
            late = 2 * k + m >= 1100                                    # past the records that choose the strand tag
            if u == 5:
                r["flag"] |= 4
            elif u == 9:
                r["tags"]["XM"] = "".join(rng.choice("zZxXhH.") for _ in seq)
                if tag != "XG" and late:                               # already called: usable with its own XG
                    r["tags"]["XG"] = "CT" if rng.random() < 0.5 else "GA"
            elif u == 13:
                del r["tags"][tag]
            elif u == 17 and tag != "XG" and late:                      # called, keeping the XG it carries
                r["tags"]["XG"] = "GA" if rng.random() < 0.5 else "CT"
            recs.append(_finish(r, rng))
    return recs


SYNTH_GRID = [
    {"nthreads": 1},
    {"nthreads": 8, "window_kib": 16},
    {"nthreads": 8, "min_mapq": 20, "min_baseq": 25, "trim": (4, 1), "window_kib": 8},
    {"nthreads": 1, "skip_duplicates": True, "trim": 2, "window_kib": 8},
]


@pytest.mark.parametrize("tag", ["XG", "YD", "ZS"])
@pytest.mark.parametrize("layout", ["se", "pe"])
def test_contract_synthetic(tag, layout, synth_genome, tmp_path):
    rng = random.Random({"XG": 10, "YD": 20, "ZS": 30}[tag] + (layout == "pe"))
    recs = synth_se(rng, tag, 1500) if layout == "se" else synth_pe(rng, tag, 1200)
    assert {op for r in recs for op, _ in r["cigar"]} >= {0, 1, 2, 3, 4, 5, 6, 7, 8}
    src = write_bam_pe(str(tmp_path / "in.bam"), recs)
    with open(src, "rb") as f:
        assert f.read().count(b"\x1f\x8b\x08\x04") > 40                 # many BGZF blocks: many windows at 8-16 KiB
    for opts in SYNTH_GRID:
        got = check_contract(src, synth_genome, tmp_path, opts, call_threads=3)
        assert got is not None and got.n > 0
        assert got.paired == (layout == "pe")
        assert 0 < got.ncalled < got.nrecs == len(recs)


def test_contract_header_longer_than_a_window(tmp_path):
    """The header of 3000 reference sequences spans several one-block windows, for both sides of the contract."""
    _, g, src = many_contigs_input(tmp_path)
    got = check_contract(src, g, tmp_path, {"window_kib": 1})
    assert got is not None and got.n > 0 and not got.paired and len(got.levels) == 3000
    assert 0 < got.ncalled < got.nrecs == 200
    assert_same_templates(got, ea.preprocessBam(src, genome=g))


# ---- 4. errors -----------------------------------------------------------------------------------------------------

def _same_error(src, g, tmp_path, **opts):
    out = str(tmp_path / "called.bam")
    with pytest.raises(ValueError) as want:
        ea.callMethylation(src, out, g, verbose=False)
    assert not os.path.exists(out)
    before = sorted(os.listdir(tmp_path))
    with pytest.raises(ValueError) as got:
        ea.preprocessBam(src, genome=g, **opts)
    assert sorted(os.listdir(tmp_path)) == before
    assert str(got.value) == str(want.value)
    return str(got.value)


def test_error_fixtures(genome, tmp_path):
    assert "Empty file provided" in _same_error(os.path.join(BAMS, "empty.bam"), genome, tmp_path)
    assert "neither of XG/YD/ZS" in _same_error(os.path.join(BAMS, "bwameth-se-unsort.bam"), genome, tmp_path)
    assert "doesn't match the provided genome" in _same_error(os.path.join(BAMS, "amplicon000meth.bam"), genome, tmp_path)


def _good(k, tag="YD"):
    return {"seq": "ACGTCG" * 5, "pos": 100 + k, "tid": 0, "qname": "g%04d" % k, "tags": {tag: "f"}}


@pytest.mark.parametrize("what", ["past_end", "cigar_length", "cigar_op"])
def test_error_records(what, synth_genome, tmp_path):
    bad = {"past_end": {"seq": "ACGT" * 5, "pos": 700 - 10 + 1, "tid": 1},
           "cigar_length": {"seq": "ACGT" * 5, "pos": 10, "tid": 0, "cigar": [(0, 15)]},
           "cigar_op": {"seq": "ACGT" * 5, "pos": 10, "tid": 0, "cigar": [(0, 10), (10, 3), (0, 10)]}}[what]
    bad = dict(bad, qname="bad", tags={"YD": "r"}, mapq=0, flag=1024)
    msg = {"past_end": "past the end", "cigar_length": "CIGAR does not match", "cigar_op": "Unknown CIGAR operation"}[what]
    recs = [_good(k) for k in range(40)] + [bad] + [_good(k) for k in range(40, 60)]
    src = write_bam(str(tmp_path / "in.bam"), recs, refs=CONTIGS)
    assert msg in _same_error(src, synth_genome, tmp_path)
    # a record callMethylation rejects is an error even where the options would have dropped it
    assert msg in _same_error(src, synth_genome, tmp_path, min_mapq=30, skip_duplicates=True)


def test_error_mm_only(synth_genome, tmp_path):
    recs = [{"seq": "ACGCGTACGA" * 3, "pos": 50 + k, "tid": 0, "qname": "m%03d" % k, "flag": 0,
             "tags": {"MM": "C+m,0,1;", "ML": [200, 10]}} for k in range(30)]
    src = write_bam(str(tmp_path / "mm.bam"), recs, refs=CONTIGS)
    assert ea.preprocessBam(src).n > 0                              # a valid MM/ML input without a genome
    assert "neither of XG/YD/ZS" in _same_error(src, synth_genome, tmp_path)


# ---- 5. through the report functions ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["dragen-pe-namesort-xg.bam", "bwameth-se-unsort-yd.bam", "bsmap-pe-namesort-zs.bam"])
def test_reports_pass_through(name, genome, tmp_path):
    src = os.path.join(BAMS, name)
    called = str(tmp_path / "called.bam")
    ea.callMethylation(src, called, genome, verbose=False)
    for fn, kw in ((ea.generateCytosineReport, {}), (ea.generateCytosineReport, {"report_context": "CX"}),
                   (ea.generateMhlReport, {}), (ea.generateMhlReport, {"haplotype_context": "CHG"})):
        want = fn(called, **kw)
        got = fn(src, genome=genome, **kw)
        assert want.nrow > 0 and reports_equal(dict(want), dict(got)), (fn.__name__, kw)
    bed = str(tmp_path / "contigs.bed")
    with open(bed, "w") as f:
        for name_, ln in zip(genome.rname, genome.rlen):
            f.write("%s\t0\t%d\n" % (name_, int(ln)))
    want = ea.generateBedReport(called, bed)
    got = ea.generateBedReport(src, bed, genome=FASTA)
    assert reports_equal(dict(want), dict(got))
