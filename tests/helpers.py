"""Shared test helpers: fixture loading, simulateBam-equivalent template
construction, report comparison.  Test infrastructure only."""
import functools
import json
import os

import numpy as np

from oracle import bamio

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# R/internal.R:54-65 (.context.to.bases) -- kept separately from the product's
# copy (epialleler_amd.api.CONTEXT_TO_BASES); test_host_api checks they agree.
CONTEXT_TO_BASES = {
    "CG": dict(ctx_meth="Z", ctx_unmeth="z", ooctx_meth="XH", ooctx_unmeth="xh"),
    "CHG": dict(ctx_meth="X", ctx_unmeth="x", ooctx_meth="ZH", ooctx_unmeth="zh"),
    "CHH": dict(ctx_meth="H", ctx_unmeth="h", ooctx_meth="ZX", ooctx_unmeth="zx"),
    "CxG": dict(ctx_meth="ZX", ctx_unmeth="zx", ooctx_meth="H", ooctx_unmeth="h"),
    "CX": dict(ctx_meth="ZXH", ctx_unmeth="zxh", ooctx_meth="", ooctx_unmeth=""),
}


@functools.lru_cache(maxsize=None)
def expected():
    with open(os.path.join(GOLDEN, "expected.json")) as f:
        return json.load(f)


def expected_values(section, expr_prefix, nth=0):
    """n-th known-answer value in `section` whose R expression starts with `expr_prefix`."""
    hits = [b["value"] for b in expected()[section] if b["expr"].startswith(expr_prefix)]
    return hits[nth]


@functools.lru_cache(maxsize=None)
def load_bam(name, **kw):
    """preprocessBam() on a reference BAM fixture (cached).  kw as hashable items."""
    return bamio.preprocess_bam(os.path.join(GOLDEN, "bam", name), **dict(kw))


def bam(name, **kw):
    return load_bam(name, **{k: v for k, v in sorted(kw.items())})


def ctx_to_idx(ch):
    return ((ord(ch) + 2) >> 2) & 15


def templates_from_xm(xm_strings, starts, strands, rnames=None, seq_code=1):
    """Packed templates a single-end simulateBam() BAM would yield
    (flag 0, cigar <n>M, qual 'F', see R/internal.R:296-398 defaults):
    one byte per base, (nt16<<4)|ctx_to_idx(XM char); rows sorted by (rname,start), stable."""
    n = len(xm_strings)
    rnames = [1] * n if rnames is None else list(rnames)
    order = sorted(range(n), key=lambda i: (rnames[i], starts[i], i))
    chunks = [np.frombuffer(xm_strings[i].encode("latin1"), np.uint8) for i in order]
    xm = (np.concatenate(chunks) if chunks else np.zeros(0, np.uint8)).astype(np.int64)
    packed = ((seq_code << 4) | (((xm + 2) >> 2) & 15)).astype(np.uint8)
    off = np.zeros(n + 1, np.int64)
    np.cumsum([c.size for c in chunks], out=off[1:])
    return {"xm": packed, "off": off,
            "rname": np.asarray([rnames[i] for i in order], np.int32),
            "strand": np.asarray([strands[i] for i in order], np.int32),
            "start": np.asarray([starts[i] for i in order], np.int32)}


def group_sums(rep, value, ctx_code=None):
    """sum(value) by (rname,strand) in (rname,strand) order, like the R tests'
    `[, sum(v), by=.(rname,strand,context)][order(rname,strand,context)]` for one context."""
    m = np.ones(rep["pos"].size, bool) if ctx_code is None else rep["context"] == ctx_code
    key = rep["rname"][m].astype(np.int64) * 4 + rep["strand"][m]
    v = (rep[value][m] if isinstance(value, str) else value[m]).astype(np.float64)
    out = []
    for k in np.unique(key):
        out.append(v[key == k].sum())
    return out


def group_sums_all_ctx(rep, value):
    """by=.(rname,strand,context) ordered by (rname,strand,context factor level = code)."""
    key = (rep["rname"].astype(np.int64) * 4 + rep["strand"]) * 16 + rep["context"]
    v = rep[value].astype(np.float64)
    return [v[key == k].sum() for k in np.unique(key)]


def match_amplicon(b, bed_rows, tolerance=1):
    """src/rcpp_match_target.cpp:16-45; bed_rows = [(rname_idx, start, end)], returns 1-based index or 0 for NA."""
    lens = np.diff(b["off"])
    res = np.zeros(b["start"].size, np.int64)
    for x in range(res.size):
        rs = int(b["start"][x])
        re_ = rs + int(lens[x]) - 1
        for i, (c, s, e) in enumerate(bed_rows):
            if b["rname"][x] == c and (abs(rs - s) <= tolerance or abs(re_ - e) <= tolerance):
                res[x] = i + 1
                break
    return res


def read_bed(name, levels):
    rows = []
    with open(os.path.join(GOLDEN, "bam", name)) as f:
        for ln in f:
            p = ln.split()
            if not p or p[0] in ("chr", "#chr") or not p[1].isdigit():
                continue
            rows.append((levels.index(p[0]) + 1, int(p[1]), int(p[2])))
    return rows


def assert_reports_equal(a, b, float_cols=()):
    assert set(a.keys()) == set(b.keys())
    for k in a:
        assert a[k].shape == b[k].shape, (k, a[k].shape, b[k].shape)
        if k in float_cols:
            # bit-exact including NaN positions
            assert np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)) or \
                np.array_equal(a[k], b[k], equal_nan=True), k
        else:
            assert np.array_equal(a[k], b[k]), k


# ---- a minimal BAM writer for the tests (what the reference's simulateBam() gives its long-read tests) ----------

def write_bam(path, records, refs=(("chrS", 1000),)):
    """records: dicts with seq (str), flag, pos (1-based), optional qname, mapq, cigar [(op, len)], qual (bytes or int),
    tid, tags {name: str (Z) | list of ints (B:C)}.  Defaults follow R/internal.R:296-398: mapq 60, cigar <len>M,
    quality 'F'."""
    import struct
    import zlib
    nt16 = {c: i for i, c in enumerate("=ACMGRSVTWYHKDBN")}
    body = bytearray(b"BAM\1")
    text = "@HD\tVN:1.0\tSO:unknown\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
    body += struct.pack("<i", len(text)) + text.encode()
    body += struct.pack("<i", len(refs))
    for name, ln in refs:
        body += struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<i", ln)
    for k, r in enumerate(records):
        seq = r["seq"]
        n = len(seq)
        qname = (r.get("qname") or ("q%06d" % k)).encode() + b"\0"
        cigar = r.get("cigar") or [(0, n)]
        qual = r.get("qual", 37)
        qual = bytes([qual]) * n if isinstance(qual, int) else bytes(qual)
        packed = bytearray((n + 1) // 2)
        for i, ch in enumerate(seq):
            packed[i >> 1] |= nt16[ch] << (4 if (i & 1) == 0 else 0)
        aux = bytearray()
        for tag, val in (r.get("tags") or {}).items():
            if isinstance(val, str):
                aux += tag.encode() + b"Z" + val.encode() + b"\0"
            else:
                aux += tag.encode() + b"BC" + struct.pack("<i", len(val)) + bytes(val)
        core = struct.pack("<iiBBHHHiiii", r.get("tid", 0), r["pos"] - 1, len(qname), r.get("mapq", 60), 4680, len(cigar),
                           r.get("flag", 0), n, -1, -1, 0)
        rec = core + qname + b"".join(struct.pack("<I", (ln << 4) | op) for op, ln in cigar) + bytes(packed) + qual + bytes(aux)
        body += struct.pack("<i", len(rec)) + rec

    def block(data):
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        comp = co.compress(bytes(data)) + co.flush()
        return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(comp) + 25) + comp +
                struct.pack("<II", zlib.crc32(bytes(data)) & 0xFFFFFFFF, len(data)))

    with open(path, "wb") as f:
        for i in range(0, len(body), 60000):
            f.write(block(body[i:i + 60000]))
        f.write(block(b""))
    return path


def dirty_allocator(bam):
    """Leaves a freed block of non-zero int32s of the batch's row count in torch's caching allocator, so that the next
    torch.empty of that size (the `pass` column of cytosine_report_fused) starts out as garbage, not as zeros."""
    import torch
    junk = torch.full((max(bam.n, 1),), 0x5A5A5A5A, dtype=torch.int32, device="cuda:%d" % (bam.device or 0))
    del junk


# ---- plain restatements of the per-read decisions (numpy, float64), independent of the oracle and of the kernels -------

def class_counts(xm, off, letters):
    """Per row: sum over the letters of a class string of the count of that letter's context index in the row (a repeated
    letter counts twice, as in rcpp_threshold_reads.cpp:39-47)."""
    xm = np.asarray(xm, np.uint8)
    off = np.asarray(off, np.int64)
    n = off.size - 1
    lens = np.diff(off)
    row = np.repeat(np.arange(n, dtype=np.int64), lens)
    hist = np.bincount(row * 16 + (xm[:int(off[-1])] & 15), minlength=16 * n).reshape(n, 16).astype(np.int64)
    out = np.zeros(n, np.int64)
    for ch in letters:
        out += hist[:, ctx_to_idx(ch)]
    return out


def threshold_np(xm, off, cls4, min_n, min_beta, max_oo):
    """rcpp_threshold_reads.cpp:43-70: a read passes when it has a methylated context base, at least min_n context bases
    (unsigned compare), !(n_m / n_all < min_beta), and no out-of-context base or !(o_m / o_all > max_oo) -- divisions and
    comparisons in float64, so NaN thresholds compare false as they do there.  cls4 = (ctx_meth, ctx_unmeth, ooctx_meth,
    ooctx_unmeth)."""
    n_m, n_u, o_m, o_u = (class_counts(xm, off, c) for c in cls4)
    n_all = n_m + n_u
    with np.errstate(invalid="ignore", divide="ignore"):
        frac = n_m.astype(np.float64) / n_all.astype(np.float64)
        ofrac = o_m.astype(np.float64) / (o_m + o_u).astype(np.float64)
    ok = (n_m != 0) & ~(n_all < (int(min_n) & 0xFFFFFFFF)) & ~(frac < np.float64(min_beta))
    ok &= ~((o_m > 0) & (ofrac > np.float64(max_oo)))
    return ok.astype(np.int32)


def mhl_keep_np(xm, off, ctx, hmin, max_oo):
    """The read filter of rcpp_mhl_report.cpp:160-179: h = the read's bases whose context index is one of ctx's letters;
    out-of-context methylated codes 2,5,6,7 and unmethylated 10,13,14,15 (only those not in ctx);
    keep = !((int)h < hmin || o_m / (o_m + o_u) > max_oo), with 0 / 0 = NaN (kept)."""
    xm = np.asarray(xm, np.uint8)
    off = np.asarray(off, np.int64)
    n = off.size - 1
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))
    hist = np.bincount(row * 16 + (xm[:int(off[-1])] & 15), minlength=16 * n).reshape(n, 16).astype(np.int64)
    in_ctx = np.zeros(16, bool)
    in_ctx[[ctx_to_idx(c) for c in ctx]] = True
    h = hist[:, in_ctx].sum(axis=1)
    o_m = hist[:, [i for i in (2, 5, 6, 7) if not in_ctx[i]]].sum(axis=1)
    o_u = hist[:, [i for i in (10, 13, 14, 15) if not in_ctx[i]]].sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        frac = o_m.astype(np.float64) / (o_m + o_u).astype(np.float64)
    return ~((h < int(hmin)) | (frac > np.float64(max_oo)))


def subset(t, keep):
    """The templates of t whose keep flag is set (same order)."""
    keep = np.asarray(keep, bool)
    lens = np.diff(t["off"])
    out = {k: t[k][keep] for k in ("rname", "strand", "start")}
    out["xm"] = t["xm"][:int(t["off"][-1])][np.repeat(keep, lens)]
    out["off"] = np.concatenate(([0], np.cumsum(lens[keep]))).astype(np.int64)
    return out


# (n_m, n_all) and (o_m, o_all) exactly at the thresholds the tests use, one call below and one above: 3/10 at 0.3,
# 1/3 at 1/3, 9/10 at 0.9, 1/2 at 0.5, 1/10 at 0.1, all at 1.0 and none at 0.0
TIE_FRACS = ((3, 10), (6, 20), (1, 3), (5, 15), (33, 99), (9, 10), (27, 30), (1, 2), (5, 10), (1, 1), (4, 4), (1, 10), (3, 30), (7, 70))


def tie_batch(seed=0):
    """Templates whose context / out-of-context fractions sit exactly on, one call below and one call above the threshold
    values of the test grids, under CG (Z/z, out of context X,H/x,h) and under CHG (X/x, out of context Z,H/z,h)
    thresholding; with n_m = 0 < n_u, o_m = 0 < o_u, n_all = 2 and 3, rows without calls and empty rows."""
    rng = np.random.default_rng(seed)
    npat = {(0, 0), (0, 3), (1, 2), (2, 2), (0, 2), (2, 3), (1, 3)}
    for m, a in TIE_FRACS:
        npat.update({(m, a), (max(m - 1, 0), a), (min(m + 1, a), a)})
    opat = {(0, 0), (0, 5), (1, 1), (1, 10), (0, 10), (2, 10), (3, 30), (2, 30), (4, 30), (7, 70), (6, 70), (8, 70), (5, 5)}
    xms = []
    for meth, unmeth, om, ou in (("Z", "z", "X", "x"), ("X", "x", "Z", "z")):
        for nm, na in sorted(npat):
            for o_m, o_a in sorted(opat):
                s = list(meth * nm + unmeth * (na - nm) + om * o_m + ou * (o_a - o_m) + "." * int(rng.integers(0, 12)))
                rng.shuffle(s)
                xms.append("".join(s))
    xms += ["", "....", "", "-.+", ""]
    n = len(xms)
    order = rng.permutation(n)
    xms = [xms[i] for i in order]
    return templates_from_xm(xms, [int(v) for v in rng.integers(1, 30000, n)], [int(v) for v in rng.integers(1, 3, n)],
                             rnames=[int(v) for v in rng.integers(1, 3, n)])


# (min_n, min_beta, max_oo) at ties, limits and odd values: NaN, negative, above 1, -0.0, min_n above every count
THRESHOLD_GRID = ((0, 0.0, 1.0), (1, 0.3, 0.0), (3, 1.0, 0.1), (2, 1 / 3, 0.1), (5, 0.9, 0.0), (2, float("nan"), float("nan")),
                  (2, -0.5, 1.5), (70000, 0.5, 0.1), (2, -0.0, -0.0))


def cls4(ctx):
    c = CONTEXT_TO_BASES[ctx]
    return c["ctx_meth"], c["ctx_unmeth"], c["ooctx_meth"], c["ooctx_unmeth"]


# ---- plain restatements of the BED path (numpy, int64 / float64), independent of the kernel and of bed.py ---------------

NA_INT = -2 ** 31


def _bed_hits(t, bed, capture, param, lo, hi):
    """(hi - lo) x nbed boolean matrix: does read x fit BED row i (src/rcpp_match_target.cpp:34-38 / :70-73), in int64."""
    b_chr, b_s, b_e = (np.asarray(a, np.int64)[None, :] for a in bed)
    rs = np.asarray(t["start"][lo:hi], np.int64)[:, None]
    re_ = rs + np.diff(t["off"])[lo:hi].astype(np.int64)[:, None] - 1          # read_end = start + len - 1
    same = np.asarray(t["rname"][lo:hi], np.int64)[:, None] == b_chr
    if capture:
        return same & (np.minimum(re_, b_e) - np.maximum(rs, b_s) + 1 >= int(param))
    return same & ((np.abs(rs - b_s) <= int(param)) | (np.abs(re_ - b_e) <= int(param)))


def match_target_np(t, bed, capture, param, block=256, with_nfit=False):
    """rcpp_match_amplicon / rcpp_match_capture: the 1-based number of the FIRST BED row a read fits, or NA_INT.  bed =
    (rname code, start, end) integer arrays, NA_INT for an NA chromosome (it equals no rname).  Blocks of reads against
    all BED rows: a hit matrix, argmax of the first hit.  with_nfit: also the number of rows every read fits."""
    n, nbed = len(t["start"]), len(bed[0])
    res = np.full(n, NA_INT, np.int32)
    nfit = np.zeros(n, np.int64)
    if nbed:
        for lo in range(0, n, block):
            hit = _bed_hits(t, bed, capture, param, lo, min(lo + block, n))
            nfit[lo:lo + block] = hit.sum(axis=1)
            res[lo:lo + block] = np.where(hit.any(axis=1), hit.argmax(axis=1) + 1, NA_INT)
    return (res, nfit) if with_nfit else res


def match_target_loop(t, bed, capture, param, rows=None):
    """The same as the two nested loops of the reference, for a few hundred reads (rows: which ones, default all)."""
    lens = np.diff(t["off"])
    bed_rows = [(int(c), int(s), int(e)) for c, s, e in zip(*bed)]
    rows = range(len(t["start"])) if rows is None else rows
    res = []
    for x in rows:
        rs = int(t["start"][x])
        re_ = rs + int(lens[x]) - 1
        r = NA_INT
        for i, (c, s, e) in enumerate(bed_rows):
            if int(t["rname"][x]) != c:
                continue
            if (min(re_, e) - max(rs, s) + 1 >= param) if capture else (abs(rs - s) <= param or abs(re_ - e) <= param):
                r = i + 1
                break
        res.append(r)
    return np.asarray(res, np.int32)


def bed_report_np(t, pass_, match, nbed):
    """.getBedReport (R/internal.R:529-561) per BED row plus the NA slot (index nbed) of the unmatched reads: reads on
    strand 1 / strand 2 and VEF = passing / all, float64, NaN for a slot without a read on either strand (the NA that
    merge(all=TRUE) leaves).  A strand-0 row (the placeholder template) is counted nowhere.  has_na: the NA row exists."""
    strand = np.asarray(t["strand"])
    match = np.asarray(match, np.int64)
    pass_ = np.asarray(pass_) != 0
    slot = np.where(match < 0, nbed, match - 1)
    npl = np.zeros(nbed + 1)
    nmi = np.zeros(nbed + 1)
    npass = np.zeros(nbed + 1)
    for x in range(strand.size):
        if strand[x] == 1:
            npl[slot[x]] += 1
        elif strand[x] == 2:
            nmi[slot[x]] += 1
        else:
            continue
        npass[slot[x]] += bool(pass_[x])
    seen = (npl + nmi) > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        vef = npass / (npl + nmi)
    nan = lambda a: np.where(seen, a, np.nan)
    return {"nreads+": nan(npl), "nreads-": nan(nmi), "VEF": nan(vef), "has_na": bool(seen[nbed])}


def ecdf_np(x, q):
    """stats::ecdf(x)(q): the share of x that is <= q, for every q."""
    x = np.asarray(x, np.float64)
    return np.asarray([np.count_nonzero(x <= v) / x.size for v in np.atleast_1d(np.asarray(q, np.float64))])


def beta_np(xm, off, meth, unmeth):
    """src/rcpp_get_xm_beta.cpp:37-39: n_meth / max(n_meth + n_unmeth, 1) per read, float64."""
    n_m, n_u = class_counts(xm, off, meth), class_counts(xm, off, unmeth)
    return n_m.astype(np.float64) / np.maximum(n_m + n_u, 1).astype(np.float64)


# ---- the synthetic batch and BED of the BED-path tests (fixed seed; treat what these return as read-only) --------------

MATCH_LEVELS = ("c1", "c2", "c3")
MATCH_AMPLICON = (-1, 0, 1, 2, 5, 1000)                  # match.tolerance: nothing, exact, ..., everything on the chromosome
MATCH_CAPTURE = (-50, 0, 1, 2, 30, 150, 400)             # match.min.overlap: within a gap, touching, ..., longer than any read
MATCH_INTERIOR = {False: (0, 1, 2, 5), True: (0, 1, 2, 30, 150)}


@functools.lru_cache(maxsize=None)
def match_templates(seed=20240611):
    """3001 ragged templates (empty ones among them) on three rnames, about 1 % with the placeholder's strand code 0."""
    import synth_np
    rng = np.random.default_rng(seed)
    t = synth_np.random_templates(rng, 3001, 0, 300, 3, 60000)
    t["strand"][rng.random(3001) < 0.01] = 0
    return t


@functools.lru_cache(maxsize=None)
def match_bed(seed=20240611, nbed=2500):
    """An unsorted BED of 2500 rows as (chromosome names, codes, start, end): chromosomes c1..c3, c4 (no read is on it)
    and one that is not among the levels at all (code NA); end - start in -5..120; 600 rows are a read's own range
    moved by -3..+3 at either end; 100 rows are copies of other rows."""
    t = match_templates(seed)
    rng = np.random.default_rng(seed + 1)
    n = len(t["start"])
    code = rng.choice(np.asarray([1, 2, 3, 4, NA_INT], np.int64), size=nbed, p=[0.3, 0.3, 0.3, 0.05, 0.05])
    start = rng.integers(1, 60001, size=nbed).astype(np.int64)
    end = start + rng.integers(-5, 121, size=nbed)
    rows = rng.choice(nbed, size=600, replace=False)
    reads = rng.choice(n, size=600, replace=False)
    code[rows] = t["rname"][reads]
    start[rows] = t["start"][reads].astype(np.int64) + rng.integers(-3, 4, size=600)
    end[rows] = t["start"][reads].astype(np.int64) + np.diff(t["off"])[reads] - 1 + rng.integers(-3, 4, size=600)
    dst = rng.choice(nbed, size=100, replace=False)
    src = rng.integers(0, nbed, size=100)
    code[dst], start[dst], end[dst] = code[src], start[src], end[src]
    names = ["chrUn" if c == NA_INT else "c%d" % c for c in code]
    return names, code, start, end


def match_codes(names, levels=MATCH_LEVELS):
    """factor(seqnames, levels=levels(rname)) as integer codes: NA_INT for a chromosome that is not a level."""
    return np.asarray([levels.index(c) + 1 if c in levels else NA_INT for c in names], np.int64)


@functools.lru_cache(maxsize=None)
def match_want(capture, param, nbed=2500):
    """(first fitting row, number of fitting rows) of every template against the first nbed rows of match_bed()."""
    names, _, start, end = match_bed()
    return match_target_np(match_templates(), (match_codes(names)[:nbed], start[:nbed], end[:nbed]), capture, param, with_nfit=True)


def assert_match_design():
    """What the synthetic case must give under the restatement alone, or it tests less than it says: at every interior
    parameter some reads match and some do not, first matches fall into each of the kernel's three LDS chunks of 1024
    rows, and at least 50 reads fit several rows (so that 'first' differs from 'any')."""
    for capture in (False, True):
        for param in MATCH_INTERIOR[capture]:
            want, nfit = match_want(capture, param)
            share = np.mean(want > 0)
            assert 0 < share < 1, (capture, param, share)
            for lo, hi in ((1, 1024), (1025, 2048), (2049, 2500)):
                assert np.any((want >= lo) & (want <= hi)), (capture, param, lo)
            multi = nfit > 1
            if capture or param > 0:                       # (an exact start or end shared by several rows is rare)
                assert np.count_nonzero(multi) >= 50, (capture, param, np.count_nonzero(multi))
            assert np.all(want[multi] > 0)
