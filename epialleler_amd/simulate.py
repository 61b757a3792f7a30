"""simulateBam: BAM files with known content, from a few columns.  Mirrors R/simulateBam.R and .simulateBam
(R/internal.R:296-403), which prepare the table, and rcpp_simulate_bam (src/rcpp_simulate_bam.cpp), which writes it with
HTSlib.  Here the table's rules are restated in Python; the records are assembled on the GPU (epi_simulate_bam:
k_sim_size, k_sim_write) from the columns at their own lengths, and deflated by the library's BGZF writer.

Where this differs from R, on purpose:
  * Python types choose the tag group: ints (and bools, numpy integers) are integer tags, floats are float tags, str are
    string tags, a list of sequences is an array tag.  In R `NM=c(1,2)` is a double and becomes an 'f' tag; here
    `NM=[1, 2]` is an integer tag.
  * Random bases are a fixed function of `seed` (see _random_seq), so a call can be repeated.
  * Every record is checked before the file is opened: an invalid call leaves no partial file.  A `qual` of another length
    than its `seq` is an error (the reference reads past the string).  Integer values must fit int32, flag 0..65535 and
    mapq 0..255.
  * The CIGAR of each record has its own number of ops (rcpp_simulate_bam passes the largest count parsed so far).
"""
import ctypes as C
import os
import sys
import time

import numpy as np

from . import _lib
from ._lib import SimColumn
from .api import Report

VERSION = "1.13.4"          # the @PG line's VN: the version of epialleleR whose functions this package mirrors
SEQ_STREAM = 0x53494D       # hash3 stream of the random bases
FIELDS = ("qname", "flag", "tid", "pos", "mapq", "cigar", "mtid", "mpos", "isize", "seq", "qual")
SIM_NONE, SIM_I32, SIM_F32, SIM_STR, SIM_ARR, SIM_RANDOM = range(6)
_I32_MIN, _I32_MAX = -(1 << 31), (1 << 31) - 1


def _mix64(z):
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def hash3(seed, stream, idx):
    """synth.hip's hash3 (splitmix64's finaliser twice), on uint64 arrays."""
    with np.errstate(over="ignore"):
        s = _mix64(np.uint64(seed) + np.uint64(stream) * np.uint64(0xD1B54A32D192ED03))
        return _mix64(s ^ np.asarray(idx, dtype=np.uint64))


def _random_seq(seed, j, n):
    """Random string j of length n: base k is "ACTG"[hash3(seed, 0x53494D, (j << 32) | k) >> 62]."""
    k = np.arange(n, dtype=np.uint64) | (np.uint64(j) << np.uint64(32))
    return np.frombuffer(b"ACTG", dtype=np.uint8)[(hash3(seed, SEQ_STREAM, k) >> np.uint64(62)).astype(np.intp)].tobytes().decode()


def _vec(x):
    """An argument as a vector (R: every value is one): a scalar or a string is a vector of one."""
    if isinstance(x, (str, bytes)) or np.isscalar(x):
        return [x.decode() if isinstance(x, bytes) else x]
    if isinstance(x, np.ndarray):
        return x.reshape(-1).tolist() if x.dtype.kind in "OUS" else x.reshape(-1)
    return list(x)


def _is_int(v):
    return isinstance(v, (bool, int, np.integer, np.bool_))


def _is_num(v):
    return _is_int(v) or isinstance(v, (float, np.floating))


def _is_seq(v):
    return isinstance(v, (list, tuple, np.ndarray))


def _ints(name, x, lo=_I32_MIN, hi=_I32_MAX):
    if isinstance(x, np.ndarray) and x.dtype.kind in "iub":
        a = x.astype(np.int64)
    else:
        if not all(_is_num(v) for v in x) or any(isinstance(v, (float, np.floating)) and v != int(v) for v in x):
            raise ValueError("%s must hold whole numbers" % name)
        a = np.array([int(v) for v in x], dtype=np.int64)
    if a.size and (a.min() < lo or a.max() > hi):
        raise ValueError("%s must lie in [%d, %d]" % (name, lo, hi))
    return a


def _strs(name, x):
    if not all(isinstance(v, (str, bytes)) for v in x):
        raise ValueError("%s must hold strings" % name)
    return [v.decode() if isinstance(v, bytes) else v for v in x]


def array_subtype(values):
    """The subtype of an array tag from all its values (R/internal.R:360-386): 'f' if any is a float, else by the
    integer range c C s S i I.  Non-numeric values are an error."""
    if not all(_is_num(v) for v in values):
        raise ValueError("BAM file format does not support non-numeric arrays")
    if any(isinstance(v, (float, np.floating)) for v in values):
        return "f"
    if not values:
        return "C"                                    # R: min(integer(0)) is Inf, max is -Inf
    mn, mx = min(int(v) for v in values), max(int(v) for v in values)
    if mn < 0 and mn > -2 ** 7 and mx < 2 ** 7:
        return "c"
    if mn >= 0 and mx < 2 ** 8:
        return "C"
    if mn < 0 and mn > -2 ** 15 and mx < 2 ** 15:
        return "s"
    if mn >= 0 and mx < 2 ** 16:
        return "S"
    return "i" if mn < 0 else "I"


def _tag_column(name, value):
    """(group, values): group 'i', 'f', 's' or 'a' and the column at its own length."""
    if len(name) != 2:
        raise ValueError("tag names have two characters: %r" % name)
    if isinstance(value, np.ndarray) and value.ndim == 1 and value.dtype.kind in "iub":
        return "i", _ints(name, value)
    if isinstance(value, np.ndarray) and value.ndim == 1 and value.dtype.kind == "f":
        return "f", value.astype(np.float64)
    v = _vec(value)
    if isinstance(v, np.ndarray):
        v = v.tolist()
    if len(v) == 0:
        raise ValueError("tag %s has no values" % name)
    if all(_is_seq(e) for e in v):
        arrs = [list(np.asarray(e).reshape(-1).tolist()) if isinstance(e, np.ndarray) else list(e) for e in v]
        sub = array_subtype([x for a in arrs for x in a])
        if sub != "f":
            for a in arrs:
                _ints(name, a)
        return "a", (arrs, sub)
    if all(isinstance(e, (str, bytes)) for e in v):
        return "s", _strs(name, v)
    if all(_is_int(e) for e in v):
        return "i", _ints(name, v)
    if all(_is_num(e) for e in v):
        return "f", np.array([float(e) for e in v], dtype=np.float64)
    raise ValueError("tag %s mixes types that a BAM tag cannot hold together" % name)


def _levels_codes(x):
    lv = sorted(set(x))                               # factor(): levels in code-point order
    idx = {s: k for k, s in enumerate(lv)}
    return lv, np.array([idx[s] for s in x], dtype=np.int64)


def _prepare(qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual, tags, seed, supplied):
    """.simulateBam's table, every column at its own length (record i takes element i % len; tag columns
    (i % M_group) % len)."""
    nrecs = max([1] + [len(_vec(v)) for v in supplied] + [len(_vec(v)) for v in tags.values()])
    t = {}
    t["qname"] = None if qname is None else _strs("qname", _vec(qname))
    t["flag"] = np.zeros(1, np.int64) if flag is None else _ints("flag", _vec(flag), 0, 65535)
    rlv, t["tid"] = _levels_codes(["chrS"] if rname is None else _strs("rname", _vec(rname)))
    t["pos"] = (np.ones(1, np.int64) if pos is None else _ints("pos", _vec(pos), _I32_MIN + 1, _I32_MAX + 1)) - 1
    t["mapq"] = np.full(1, 60, np.int64) if mapq is None else _ints("mapq", _vec(mapq), 0, 255)
    groups = {"i": [], "f": [], "s": [], "a": []}
    for name, value in tags.items():
        g, col = _tag_column(name, value)
        groups[g].append((name, col))
    nbases = None
    if seq is None:
        if "XM" in tags:
            xm = _vec(tags["XM"])
            nbases = np.array([len(s) for s in _strs("XM", xm)], dtype=np.int64)
        elif tlen is not None:
            nbases = _ints("tlen", _vec(tlen))
            if nbases.min() < 0:
                raise ValueError("tlen must not be negative when it sets the length of random bases")
        else:
            nbases = np.array([10], dtype=np.int64)
        t["seq"] = None
    else:
        t["seq"] = _strs("seq", _vec(seq))
    t["cigar"] = None if cigar is None else _strs("cigar", _vec(cigar))
    rnlv, t["mtid"] = _levels_codes(["chrS"] if rnext is None else _strs("rnext", _vec(rnext)))
    t["mpos"] = (np.ones(1, np.int64) if pnext is None else _ints("pnext", _vec(pnext), _I32_MIN + 1, _I32_MAX + 1)) - 1
    t["isize"] = None if tlen is None else _ints("tlen", _vec(tlen))
    t["qual"] = None if qual is None else _strs("qual", _vec(qual))
    seq_len = nbases if t["seq"] is None else np.array([len(s.encode()) for s in t["seq"]], dtype=np.int64)
    max_tlen = int(t["isize"].max()) if t["isize"] is not None else int(seq_len.max())
    ln = int(max(t["pos"].max(), t["mpos"].max())) + 1 + max_tlen - 1
    header = ["@SQ\tSN:%s\tLN:%d" % (lv, ln) for lv in rlv] + \
             ["@PG\tID:epialleleR\tPN:epialleleR\tVN:%s\tCL:rcpp_simulate_bam()" % VERSION]
    return dict(nrecs=nrecs, t=t, nbases=nbases, seq_len=seq_len, groups=groups, header=header, rname_levels=rlv,
                rnext_levels=rnlv, seed=seed)


def _table(p):
    """The prepared table recycled to nrecs: what .simulateBam returns without an output file."""
    n, t = p["nrecs"], p["t"]
    i = np.arange(n)
    rec = lambda a: np.asarray(a)[i % len(a)]
    strs = lambda xs: np.array(xs, dtype=object)
    if t["seq"] is None:
        rnd = [_random_seq(p["seed"], j, int(nb)) for j, nb in enumerate(p["nbases"])]
        seq = strs([rnd[k % len(rnd)] for k in range(n)])
    else:
        seq = strs([t["seq"][k % len(t["seq"])] for k in range(n)])
    ls = np.array([len(s.encode()) for s in seq], dtype=np.int64)
    cols = {
        "qname": strs(["q%04d" % (k + 1) for k in range(n)]) if t["qname"] is None else strs([t["qname"][k % len(t["qname"])] for k in range(n)]),
        "flag": rec(t["flag"]).astype(np.int32), "tid": rec(t["tid"]).astype(np.int32), "pos": rec(t["pos"]),
        "mapq": rec(t["mapq"]).astype(np.int32),
        "cigar": strs(["%dM" % l for l in ls]) if t["cigar"] is None else strs([t["cigar"][k % len(t["cigar"])] for k in range(n)]),
        "mtid": rec(t["mtid"]).astype(np.int32), "mpos": rec(t["mpos"]),
        "isize": ls.copy() if t["isize"] is None else rec(t["isize"]),
        "seq": seq,
        "qual": strs(["F" * l for l in ls]) if t["qual"] is None else strs([t["qual"][k % len(t["qual"])] for k in range(n)]),
    }
    for g in "ifsa":
        cs = p["groups"][g]
        if not cs:
            continue
        m = max(len(c[0]) if g == "a" else len(c) for _, c in cs)
        for name, c in cs:
            vals = c[0] if g == "a" else c
            idx = (i % m) % len(vals)
            if g in "sa":
                cols[name] = strs([vals[k] for k in idx])
            else:
                cols[name] = np.asarray(vals)[idx]
    rep = Report(cols, p["rname_levels"])
    rep.levels["rnext"] = tuple(p["rnext_levels"])
    rep.array_types = {name: c[1] for name, c in p["groups"]["a"]}
    return rep


def _columns(p):
    """epi_sim_column structs of the prepared table (and the numpy buffers they point into)."""
    keep = []
    n = p["nrecs"]

    def col(kind, values=None, offsets=None, length=0, period=1, name=None, typ=b"\0"):
        c = SimColumn()
        c.name = name.encode() if name else None
        c.kind, c.type, c.len, c.period = kind, typ, length, period
        if values is not None:
            keep.append(values)
            c.values = values.ctypes.data
        if offsets is not None:
            keep.append(offsets)
            c.offsets = offsets.ctypes.data
        return c

    def i32(a, period, name=None):
        a = np.ascontiguousarray(a, dtype=np.int32)
        return col(SIM_I32, a, None, a.size, period, name)

    def strcol(xs, period, name=None):
        bs = [s.encode() for s in xs]
        off = np.zeros(len(bs) + 1, np.int64)
        off[1:] = np.cumsum([len(b) for b in bs])
        data = np.frombuffer(b"".join(bs) + b"\0", dtype=np.uint8).copy()
        return col(SIM_STR, data, off, len(bs), period, name)

    t = p["t"]
    f = [None] * len(FIELDS)
    f[0] = col(SIM_NONE, period=n) if t["qname"] is None else strcol(t["qname"], n)
    f[1], f[2], f[3], f[4] = i32(t["flag"], n), i32(t["tid"], n), i32(t["pos"], n), i32(t["mapq"], n)
    f[5] = col(SIM_NONE, period=n) if t["cigar"] is None else strcol(t["cigar"], n)
    f[6], f[7] = i32(t["mtid"], n), i32(t["mpos"], n)
    f[8] = col(SIM_NONE, period=n) if t["isize"] is None else i32(t["isize"], n)
    if t["seq"] is None:
        nb = np.ascontiguousarray(p["nbases"], dtype=np.int32)
        f[9] = col(SIM_RANDOM, nb, None, nb.size, n)
    else:
        f[9] = strcol(t["seq"], n)
    f[10] = col(SIM_NONE, period=n) if t["qual"] is None else strcol(t["qual"], n)
    tags = []
    for g in "ifsa":
        cs = p["groups"][g]
        if not cs:
            continue
        m = max(len(c[0]) if g == "a" else len(c) for _, c in cs)
        for name, c in cs:
            if g == "i":
                tags.append(i32(c, m, name))
            elif g == "f":
                a = np.ascontiguousarray(c, dtype=np.float32)
                tags.append(col(SIM_F32, a, None, a.size, m, name))
            elif g == "s":
                tags.append(strcol(c, m, name))
            else:
                arrs, sub = c
                off = np.zeros(len(arrs) + 1, np.int64)
                off[1:] = np.cumsum([len(a) for a in arrs])
                flat = [x for a in arrs for x in a]
                vals = np.array(flat + [0], dtype=np.float32 if sub == "f" else np.int64)
                vals = vals.astype(np.float32) if sub == "f" else vals.astype(np.int32)
                tags.append(col(SIM_ARR, vals, off, len(arrs), m, name, sub.encode()))
    return (SimColumn * len(FIELDS))(*f), (SimColumn * max(len(tags), 1))(*tags) if tags else None, len(tags), keep


def rcpp_simulate_bam(header, fields, tags, ntags, out_fn, seed, nthreads=1, window_kib=0, nrecs=None):
    """epi_simulate_bam on prepared columns (see _columns).  Returns the number of records written."""
    lib = _lib.load()
    eng = C.c_void_p()
    _lib.check(lib.epi_default_engine(C.byref(eng)))              # no device: EpihipError, there is no CPU path
    lines = (C.c_char_p * len(header))(*[h.encode() for h in header])
    nw = C.c_int64(0)
    rc = lib.epi_simulate_bam(eng, os.path.expanduser(str(out_fn)).encode(), lines, len(header), int(nrecs), fields,
                              tags, int(ntags), C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), int(max(nthreads, 1)),
                              int(window_kib), C.byref(nw))
    if rc == _lib.EPI_ERR_ARG:
        raise ValueError(lib.epi_last_error().decode("utf-8", "replace"))    # stop(...) in the reference
    _lib.check(rc)
    return int(nw.value)


def simulateBam(output_bam_file=None, qname=None, flag=None, rname=None, pos=None, mapq=None, cigar=None, rnext=None,
                pnext=None, tlen=None, seq=None, qual=None, verbose=False, seed=None, nthreads=1, window_kib=0, **tags):
    """R/simulateBam.R.  Record count: the longest argument supplied (tags included), at least 1; every field is
    recycled to it, and the columns of each tag group are recycled to the group's longest column first.  Defaults:
    qname "q%04d" of the record number, flag 0, rname / rnext "chrS", pos / pnext 1, mapq 60, cigar "<nchar(seq)>M",
    tlen nchar(seq), qual "F" for every base.  Without `seq`, one random ACGT string is made per element of nchar(XM), else
    of tlen, else of [10]: base k of string j is "ACTG"[hash3(seed, 0x53494D, (j << 32) | k) >> 62] with synth.hip's
    hash3 (`seed` None draws one).

    Tags by Python type: int -> integer tag (narrowest of c C s S i I), float -> 'f', str -> 'Z', a list of sequences ->
    'B' array (subtype from all its values, see array_subtype).

    output_bam_file None: returns the prepared table (a Report: qname, flag, tid, pos (0-based), mapq, cigar, mtid, mpos,
    isize, seq, qual, then the tags in group order i, f, s, a) and needs no device.  Otherwise writes the BAM on the GPU
    and returns the number of records.  nthreads: BGZF compressing threads; window_kib: uncompressed bytes per window
    (0: ~64 MiB); the file does not depend on either."""
    if verbose:
        sys.stderr.write("Writing sample BAM ")
    t0 = time.time()
    if seed is None:
        seed = int.from_bytes(os.urandom(8), "little")
    supplied = [v for v in (output_bam_file, qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual)
                if v is not None]
    p = _prepare(qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual, tags, seed, supplied)
    if output_bam_file is None:
        res = _table(p)
    else:
        fields, tcols, ntags, keep = _columns(p)
        res = rcpp_simulate_bam(p["header"], fields, tcols, ntags, output_bam_file, seed, nthreads, window_kib, p["nrecs"])
        del keep
    if verbose:
        sys.stderr.write("[%.3fs]\n" % (time.time() - t0))
    return res
