"""A plain loop restatement of generateRegionReport's definitions (include/epihip.h, epi_batch_region_report_dev), independent
of the product: kept rows by helpers.mhl_keep_np, a row's calls in a region by slicing its bytes, runs by a loop over the
calls, every sum in Python integers and every ratio in numpy float64 scalars, one operation at a time in the stated order.
Test infrastructure only; never imported by the package."""
import numpy as np

import helpers as H

INT_COLS = ("rname", "start", "end", "nreads", "nlong", "kreads", "tbase", "mbase", "cbase", "ndiscordant", "nmethylated",
            "n_u", "n_x", "n_m", "maxsites")
FLOAT_COLS = ("beta", "pdr", "chalm", "mcr", "mbs", "mhl")
COLUMNS = INT_COLS + FLOAT_COLS
NAN = np.float64("nan")
F = np.float64


def ctx_letters(context):
    c = H.CONTEXT_TO_BASES[context]
    return c["ctx_meth"] + c["ctx_unmeth"]


def default_offset(context):
    return {"CG": 1, "CHG": 2}.get(context, 0)


def runs_of(calls):
    """Lengths of the maximal runs of True in a sequence of booleans"""
    out, run = [], 0
    for c in calls:
        if c:
            run += 1
        elif run:
            out.append(run)
            run = 0
    if run:
        out.append(run)
    return out


def row_calls(t, x, in_ctx, start, end, reverse_offset):
    """The calls of row x in [start, end], in row order: True = methylated"""
    o0, o1 = int(t["off"][x]), int(t["off"][x + 1])
    shift = int(t["start"][x]) - (int(reverse_offset) if int(t["strand"][x]) == 2 else 0)      # byte i is at shift + i
    i0, i1 = max(0, int(start) - shift), min(o1 - o0, int(end) - shift + 1)
    if i1 <= i0:
        return []
    code = t["xm"][o0 + i0:o0 + i1] & 15
    return [bool(c < 8) for c in code[in_ctx[code]]]


def ratio(a, b):
    return F(a) / F(b) if b else NAN


def region_row(rows_calls, min_sites, max_sites, u_max, m_min, weights=None):
    """One region from the call lists of its kept rows -> (integers dict, ratios dict, accumulators).  weights: how many
    rows each call list stands for (default: one)"""
    c = dict.fromkeys(INT_COLS[3:], 0)
    Hn, M, S2 = ([0] * (max_sites + 2) for _ in range(3))
    for k, calls in enumerate(rows_calls):
        wt = 1 if weights is None else int(weights[k])
        n = len(calls)
        if n < 1:
            continue
        c["nreads"] += wt
        if n > max_sites:
            c["nlong"] += wt
            continue
        m = sum(calls)
        r = runs_of(calls)
        c["maxsites"] = max(c["maxsites"], n)
        c["tbase"] += wt * n
        c["mbase"] += wt * m
        if m >= 1:
            c["cbase"] += wt * (n - m)
        Hn[n] += wt
        for l in range(1, max(r, default=0) + 1):                        # (no run reaches a larger l)
            M[l] += wt * sum(max(0, rj - l + 1) for rj in r)
        if n < min_sites:
            continue
        c["kreads"] += wt
        c["ndiscordant"] += wt * (0 < m < n)
        c["nmethylated"] += wt * (m >= 1)
        if F(m) <= F(u_max) * F(n):
            c["n_u"] += wt
        elif F(m) >= F(m_min) * F(n):
            c["n_m"] += wt
        else:
            c["n_x"] += wt
        S2[n] += wt * sum(rj * rj for rj in r)
    ms = c["maxsites"]
    d = {"beta": ratio(c["mbase"], c["tbase"]), "pdr": ratio(c["ndiscordant"], c["kreads"]),
         "chalm": ratio(c["nmethylated"], c["kreads"]), "mcr": ratio(c["cbase"], c["tbase"])}
    acc = F(0.0)
    for n in range(min_sites, ms + 1):                                   # ascending n
        acc = acc + F(S2[n]) / F(n * n)
    d["mbs"] = acc / F(c["kreads"]) if c["kreads"] else NAN
    T = [0] * (max_sites + 2)
    for l in range(1, ms + 1):
        T[l] = sum(Hn[n] * max(0, n - l + 1) for n in range(1, max_sites + 1))
    num, den = F(0.0), F(0.0)
    for l in range(1, ms + 1):                                           # ascending l
        assert T[l] > 0
        num = num + F(l) * (F(M[l]) / F(T[l]))
        den = den + F(l)
    d["mhl"] = num / den if ms else NAN
    return c, d, {"H": Hn, "M": M, "S2": S2, "T": T}


def restate(t, regions, ctx, min_sites=4, max_sites=64, reverse_offset=1, u_max=0.25, m_min=0.75, max_oo=0.1, with_acc=False):
    """t: templates (xm, off, rname, strand, start); regions: (rname codes, start, end); ctx: context letters in both cases.
    -> dict of columns (int32 / float64), one row per region in the order given"""
    chrom, rs, re_ = (np.asarray(a, np.int64) for a in regions)
    nreg = chrom.size
    n = len(t["start"])
    keep = H.mhl_keep_np(t["xm"], t["off"], ctx, 0, max_oo) if n else np.zeros(0, bool)
    in_ctx = np.zeros(16, bool)
    in_ctx[[H.ctx_to_idx(ch) for ch in ctx]] = True
    lens = np.diff(t["off"]).astype(np.int64)
    shift = t["start"].astype(np.int64) - np.where(t["strand"] == 2, int(reverse_offset), 0)
    out = {k: np.zeros(nreg, np.int32) for k in INT_COLS}
    out.update({k: np.full(nreg, np.nan, np.float64) for k in FLOAT_COLS})
    accs = []
    for g in range(nreg):
        cand = np.flatnonzero(keep & (t["rname"] == chrom[g]) & (shift <= re_[g]) & (shift + lens - 1 >= rs[g])) if n else []
        c, d, acc = region_row([row_calls(t, int(x), in_ctx, rs[g], re_[g], reverse_offset) for x in cand], min_sites, max_sites, u_max, m_min)
        out["rname"][g], out["start"][g], out["end"][g] = chrom[g], rs[g], re_[g]
        for k, v in c.items():
            out[k][g] = v
        for k, v in d.items():
            out[k][g] = v
        accs.append(acc)
    if with_acc:
        out["acc"] = accs
    return out


def bed_regions(levels, chrom, start, end):
    """(rname codes, start, end) of BED rows under the BAM's levels: NA for a sequence the BAM does not have"""
    code = {c: i + 1 for i, c in enumerate(levels or ())}
    return (np.asarray([code.get(c, H.NA_INT) for c in chrom], np.int64), np.asarray(start, np.int64), np.asarray(end, np.int64))


def same(got, want, label=""):
    """Integers equal, doubles bit for bit"""
    for k in INT_COLS:
        g = np.asarray(got[k])
        assert g.dtype == np.int32 and np.array_equal(g, want[k]), (label, k, np.flatnonzero(g != want[k])[:5])
    for k in FLOAT_COLS:
        g = np.asarray(got[k])
        assert g.dtype == np.float64, (label, k)
        bad = np.flatnonzero(g.view(np.uint64) != np.asarray(want[k], np.float64).view(np.uint64))     # (NaN: the quiet NaN of both)
        assert bad.size == 0, (label, k, bad[:5], g[bad[:5]], want[k][bad[:5]])
