"""generateFdrpReport restated from its definitions (include/epihip.h, epi_batch_fdrp_report_dev): loops over rows, sites
and pairs.  The site table is the CPU restatement's cx_report with an all-ones pass vector, the kept rows are
helpers.mhl_keep_np; nothing here reads a GPU result.  fdrp and qfdrp perform the IEEE operations of the definition in its
order (qfdrp's terms H[o] / o are added in a Python loop in ascending o: numpy's pairwise sum has another order), so a
GPU table is expected to agree bit for bit."""
import numpy as np

import helpers as H
from oracle import oracle as orc

INT_COLS = ("rname", "strand", "pos", "context", "coverage", "nreads", "npairs", "ndiscordant")
FLOAT_COLS = ("fdrp", "qfdrp")


def site_table(t, ctx):
    """The un-thresholded cytosine report of the templates t: its six columns, in its row order."""
    n = t["off"].size - 1
    cx = orc.cx_report(np.asarray(t["xm"], np.uint8), t["off"], t["rname"], t["strand"], t["start"], np.ones(max(n, 1), np.int32)[:n],
                       H.CONTEXT_TO_BASES[ctx]["ctx_meth"])
    return {q: np.asarray(cx[q]) for q in ("rname", "strand", "pos", "context", "meth", "unmeth")}


def _popcount(x):
    return bin(x).count("1")


_bit_count = getattr(int, "bit_count", _popcount)          # (restate_indexed: three times as fast where Python has it)


def selected_ranks(c, m):
    """Ranks (in the list of the c covering rows) of the rows that are used."""
    return list(range(c)) if c <= m else [(j * c) // m for j in range(m)]


def restate(t, ctx, flank_sites=8, max_reads=40, min_overlap=1, max_distance=0, max_oo=0.1, min_reads=2):
    """The FDRP table of the templates t as a dict of its ten columns, plus `sites` (the whole site table) and `used`: per
    reported row the batch rows that were compared."""
    W, m = int(flank_sites), int(max_reads)
    c_ = H.CONTEXT_TO_BASES[ctx]
    sites = site_table(t, ctx)
    n = t["off"].size - 1
    xm = np.asarray(t["xm"], np.uint8)
    keep = H.mhl_keep_np(xm, t["off"], c_["ctx_meth"] + c_["ctx_unmeth"], 0, max_oo) if n else np.zeros(0, bool)
    N = sites["pos"].size
    out = {q: [] for q in INT_COLS + FLOAT_COLS}
    used = []
    # per (rname, strand) segment: its sites by position and every kept row's calls as two integers, bit j = site j
    segs = {}
    for r in np.unique(sites["rname"]):
        for s in (1, 2):
            cxrows = np.flatnonzero((sites["rname"] == r) & (sites["strand"] == s))
            P = sites["pos"][cxrows].astype(np.int64)
            assert np.all(np.diff(P) > 0)
            code = sites["context"][cxrows]
            calls = []                                      # (batch row, valid bits, methylated bits), ascending batch row
            for x in np.flatnonzero((t["rname"] == r) & (t["strand"] == s) & keep):
                st, o0, o1 = int(t["start"][x]), int(t["off"][x]), int(t["off"][x + 1])
                a, b = int(np.searchsorted(P, st)), int(np.searchsorted(P, st + (o1 - o0)))
                v = mm = 0
                for j in range(a, b):
                    nib = int(xm[o0 + (int(P[j]) - st)]) & 15
                    if (nib & 7) == int(code[j]):
                        v |= 1 << j
                        if nib < 8:
                            mm |= 1 << j
                if v:
                    calls.append((int(x), v, mm))
            segs[(int(r), s)] = (P, calls)
    for i in range(N):
        P, calls = segs[(int(sites["rname"][i]), int(sites["strand"][i]))]
        j = int(np.searchsorted(P, int(sites["pos"][i])))
        cover = [q for q in calls if (q[1] >> j) & 1]
        c = len(cover)
        sel = [cover[k] for k in selected_ranks(c, m)]
        nreads = len(sel)
        win = 0
        for w in range(max(0, j - W), min(P.size, j + W + 1)):
            if max_distance == 0 or abs(int(P[w]) - int(P[j])) <= max_distance:
                win |= 1 << w
        npairs = ndisc = 0
        Hh = [0] * (2 * W + 2)
        for a in range(nreads):
            for b in range(a + 1, nreads):
                both = sel[a][1] & sel[b][1] & win
                o = _popcount(both)
                h = _popcount((sel[a][2] ^ sel[b][2]) & both)
                if o >= min_overlap:
                    npairs += 1
                    ndisc += 1 if h > 0 else 0
                    Hh[o] += h
        if nreads < max(min_reads, 2) or npairs < 1:
            continue
        q = np.float64(0.0)
        for o in range(1, 2 * W + 2):
            q = q + np.float64(Hh[o]) / np.float64(o)
        for name in ("rname", "strand", "pos", "context"):
            out[name].append(int(sites[name][i]))
        out["coverage"].append(c); out["nreads"].append(nreads); out["npairs"].append(npairs); out["ndiscordant"].append(ndisc)
        out["fdrp"].append(np.float64(ndisc) / np.float64(npairs))
        out["qfdrp"].append(q / np.float64(npairs))
        used.append([q_[0] for q_ in sel])
    res = {q: np.asarray(out[q], np.int32) for q in INT_COLS}
    res.update({q: np.asarray(out[q], np.float64) for q in FLOAT_COLS})
    res["sites"] = sites
    res["used"] = used
    return res


def restate_indexed(t, ctx, flank_sites=8, max_reads=40, min_overlap=1, max_distance=0, max_oo=0.1, min_reads=2):
    """restate for large tables: the same definitions in the same loops, but the rows that cover a site are looked up in a
    list per site that is filled while the rows are walked (restate scans every row of the segment per site: 48 s for
    65 000 sites on one sequence), and a row's calls are two integers whose bit 0 is the row's OWN first site, so that no
    integer is as long as the segment.  Rows are walked in ascending batch row: every site's list is in that order.
    test_fdrp_host.py shows the two equal, column for column and in `used`."""
    W, m = int(flank_sites), int(max_reads)
    c_ = H.CONTEXT_TO_BASES[ctx]
    sites = site_table(t, ctx)
    n = t["off"].size - 1
    xm = np.asarray(t["xm"], np.uint8)
    keep = H.mhl_keep_np(xm, t["off"], c_["ctx_meth"] + c_["ctx_unmeth"], 0, max_oo) if n else np.zeros(0, bool)
    N = sites["pos"].size
    out = {q: [] for q in INT_COLS + FLOAT_COLS}
    used = []
    segs = {}
    for r in np.unique(sites["rname"]):
        for s in (1, 2):
            cxrows = np.flatnonzero((sites["rname"] == r) & (sites["strand"] == s))
            P = sites["pos"][cxrows].astype(np.int64)
            assert np.all(np.diff(P) > 0)
            code = sites["context"][cxrows].tolist()
            Pl = P.tolist()
            cover = [[] for _ in Pl]                        # per site: (batch row, its first site, valid bits, methylated bits)
            for x in np.flatnonzero((t["rname"] == r) & (t["strand"] == s) & keep):
                st, o0, o1 = int(t["start"][x]), int(t["off"][x]), int(t["off"][x + 1])
                a, b = int(np.searchsorted(P, st)), int(np.searchsorted(P, st + (o1 - o0)))
                row = xm[o0:o1].tolist()
                v = mm = 0
                for j in range(a, b):
                    nib = row[Pl[j] - st] & 15
                    if (nib & 7) == code[j]:
                        v |= 1 << (j - a)
                        if nib < 8:
                            mm |= 1 << (j - a)
                entry = (int(x), a, v, mm)
                for j in range(a, b):
                    if (v >> (j - a)) & 1:
                        cover[j].append(entry)
            segs[(int(r), s)] = (P, Pl, {p: j for j, p in enumerate(Pl)}, cover)
    for i in range(N):
        P, Pl, where, cover = segs[(int(sites["rname"][i]), int(sites["strand"][i]))]
        j = where[int(sites["pos"][i])]
        c = len(cover[j])
        sel = [cover[j][k] for k in selected_ranks(c, m)]
        nreads = len(sel)
        w0 = max(0, j - W)
        win = 0                                             # bit 0 = site w0
        for w in range(w0, min(len(Pl), j + W + 1)):
            if max_distance == 0 or abs(Pl[w] - Pl[j]) <= max_distance:
                win |= 1 << (w - w0)
        # the selected rows' calls inside the window, bit 0 = site w0
        vs = [((q[2] >> (w0 - q[1])) if w0 >= q[1] else (q[2] << (q[1] - w0))) & win for q in sel]
        ms = [((q[3] >> (w0 - q[1])) if w0 >= q[1] else (q[3] << (q[1] - w0))) & win for q in sel]
        npairs = ndisc = 0
        Hh = [0] * (2 * W + 2)
        for a in range(nreads):
            va, ma = vs[a], ms[a]
            for b in range(a + 1, nreads):
                both = va & vs[b]
                o = _bit_count(both)
                h = _bit_count((ma ^ ms[b]) & both)
                if o >= min_overlap:
                    npairs += 1
                    ndisc += 1 if h > 0 else 0
                    Hh[o] += h
        if nreads < max(min_reads, 2) or npairs < 1:
            continue
        q = np.float64(0.0)
        for o in range(1, 2 * W + 2):
            q = q + np.float64(Hh[o]) / np.float64(o)
        for name in ("rname", "strand", "pos", "context"):
            out[name].append(int(sites[name][i]))
        out["coverage"].append(c); out["nreads"].append(nreads); out["npairs"].append(npairs); out["ndiscordant"].append(ndisc)
        out["fdrp"].append(np.float64(ndisc) / np.float64(npairs))
        out["qfdrp"].append(q / np.float64(npairs))
        used.append([q_[0] for q_ in sel])
    res = {q: np.asarray(out[q], np.int32) for q in INT_COLS}
    res.update({q: np.asarray(out[q], np.float64) for q in FLOAT_COLS})
    res["sites"] = sites
    res["used"] = used
    return res
