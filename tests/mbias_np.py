"""A plain loop restatement of the M-bias report's definition (include/epihip.h, epi_batch_mbias_report_dev) over
(xm, off, strand), and of suggestTrim from its description -- test infrastructure, written from the text and not from the
kernel or the product's Python."""
import numpy as np

COLUMNS = ("end", "strand", "context", "offset", "meth", "unmeth", "beta")
CODES = (2, 6, 7)                                            # CHH, CHG, CG: the order of the table's contexts
CLASS = {7: (2, 0), 15: (2, 1), 6: (1, 0), 14: (1, 1), 2: (0, 0), 10: (0, 1)}   # code -> (context index k, state: 0 meth, 1 unmeth)
CONTEXT_CODES = {"CG": (7,), "CHG": (6,), "CHH": (2,), "CxG": (6, 7), "CX": (2, 6, 7)}


def counts(xm, off, strand, max_offset):
    """-> (tables[2 ends][2 strands][3 contexts][max_offset][2 states], totals[2][3][2]), int64; one loop over the bytes"""
    M = int(max_offset)
    tab = np.zeros((2, 2, 3, M, 2), np.int64)
    tot = np.zeros((2, 3, 2), np.int64)
    xm = np.asarray(xm, np.uint8)
    for x in range(len(off) - 1):
        a, L = int(off[x]), int(off[x + 1]) - int(off[x])
        s = int(strand[x]) - 1
        row = xm[a:a + L] & 15
        for i in np.flatnonzero(np.isin(row, list(CLASS))):
            k, state = CLASS[int(row[i])]
            i = int(i)
            tot[s, k, state] += 1
            if i < M:
                tab[0, s, k, i, state] += 1
            if L - 1 - i < M:
                tab[1, s, k, L - 1 - i, state] += 1
    return tab, tot


def beta(meth, unmeth):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.asarray(meth, np.int64).astype(np.float64) / (np.asarray(meth, np.int64) + np.asarray(unmeth, np.int64)).astype(np.float64)


def table(tab, context="CX"):
    """The report's columns from counts()' tables: rows in the order end, strand, context, offset; dense"""
    M = tab.shape[3]
    rows = [(e + 1, s + 1, CODES[k], d, tab[e, s, k, d, 0], tab[e, s, k, d, 1])
            for e in range(2) for s in range(2) for k in range(3) if CODES[k] in CONTEXT_CODES[context] for d in range(M)]
    cols = [np.asarray([r[c] for r in rows], np.int32 if c < 4 else np.int64) for c in range(6)]
    assert all(int(c.max(initial=0)) < 2 ** 31 for c in cols[4:])
    out = dict(zip(COLUMNS, [c.astype(np.int32) for c in cols]))
    out["beta"] = beta(out["meth"], out["unmeth"])
    return out


def totals_table(tot, context="CX"):
    rows = [(s + 1, CODES[k], tot[s, k, 0], tot[s, k, 1]) for s in range(2) for k in range(3) if CODES[k] in CONTEXT_CODES[context]]
    out = dict(strand=np.asarray([r[0] for r in rows], np.int32), context=np.asarray([r[1] for r in rows], np.int32),
               meth=np.asarray([r[2] for r in rows], np.int64), unmeth=np.asarray([r[3] for r in rows], np.int64))
    out["beta"] = beta(out["meth"], out["unmeth"])
    return out


def restate(t, max_offset, context="CX"):
    """(table, totals) of the templates t (dict with xm, off, strand)"""
    tab, tot = counts(t["xm"], t["off"], t["strand"], max_offset)
    return table(tab, context), totals_table(tot, context)


def same(got, want, label=""):
    """Every cell equal; doubles bit for bit (NaN included)"""
    assert list(got.keys()) == list(want.keys()), (label, list(got.keys()))
    for k, w in want.items():
        g = np.asarray(got[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (label, k, g.dtype, g.shape, w.dtype, w.shape)
        if w.dtype == np.float64:
            assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), (label, k)
        else:
            assert np.array_equal(g, w), (label, k, np.flatnonzero(g != w)[:8])


def suggest_trim(rep, context="CG", max_delta=0.05, min_calls=100, run=3):
    """(trim5, trim3) from a report's columns, by the description: per end pool both strands of the context; D0 = max_offset //
    2; plateau over offsets >= D0 (ValueError on an empty one); d conforms with fewer than min_calls calls or within max_delta
    of the plateau; the smallest t in [0, D0] with every d in [t, min(t + run, D0)) conforming."""
    max_offset = int(np.max(rep["offset"])) + 1
    D0 = max_offset // 2
    out = []
    for end in (1, 2):
        meth, calls = [0] * max_offset, [0] * max_offset
        for e, c, d, m, u in zip(rep["end"], rep["context"], rep["offset"], rep["meth"], rep["unmeth"]):
            if int(e) == end and int(c) in CONTEXT_CODES[context]:
                meth[int(d)] += int(m)
                calls[int(d)] += int(m) + int(u)
        if sum(calls[D0:]) == 0:
            raise ValueError("empty plateau")
        plateau = sum(meth[D0:]) / sum(calls[D0:])
        ok = [calls[d] < min_calls or abs(meth[d] / calls[d] - plateau) <= max_delta for d in range(max_offset)]
        t = 0
        while not all(ok[d] for d in range(t, min(t + run, D0))):
            t += 1
        out.append(t)
    return tuple(out)
