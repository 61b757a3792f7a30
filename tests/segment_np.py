"""The plain restatement (Python integers, loops, no GPU result read) of the methylation-segment HMM as include/epihip.h defines
it (epi_cx_segment_dev): the quantisation, the coverage clip, the Viterbi decode per chain with its tie rules, the hard-EM
counts and re-estimate, the segment table, and the tables the tests share.  It is written from the definition, not from the
kernels: one pass forward over a chain keeping every psi, one pass back.  Scores and table entries are Python integers
(unbounded), so nothing here can wrap; the doubles of the fit come from single IEEE operations and are compared bit for bit.
Test infrastructure only; treat what the functions return as read-only."""
import math

import numpy as np

import smooth_np as S

CX = S.CX
SITE_COLUMNS = CX + ("state",)
SEG_INT = ("rname", "strand", "context", "start", "end", "state", "nsites")
SEG_FLOAT = ("meth", "unmeth", "beta")
SEGMENT_COLUMNS = SEG_INT + SEG_FLOAT
FLOOR = 2.0 ** -16
MIN_STATES, MAX_STATES, MAX_COVERAGE, MAX_SITES = 2, 4, 32767, 2 ** 26
Q_FLOOR = -726817                                             # q(2^-16)


def q(x):
    """floor(log(x) * 65536 + 0.5): libm's log in fp64, one multiplication by a power of two (exact), one addition"""
    return int(math.floor(math.log(x) * 65536.0 + 0.5))


def check_model(p, trans, init):
    """ValueError where the call gives EPI_ERR_ARG for the model"""
    K = len(p)
    if not MIN_STATES <= K <= MAX_STATES or len(init) != K or len(trans) != K or any(len(row) != K for row in trans):
        raise ValueError("bad model: states")
    rows = [list(map(float, row)) for row in trans]
    for x, top in [(float(v), 1.0 - FLOOR) for v in p] + [(v, 1.0) for row in rows for v in row] + [(float(v), 1.0) for v in init]:
        if not (x >= FLOOR and x <= top):
            raise ValueError("bad model: range")
    for row in rows + [list(map(float, init))]:
        s = 0.0
        for v in row:
            s += v
        if not abs(s - 1.0) <= 1e-9:
            raise ValueError("bad model: sum")


def quantise(p, trans, init):
    """The four tables as Python integers: A[k], B[k], T[j][k], I[k]"""
    K = len(p)
    return dict(A=[q(float(p[k])) for k in range(K)], B=[q(1.0 - float(p[k])) for k in range(K)],
                T=[[q(float(trans[j][k])) for k in range(K)] for j in range(K)], I=[q(float(init[k])) for k in range(K)])


def tables_flat(tab):
    return tab["A"] + tab["B"] + [x for row in tab["T"] for x in row] + tab["I"]


def clip(meth, unmeth, max_coverage):
    meth, unmeth = int(meth), int(unmeth)
    cov = meth + unmeth
    if cov > max_coverage:
        m = (meth * max_coverage) // cov
        return m, max_coverage - m
    return meth, unmeth


def decode_chain(tab, m, u):
    """(states, score) of one chain from its clipped counts: delta and every psi by the definition, ties to the smallest index"""
    K = len(tab["A"])
    A, B, T, I = tab["A"], tab["B"], tab["T"], tab["I"]
    L = len(m)
    delta = [I[k] + m[0] * A[k] + u[0] * B[k] for k in range(K)]
    psi = [None]
    for i in range(1, L):
        new, back = [], []
        for k in range(K):
            cand = [delta[j] + T[j][k] for j in range(K)]
            best = max(cand)
            back.append(cand.index(best))                      # the smallest j attaining it
            new.append(best + m[i] * A[k] + u[i] * B[k])
        delta = new
        psi.append(back)
    score = max(delta)
    states = [0] * L
    states[L - 1] = delta.index(score)                         # the smallest k attaining it
    for i in range(L - 1, 0, -1):
        states[i - 1] = psi[i][states[i]]
    return states, score


def series(t, max_gap):
    """(rows in series order, first site of every chain + [n]) of the CX table t"""
    cols = {k: np.asarray(t[k], np.int64) for k in CX}
    n = cols["pos"].size
    cls = (cols["strand"] - 1) * 8 + cols["context"]
    order = sorted(range(n), key=lambda i: int(cls[i]))        # (sorted is stable)
    starts = []
    for s, row in enumerate(order):
        prev = order[s - 1] if s else None
        if s == 0 or cls[row] != cls[prev] or cols["rname"][row] != cols["rname"][prev] or cols["pos"][row] - cols["pos"][prev] > max_gap:
            starts.append(s)
    return order, starts + [n]


def reestimate(K, M, U, N, S_, p, trans, init):
    """step 3, one IEEE division per entry; returns new lists"""
    p, trans, init = list(p), [list(row) for row in trans], list(init)
    for k in range(K):
        if M[k] + U[k] == 0:
            continue
        x = float(M[k] + 1) / float(M[k] + U[k] + 2)
        p[k] = min(max(x, FLOOR), 1.0 - FLOOR)
    for j in range(K):
        row = sum(N[j])
        if row == 0:
            continue
        trans[j] = [float(N[j][k] + 1) / float(row + K) for k in range(K)]
    total = sum(S_)
    init = [float(S_[k] + 1) / float(total + K) for k in range(K)]
    return p, trans, init


def segment_np(t, p, trans, init, max_gap=5000, max_coverage=1000, max_iter=10):
    """The whole call on the CX table t: `state` (int32, t's row order), `segments` (the ten columns), `fit`, `nchain`,
    `nsegment`; ValueError where the call gives EPI_ERR_ARG."""
    check_model(p, trans, init)
    if not 1 <= max_coverage <= MAX_COVERAGE or max_iter < 1 or max_gap < 0:
        raise ValueError("bad argument")
    cols = {k: np.asarray(t[k], np.int64) for k in CX}
    n = cols["pos"].size
    if n > MAX_SITES:
        raise ValueError("too many rows")
    if not S.is_sorted(t) or (n and (not np.isin(cols["strand"], (1, 2)).all() or cols["context"].min() < 0 or cols["context"].max() > 7 or
                                     min(cols["pos"].min(), cols["meth"].min(), cols["unmeth"].min()) < 0)):
        raise ValueError("bad table")
    K = len(p)
    p, trans, init = [float(x) for x in p], [[float(x) for x in row] for row in trans], [float(x) for x in init]
    fit = dict(p=p, trans=trans, init=init, score=0, iterations=0, converged=0)
    out = dict(state=np.zeros(n, np.int32), nchain=0, nsegment=0, fit=fit,
               segments={k: np.zeros(0, np.int32 if k in SEG_INT else np.float64) for k in SEGMENT_COLUMNS})
    if n == 0:
        return out
    order, starts = series(t, max_gap)
    chains = list(zip(starts, starts[1:]))
    clipped = [clip(cols["meth"][row], cols["unmeth"][row], max_coverage) for row in order]
    m, u = [c[0] for c in clipped], [c[1] for c in clipped]
    tab = quantise(p, trans, init)
    for it in range(1, max_iter + 1):
        states, score = [0] * n, 0
        for lo, hi in chains:
            st, sc = decode_chain(tab, m[lo:hi], u[lo:hi])
            states[lo:hi] = st
            score += sc
        fit.update(p=p, trans=trans, init=init, score=score, iterations=it)
        if it == max_iter:
            break
        M, U, N, S_ = [0] * K, [0] * K, [[0] * K for _ in range(K)], [0] * K
        for lo, hi in chains:
            S_[states[lo]] += 1
            for s in range(lo, hi):
                M[states[s]] += m[s]
                U[states[s]] += u[s]
                if s > lo:
                    N[states[s - 1]][states[s]] += 1
        new_p, new_trans, new_init = reestimate(K, M, U, N, S_, p, trans, init)
        new_tab = quantise(new_p, new_trans, new_init)
        if new_tab == tab:
            fit["converged"] = 1
            break
        p, trans, init, tab = new_p, new_trans, new_init, new_tab
    rows = []
    for lo, hi in chains:
        s = lo
        while s < hi:
            e = s
            while e + 1 < hi and states[e + 1] == states[s]:
                e += 1
            first, last = order[s], order[e]
            meth = sum(int(cols["meth"][order[x]]) for x in range(s, e + 1))
            unmeth = sum(int(cols["unmeth"][order[x]]) for x in range(s, e + 1))
            beta = float(meth) / float(meth + unmeth) if meth + unmeth else float("nan")
            rows.append((int(cols["rname"][first]), int(cols["strand"][first]), int(cols["context"][first]), int(cols["pos"][first]),
                         int(cols["pos"][last]), states[s], e + 1 - s, float(meth), float(unmeth), beta))
            s = e + 1
    out["state"][np.asarray(order)] = np.asarray(states, np.int32)
    out["segments"] = {k: np.asarray([r[i] for r in rows], np.int32 if k in SEG_INT else np.float64) for i, k in enumerate(SEGMENT_COLUMNS)}
    out["nchain"], out["nsegment"] = len(chains), len(rows)
    return out


def start_model(state_beta=(0.1, 0.5, 0.9), stay=0.99):
    """segmentCytosineReport's starting model"""
    K = len(state_beta)
    rest = (1.0 - float(stay)) / (K - 1)
    return ([float(x) for x in state_beta], [[float(stay) if j == k else rest for k in range(K)] for j in range(K)], [1.0 / K] * K)


def random_model(rng, K, dyadic):
    """A model of K states; dyadic: every parameter a power of two or a sum of few, so that the tables tie often"""
    if dyadic:
        p = [float(x) for x in rng.choice([0.125, 0.25, 0.5, 0.75, 0.875], K)]
        rows = {2: [[0.5, 0.5], [0.75, 0.25], [0.25, 0.75]], 3: [[0.5, 0.25, 0.25], [0.25, 0.5, 0.25], [0.25, 0.25, 0.5]],
                4: [[0.25] * 4, [0.5, 0.25, 0.125, 0.125], [0.125, 0.125, 0.25, 0.5]]}[K]
        trans = [list(rows[int(rng.integers(len(rows)))]) for _ in range(K)]
        init = list(rows[int(rng.integers(len(rows)))])
        return p, trans, init
    p = [float(x) for x in rng.uniform(0.02, 0.98, K)]
    norm = lambda v: [float(x) for x in (v / v.sum())]
    trans = [norm(rng.uniform(0.05, 1.0, K)) for _ in range(K)]
    return p, trans, norm(rng.uniform(0.05, 1.0, K))


def bits(x):
    return np.asarray(x, np.float64).reshape(-1).view(np.uint64)


def same_fit(got, want, what=""):
    """the fit's doubles bit for bit, its integers equal"""
    for k in ("p", "trans", "init"):
        assert np.array_equal(bits(got[k]), bits(want[k])), (what, k, got[k], want[k])
    for k in ("score", "iterations", "converged"):
        assert int(got[k]) == int(want[k]), (what, k, got[k], want[k])


def same_segments(got, want, what=""):
    """integer columns equal, float columns bit for bit (NaN where want has NaN)"""
    for k in SEGMENT_COLUMNS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        if k in SEG_FLOAT:
            assert g.dtype == np.float64 and np.array_equal(np.isnan(g), np.isnan(w)), (what, k)
            assert np.array_equal(bits(g[~np.isnan(g)]), bits(w[~np.isnan(w)])), (what, k)
        else:
            assert g.dtype == np.int32 and np.array_equal(g, w), (what, k, np.flatnonzero(g != w)[:5])
