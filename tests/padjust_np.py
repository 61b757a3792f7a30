"""Plain numpy restatement of the p-value adjustment as include/epihip.h defines it (epi_p_adjust_dev): a stable argsort with
NaN last, each method's terms in the header's operation order, running minimum / maximum, min(1, t) back to the rows.  Every
term is one IEEE division and / or multiplication and minimum and maximum are exact, so the GPU tests compare bit for bit.
Nothing here reads a GPU result."""
import numpy as np

METHODS = ("none", "bonferroni", "holm", "hochberg", "BH", "BY")
CODES = {"none": 0, "bonferroni": 1, "holm": 2, "hochberg": 3, "BH": 4, "BY": 5}


def harmonic(N):
    """The sum of 1.0 / k over k = 1 .. N in ascending k, sequentially in fp64 (np.sum would sum pairwise)."""
    return float(np.cumsum(1.0 / np.arange(1, N + 1, dtype=np.float64))[-1]) if N > 0 else 0.0


def order_np(p):
    """order[r]: the row with ascending rank r; stable, NaN last; -0.0 as 0.0."""
    return np.argsort(np.asarray(p, np.float64) + 0.0, kind="stable")


def adjust_np(p, method, n_tests=None):
    """(q, order, m).  Raises ValueError where the library returns EPI_ERR_ARG."""
    p = np.asarray(p, np.float64).reshape(-1) + 0.0
    valid = ~np.isnan(p)
    m = int(valid.sum())
    if np.any(valid & ~((p >= 0.0) & (p <= 1.0))):
        raise ValueError("a p-value outside [0, 1]")
    if n_tests is not None and n_tests > 0 and n_tests < m:
        raise ValueError("n_tests below the number of p-values")
    N = n_tests if n_tests is not None and n_tests > 0 else m
    order = order_np(p)
    q = np.full(p.size, np.nan)
    if m == 0:
        return q, order, m
    s = p[order[:m]]
    j = np.arange(1, m + 1, dtype=np.int64)
    jd = j.astype(np.float64)
    Nd = np.float64(N)
    if method == "none":
        t = s
    elif method == "bonferroni":
        t = Nd * s
    elif method == "holm":
        t = np.maximum.accumulate((N + 1 - j).astype(np.float64) * s)
    elif method == "hochberg":
        t = np.minimum.accumulate(((N + 1 - j).astype(np.float64) * s)[::-1])[::-1]
    elif method == "BH":
        t = np.minimum.accumulate(((Nd / jd) * s)[::-1])[::-1]
    elif method == "BY":
        c = np.float64(harmonic(N))
        t = np.minimum.accumulate((((c * Nd) / jd) * s)[::-1])[::-1]
    else:
        raise ValueError(method)
    q[order[:m]] = np.minimum(1.0, t)
    return q, order, m


def brute_np(p, method):
    """BH and Holm straight from their textbook definitions, O(m^2): q_i = min over k >= rank(i) of m p_(k) / k, and
    max over k <= rank(i) of (m - k + 1) p_(k); no NaN.  For agreement to rounding, not bit for bit."""
    p = np.asarray(p, np.float64)
    m = p.size
    srt = np.sort(p)
    rank = np.empty(m, np.int64)
    rank[np.argsort(p, kind="stable")] = np.arange(1, m + 1)
    q = np.empty(m)
    for i in range(m):
        if method == "BH":
            k = np.arange(rank[i], m + 1)
            q[i] = min(1.0, float(np.min(m * srt[k - 1] / k)))
        else:
            k = np.arange(1, rank[i] + 1)
            q[i] = min(1.0, float(np.max((m - k + 1) * srt[k - 1])))
    return q


def digit_passes(p):
    """How many of the key's eight bytes differ somewhere in the column: the radix passes the library runs."""
    p = np.asarray(p, np.float64).reshape(-1) + 0.0
    key = np.where(np.isnan(p), np.uint64(0xFFFFFFFFFFFFFFFF), p.view(np.uint64))
    return sum(int(np.unique((key >> np.uint64(8 * d)) & np.uint64(255)).size > 1) for d in range(8))
