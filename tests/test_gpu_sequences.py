"""Long mixed sequences of calls on a few batches at once, every result against the oracle.  Most speed-ups keep state on
the batch for the next call (remembered tile counts, threshold tables, pool slot sizes, the direct-mode record of the
last CX report's tile offsets); a cache keyed on the wrong thing only shows in such a sequence.  Batches come from the
fuzz generator plus one with raw garbage bytes (the unused low nibbles 1, 3 and 4, which count differently under a
failed read), through every constructor.  Every CX call through the C entry points also checks `written` against the
rule of include/epihip.h, predicted from the oracle's tables alone: the tile kernel writes the caller's columns when the
last pool report on the batch had the same contexts, no position is deeper than 255 rows, the kept row count is above 0
and fits, and every tile of the absolute grid yields as many rows as then.  The reports that came later take part as
operations of their own, each checked as in test_gpu_fuzz_reports.py: the heterogeneity report (whose own CX report keeps
or replaces the direct-mode record: Slot.het, with the capacity the library reports afterwards and the `written` of the
next C-level CX call against it), base frequencies, and the multi-target pattern tables and summaries, which keep
scratch groups and hash tables on the batch.  The linkage report and the heterogeneity comparison share the het_* buffers
of the batch with the heterogeneity report, at other sizes, and their own CX reports treat the record as its own does
(Slot.het again).  `link` remembers its restated pair table on the slot as the batch's live linkage report until an
operation on the slot ends it: any CX, lMHL, heterogeneity or linkage report, either side of a comparison, or a reopen;
thresholding, beta, base frequencies and the pattern calls leave it alone (linkage.hip and include/epihip.h: blocks_dev
needs the last report on the batch to be a linkage report).  `blocks_late` asks for the blocks through the C entry points
with fresh thresholds, twice where the report is live: the blocks of the remembered table, however many operations on
other batches lie between, and the pair table still that one; or a call sequence error.  `cmp` compares two slots, mostly
the first batch and its sibling (the last slot), in a drawn order: the record of both slots is modelled, the second
batch first as the library runs them, and whatever comes next on either slot is checked as always, so a site table or a
counter that the comparison left on the wrong batch shows there.  Bounded by a list of seeds; a failure names its seed
and step."""
import collections
import ctypes as C

import numpy as np
import pytest

import helpers as H
import synth_np
import test_extract_patterns as TP
import test_gpu_cx_direct as D
import test_gpu_fuzz as F
import test_gpu_fuzz_reports as R
import test_gpu_linkage as LK
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

SEEDS = list(range(5000, 5080))
GROUPS = 16
CX_LETTERS = ("Z", "ZZ", "Zz", "X", "ZX", "ZXH", "H")
NAMED = ("CG", "CHG", "CHH", "CxG", "CX")
MHL_CTX = ("Zz", "Xx", "Hh", "ZzXx", "ZzXxHh")
PASSES = ("none", "oracle", "random", "false", "na")
MAKERS = ("arrays", "pinned", "device", "zero_copy")
OPS = (("cx_c", 10), ("cx_py", 2), ("fused_py", 2), ("gcr", 1), ("mhl", 2), ("thr", 1), ("beta", 1), ("pat", 1), ("reopen", 1),
       ("het", 2), ("freqs", 1), ("pat_multi", 1), ("summ", 1), ("link", 2), ("blocks_late", 2), ("cmp", 2))
NA = -2 ** 31
# Paths over the whole seed list: C-level CX calls (`written` asserted) and Python-level ones (py_: tables only).  pool:
# no record with these contexts yet; fallback: a direct launch in which some tile's count differed, the new row count
# above / not above the kept one (above: the Python columns are allocated again).
# het_replaces / het_keeps: a heterogeneity report whose own CX report replaced the record / met one with its contexts and
# left it alone; direct_after_het: a C-level direct launch on a record that a heterogeneity report was the last to touch
# (kept or made; repeated launches count); direct_after_het_replaces: such a launch on a record that the report MADE.
# link_replaces / link_keeps: the same for the CX report under a linkage report; direct_after_link: a C-level direct launch on
# a record that a linkage report was the last to touch.  blocks_late_live: blocks computed, perhaps many operations on other
# batches later, from the counters of a linkage report that no operation on its batch has ended; blocks_late_refused: asked
# for on a batch whose last report is no linkage report (a call sequence error).  cmp_pair: a comparison of the first batch
# with its sibling, either order; cmp_self: of a batch with itself (its second CX report meets the record that the first one
# made); cmp_b_replaces: the CX report on the SECOND batch of a comparison replaced that batch's record;
# direct_after_cmp_on_b: a C-level direct launch on a record that a comparison, with the batch as its second, was the last
# to touch.
MIN_PATHS = {"pool": 150, "direct": 100, "fallback_above": 8, "fallback_below": 8, "py_direct": 40, "py_fallback_above": 5,
             "het_replaces": 5, "het_keeps": 5, "direct_after_het": 5, "direct_after_het_replaces": 5,
             "link_replaces": 5, "link_keeps": 5, "direct_after_link": 5, "blocks_late_live": 5, "blocks_late_refused": 5,
             "cmp_pair": 5, "cmp_self": 5, "cmp_b_replaces": 5, "direct_after_cmp_on_b": 5}
RAN = {}                                               # group -> its path counts (this session)


@pytest.fixture(scope="module")
def ea():
    import epialleler_amd
    return epialleler_amd


def ctx_mask(letters):
    m = 0
    for ch in letters:
        m |= 1 << H.ctx_to_idx(ch)
    return m


def deep(t):
    """k_row_stats: some row x + 255 of the same rname starts before the end of row x (u8 counters could overflow)."""
    n = t["start"].size
    if n <= 255:
        return False
    L = np.diff(t["off"])
    s = t["start"].astype(np.int64)
    x = np.arange(n - 255)
    return bool(np.any((L[x] > 0) & (t["rname"][x + 255] == t["rname"][x]) & (s[x + 255] < s[x] + L[x])))


class Slot:
    """One batch of the sequence and what the library should remember about it."""

    def __init__(self, ea, t, maker):
        self.t, self.maker = t, maker
        self.n = t["start"].size
        self.deep = deep(t)
        self.open(ea, maker)

    def open(self, ea, maker):
        import torch
        t = self.t
        self.maker = maker
        self.rec = None                                # (context mask, per-tile counts, row count) of the kept record
        # "het", "link", "cmp_a", "cmp_b": the report whose own CX report was the last call to keep or replace the record
        self.after = None
        self.het_made = False                          # the record is one that a heterogeneity report made
        self.link = None                               # (call, restated pair table) of the linkage report the batch holds
        nb = int(t["off"][-1])
        if maker == "arrays":
            self.bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"])
        elif maker == "pinned":
            cols = [torch.from_numpy(np.ascontiguousarray(t[k])).pin_memory() for k in ("xm", "off", "rname", "strand", "start")]
            self.bam = ea.ProcessedBam.from_pinned(cols[0], nb, *cols[1:])
        else:
            xm = torch.full(((nb + 15) // 16 * 16 + 16,), 0xFB, dtype=torch.uint8, device="cuda:0")
            xm[:nb] = torch.from_numpy(t["xm"]).cuda()
            dev = lambda k: torch.from_numpy(np.ascontiguousarray(t[k])).cuda()
            self.bam = ea.ProcessedBam.from_device(xm, nb, dev("off"), dev("rname"), dev("strand"), dev("start"),
                                                   realign=maker == "device")

    def predict(self, letters, want, T):
        """(path, capacity the library reports before the call); updates the record as the library does."""
        mask = ctx_mask(letters)
        counts, nrow = D.tile_counts(want, T), int(want["pos"].size)
        same = self.rec is not None and self.rec[0] == mask
        cap = self.rec[2] if same else -1
        if not same:
            path = "pool"
        elif self.rec[2] > 0 and not self.deep:
            path = "direct" if self.rec[1] == counts else ("fallback_above" if nrow > self.rec[2] else "fallback_below")
        else:
            path = "pool_again"                        # same contexts, but pile-ups or an empty kept table: the record stays
        if self.n > 0 and path in ("pool", "fallback_above", "fallback_below"):
            self.rec = (mask, counts, nrow)
            self.after, self.het_made = None, False
        return path, cap

    def het(self, letters, sites, T, by="het"):
        """What a heterogeneity report does to the record (a linkage report and either side of a comparison do the same: all
        go through site_cx_report; `by` names which): its own CX report is a pool report without caller columns, for the
        upper-case letters of its context, all rows passing (`sites`: that table).  A record with the same contexts stays
        as it is, also one made under another pass vector (cx_keep_offsets); any other is replaced by this table's tile
        counts and row count.  -> the path's name"""
        mask = ctx_mask(letters)
        if self.n == 0:
            return "het_empty"
        self.after = by
        if self.rec is not None and self.rec[0] == mask:
            return "het_keeps"
        self.rec = (mask, D.tile_counts(sites, T), int(sites["pos"].size))
        self.het_made = by == "het"
        return "het_replaces"


def make_slots(ea, rng, seed):
    ts = [F.make_batch(rng, seed * 7 + k)[1] for k in range(int(rng.integers(2, 4)))]
    ts.append(synth_np.random_templates(rng, int(rng.integers(50, 3000)), 0, int(rng.integers(20, 500)), int(rng.integers(1, 4)),
                                        int(rng.integers(200, 20000)), p_garbage=float(rng.choice([0.02, 0.1, 0.3]))))
    ts.append(R.sibling(rng, ts[0]))                    # the last slot: a second sample of the first batch's library
    return [Slot(ea, t, MAKERS[(seed + k) % len(MAKERS)]) for k, t in enumerate(ts)]


def blocks_late(ea, s, bcall):
    """epi_batch_linkage_blocks_dev on the slot and what it must give: the blocks of the linkage report the batch holds (and
    the pair table untouched), or a call sequence error from it and from the blocks' fetch -> the path's name"""
    import torch
    lib, api = ea._lib.load(), ea.api
    nb = C.c_int64(-1)
    rc = lib.epi_batch_linkage_blocks_dev(s.bam.batch(), bcall[0], bcall[1], api._stream(s.bam.device), C.byref(nb))
    if s.link is None:
        ic = list(torch.empty((5, 8), dtype=torch.int32, device="cuda:%d" % s.bam.device).unbind(0))
        dc = list(torch.empty((1, 8), dtype=torch.float64, device="cuda:%d" % s.bam.device).unbind(0))
        assert rc == ea._lib.EPI_ERR_STATE and nb.value == 0, ("blocks without a linkage report", rc, nb.value)
        assert lib.epi_batch_linkage_blocks_fetch_dev(s.bam.batch(), api._ptr_array(ic), api._ptr_array(dc), None) == ea._lib.EPI_ERR_STATE
        return "blocks_late_refused"
    call, want = s.link
    wb = R.blocks_want(want, bcall)
    assert (rc, nb.value) == (ea._lib.EPI_OK, wb["start"].size), ("blocks of the live linkage report", rc, nb.value, wb["start"].size)
    got = api._fetch_table(s.bam, lib.epi_batch_linkage_blocks_fetch_dev, nb.value, 5, api.BLOCK_COLUMNS, False)
    LK.assert_table(got, wb, LK.BLOCK_INT_COLS, LK.BLOCK_FLOAT_COLS, ("late blocks",) + tuple(call) + tuple(bcall))
    LK.assert_same(R.fetch_pairs(ea, s.bam, int(want["pos"].size)), want, ("pairs after late blocks",) + tuple(call))
    return "blocks_late_live"


def pick_pass(rng, s, kind, c4=None, thr=None):
    return R.pick_pass(rng, s.t, kind, c4, thr)


def named_of(letters):
    """the named context whose cytosine report has the contexts of `letters` (None: there is none)"""
    for name in NAMED:
        if ctx_mask(H.CONTEXT_TO_BASES[name]["ctx_meth"]) == ctx_mask(letters):
            return name
    return None


def refused_fetch(ea, s, which):
    """the lMHL or the CX fetch right after a heterogeneity report: a call sequence error, and the batch is as before"""
    import torch
    from epialleler_amd import _lib, api
    lib = _lib.load()
    ic = list(torch.empty((6, 8), dtype=torch.int32, device="cuda:%d" % (s.bam.device or 0)).unbind(0))
    dc = list(torch.empty((2, 8), dtype=torch.float64, device="cuda:%d" % (s.bam.device or 0)).unbind(0))
    if which == "mhl":
        return lib.epi_batch_mhl_fetch_dev(s.bam.batch(), api._ptr_array(ic[:5]), api._ptr_array(dc), None) == _lib.EPI_ERR_STATE
    return lib.epi_batch_cx_fetch_dev(s.bam.batch(), api._ptr_array(ic), None) == _lib.EPI_ERR_STATE


def cpu(rep):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in dict(rep).items()}


def run_seed(ea, seed, paths):
    lib = ea._lib.load()
    rng = np.random.default_rng(seed)
    slots = make_slots(ea, rng, seed)
    last = {}                                          # slot -> the last CX call's (letters, pass kind, thresholds)
    ops, weights = zip(*OPS)
    weights = np.asarray(weights, np.float64) / sum(weights)
    nsteps = int(rng.integers(15, 26))
    try:
        for step in range(nsteps):
            # the garbage batch (last but one) 40 % of the time: only its reads change a tile's row count with `pass`
            k = len(slots) - 2 if rng.random() < 0.4 else int(rng.choice([q for q in range(len(slots)) if q != len(slots) - 2]))
            s = slots[k]
            t = s.t
            op = str(rng.choice(ops, p=weights))
            live = [q for q in range(len(slots)) if slots[q].link is not None]
            if op == "blocks_late" and live and rng.random() < 0.6:   # a batch that holds a linkage report, however long ago
                k = int(rng.choice(live))
                s, t = slots[k], slots[k].t
            c4 = H.cls4(str(rng.choice(NAMED)))
            thr = (int(rng.choice(F.MN)), float(rng.choice(F.MB)), float(rng.choice(F.MO)))
            what = (step, op, k, s.maker)
            try:
                if op in ("cx_c", "cx_py", "fused_py", "gcr"):
                    if k in last and rng.random() < 0.6:   # the same contexts again, often the same pass: direct mode's chance
                        letters, pk, c4, thr = last[k]
                        if rng.random() < 0.5:
                            pk = str(rng.choice(PASSES))
                    else:
                        letters, pk = str(rng.choice(CX_LETTERS)), str(rng.choice(PASSES))
                    fused = op == "fused_py" or (op == "cx_c" and rng.random() < 0.3)
                    named = None
                    if op == "gcr":
                        named = str(rng.choice(NAMED))
                        letters = H.CONTEXT_TO_BASES[named]["ctx_meth"]
                        fused = rng.random() < 0.5
                        c4, thr = H.cls4(named), (2, 0.5, 0.1)
                        pk = "none"
                    if fused:
                        pk = "oracle"
                    last[k] = (letters, pk, c4, thr)
                    p = pick_pass(rng, s, pk, c4, thr)
                    want = orc.cx_report(t["xm"], t["off"], t["rname"], t["strand"], t["start"], p, letters)
                    T = lib.epi_cx_tile_positions(letters.encode())
                    after, het_made = s.after, s.het_made
                    s.link = None
                    path, cap = s.predict(letters, want, T)
                    what += (letters, pk, fused, thr, path)
                    assert D.capacity(ea, s.bam, letters) == cap, ("capacity", cap)
                    if op == "cx_c":
                        named_thr = [n for n in NAMED if H.cls4(n) == c4][0]
                        got, written = D.report(ea, s.bam, named_thr, fused, letters=letters, thr=thr, pass_=p)
                        H.assert_reports_equal(got, want)
                        assert written == (path == "direct"), ("written", written)
                        paths[path] += 1
                        paths["direct_after_het"] += path == "direct" and after == "het"
                        paths["direct_after_link"] += path == "direct" and after == "link"
                        paths["direct_after_cmp_on_b"] += path == "direct" and after == "cmp_b"
                        paths["direct_after_het_replaces"] += path == "direct" and het_made and after == "het"
                    else:
                        H.dirty_allocator(s.bam)
                        if op == "cx_py":
                            got = ea.rcpp_cx_report(s.bam, p, letters)
                        elif op == "fused_py":
                            got, gp = ea.cytosine_report_fused(s.bam, *c4, *thr, letters, return_pass=True)
                            assert np.array_equal(gp.astype(np.int32), p), "fused pass"
                        else:
                            dev = bool(rng.random() < 0.5)
                            got = ea.generateCytosineReport(s.bam, threshold_reads=fused, threshold_context=named, as_device=dev)
                        H.assert_reports_equal(cpu(got), want)
                        paths["py_" + path] += 1
                elif op == "mhl":
                    hctx = str(rng.choice(MHL_CTX))
                    hmax, hmin = int(rng.choice([0, 0, 1, 3, 50])), int(rng.choice([0, 0, 2, 5]))
                    moo = float(rng.choice([0.1, 0.0, 1.0, float("nan"), -0.5]))
                    what += (hctx, hmax, hmin, moo)
                    s.link = None
                    H.assert_reports_equal(cpu(ea.rcpp_mhl_report(s.bam, hctx, hmax, hmin, moo, as_device=bool(rng.random() < 0.3))),
                                           orc.mhl_report(t["xm"], t["off"], t["rname"], t["strand"], t["start"], hctx, hmax, hmin, moo),
                                           float_cols=("length", "lmhl"))
                elif op == "thr":
                    what += (c4, thr)
                    H.dirty_allocator(s.bam)
                    got = ea.rcpp_threshold_reads(s.bam, *c4, *thr)
                    assert np.array_equal(got.astype(np.int32), orc.threshold_reads(t["xm"], t["off"], *c4, *thr)), "threshold"
                elif op == "beta":
                    got = ea.rcpp_get_xm_beta(s.bam, c4[0], c4[1])
                    want = orc.get_xm_beta(t["xm"], t["off"], c4[0], c4[1])
                    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), "beta"
                elif op == "pat":
                    if s.n == 0:
                        continue
                    x = int(rng.integers(0, s.n))
                    rn, ts = int(t["rname"][x]), int(t["start"][x]) + int(rng.integers(0, 50))
                    te = ts + int(rng.integers(0, 600))
                    ctx = str(rng.choice(["Zz", "ZzXx", "HhXxZz", "Hh"]))
                    clip, ro, mo = bool(rng.integers(0, 2)), int(rng.integers(0, 3)), int(rng.integers(1, 30))
                    freq = float(rng.choice([0.0, 0.01, 0.2]))
                    hl = sorted({int(v) for v in rng.integers(ts, te + 1, size=int(rng.integers(0, 4)))})
                    what += (rn, ts, te, ctx, clip, ro, mo, freq, hl)
                    rep = ea.rcpp_extract_patterns(s.bam, rn, ts, te, mo, ctx, freq, clip, ro, hl)
                    o = orc.extract_patterns(t["xm"], t["off"], t["rname"], t["strand"], t["start"], rn, ts, te, mo, ctx, freq, clip, ro, hl)
                    a = TP.table_from_report(rep)
                    b = TP.table_from(o["strand"], o["start"], o["end"], o["nbase"], o["beta"], ["%016X" % int(v) for v in o["fnv"]],
                                      o["positions"], o["cells"])
                    assert a["positions"] == b["positions"] and a["pattern"] == b["pattern"], "patterns"
                    for c in ("strand", "start", "end", "nbase", "cells"):
                        assert np.array_equal(a[c], b[c]), c
                    assert np.array_equal(np.asarray(a["beta"], np.float64).view(np.uint64),
                                          np.asarray(b["beta"], np.float64).view(np.uint64)), "pattern beta"
                elif op == "het":
                    name = named_of(last[k][0]) if k in last and rng.random() < 0.6 else None    # the CX ops' coin: the same contexts again
                    call = R.draw_het(rng, t, ctx=name)
                    fetch = str(rng.choice(["none", "none", "mhl", "cx"]))
                    letters = H.CONTEXT_TO_BASES[call[0]]["ctx_meth"]
                    what += call + (fetch,)
                    want = R.het_want(t, call)
                    if want is None:
                        paths["het_skipped"] += 1
                        continue
                    hp = s.het(letters, want["sites"], lib.epi_cx_tile_positions(letters.encode()))
                    what += (hp,)
                    s.link = None
                    R.check_het(ea, s.bam, t, call, want)
                    assert D.capacity(ea, s.bam, letters) == (s.rec[2] if s.n else -1), ("capacity after het", s.rec and s.rec[2])
                    paths[hp] += 1
                    last[k] = (letters, "none", H.cls4(call[0]), thr)
                    if fetch != "none":
                        assert refused_fetch(ea, s, fetch), "fetch after a heterogeneity report"
                elif op == "freqs":
                    f = R.draw_freqs(rng, t)
                    what += (f["pass_kind"], int(f["chr"].size))
                    R.check_freqs(ea, s.bam, t, f)
                elif op in ("pat_multi", "summ"):
                    p = R.draw_patterns(rng, t)
                    what += tuple(p[q] for q in ("targets", "mo", "ctx", "freq", "clip", "ro", "hl", "bin"))
                    (R.check_multi if op == "pat_multi" else R.check_summ)(ea, s.bam, t, p)
                elif op == "link":
                    name = named_of(last[k][0]) if k in last and rng.random() < 0.6 else None    # the CX ops' coin, as for het
                    call, _ = R.draw_link(rng, t, ctx=name)
                    letters = H.CONTEXT_TO_BASES[call[0]]["ctx_meth"]
                    what += call
                    want = R.link_want(t, call)
                    if want is None:
                        paths["link_skipped"] += 1
                        continue
                    lp = s.het(letters, want["sites"], lib.epi_cx_tile_positions(letters.encode()), by="link").replace("het_", "link_")
                    what += (lp,)
                    s.link = None
                    R.check_link(ea, s.bam, t, call, want)
                    assert D.capacity(ea, s.bam, letters) == (s.rec[2] if s.n else -1), ("capacity after link", s.rec and s.rec[2])
                    s.link = (call, want)
                    paths[lp] += 1
                    last[k] = (letters, "none", H.cls4(call[0]), thr)
                elif op == "blocks_late":
                    # twice with fresh thresholds where the report is live: the second call finds the first one's block lengths
                    for _ in range(1 if s.link is None else 2):
                        bcall = (float(rng.choice(R.MIN_R2)), int(rng.choice(R.MIN_SITES)))
                        what += bcall
                        bp = blocks_late(ea, s, bcall)
                    paths[bp] += 1
                elif op == "cmp":
                    sib = len(slots) - 1
                    if rng.random() < 0.7:                 # the first batch and its sibling
                        ka, kb = 0, sib
                    elif rng.random() < 1 / 3:             # the slot itself
                        ka, kb = k, k
                    else:                                  # any other slot: usually no common site
                        ka, kb = k, int(rng.choice([q for q in range(len(slots)) if q != k]))
                    if rng.random() < 0.5:
                        ka, kb = kb, ka
                    sa, sb = slots[ka], slots[kb]
                    name = named_of(last[ka][0]) if ka in last and rng.random() < 0.6 else None
                    call = R.draw_het(rng, sa.t, ctx=name)
                    letters = H.CONTEXT_TO_BASES[call[0]]["ctx_meth"]
                    what += (ka, kb, sb.maker) + call
                    want = R.cmp_want(sa.t, sb.t, call)
                    if want is None:
                        paths["cmp_skipped"] += 1
                        continue
                    # the library runs the second batch's CX report first; with one slot on both sides its second report meets
                    # the record that the first one made
                    T = lib.epi_cx_tile_positions(letters.encode())
                    pb = sb.het(letters, want["sites_b"], T, by="cmp_b")
                    pa = sa.het(letters, want["sites_a"], T, by="cmp_a")
                    what += (pb, pa)
                    assert ka != kb or pa == "het_keeps"
                    sa.link = sb.link = None
                    R.check_cmp(ea, sa.bam, sb.bam, sa.t, sb.t, call, want)
                    for q in (sa, sb):
                        assert D.capacity(ea, q.bam, letters) == (q.rec[2] if q.n else -1), ("capacity after cmp", q.maker, q.rec and q.rec[2])
                    paths["cmp_pair"] += {ka, kb} == {0, sib}
                    paths["cmp_self"] += ka == kb
                    paths["cmp_b_replaces"] += pb == "het_replaces"
                    paths["cmp"] += 1
                    last[ka] = last[kb] = (letters, "none", H.cls4(call[0]), thr)
                else:                                      # reopen: a fresh batch of the same rows, maybe another constructor
                    s.bam.close()
                    last.pop(k, None)
                    s.open(ea, str(rng.choice(MAKERS)))
                    what += (s.maker,)
            except AssertionError as e:
                raise AssertionError("seed %d, step %d: %r: %s" % (seed, step, what, e)) from e
    finally:
        for s in slots:
            s.bam.close()


def run_group(ea, group):
    paths = collections.Counter()
    for seed in SEEDS[group::GROUPS]:
        run_seed(ea, seed, paths)
    RAN[group] = paths
    return paths


@pytest.mark.parametrize("group", range(GROUPS))
def test_sequences(ea, group):
    paths = run_group(ea, group)
    print("group %d paths: %s" % (group, dict(sorted(paths.items()))))
    assert paths["pool"] and paths["direct"]


def test_paths_over_all_seeds(ea):
    """Every path of the direct-mode rule was taken (and checked) a minimum number of times over the whole seed list; the
    groups not run in this session are run here."""
    total = collections.Counter()
    for g in range(GROUPS):
        total.update(RAN[g] if g in RAN else run_group(ea, g))
    print("paths over all seeds: %s" % dict(sorted(total.items())))
    for p, m in MIN_PATHS.items():
        assert total[p] >= m, (p, dict(total))
