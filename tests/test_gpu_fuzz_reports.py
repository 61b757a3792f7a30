"""The fuzz generator's batches (test_gpu_fuzz.make_batch) and a few deliberate ones through the reports that came after
it: the heterogeneity report against its restatement (test_gpu_heterogeneity.restate), base frequencies against the
reference's loop restated (test_gpu_vcf.restated_base_freqs_fast), the multi-target pattern tables against the CPU
oracle, the pattern summaries against a plain group-by of the ORACLE's table (no GPU report enters it), the linkage report
and the haplotype blocks against test_gpu_linkage.restate / restate_blocks (and the pair table fetched again after the
blocks), and the heterogeneity comparison of the batch with a sibling (`sibling`: a second sample of the same rows, calls
flipped, a tenth of the positions blanked) in both orders against test_gpu_heterogeneity_compare.restate, with those
modules' own tolerances.  Every argument is drawn from the seed's generators; the draws of a seed (`plan`) and what the
oracle and the restatements make of them (`het_want`, `freqs_want`, `pattern_wants`, `link_want`, `blocks_want`,
`cmp_want`) need no GPU: test_fuzz_reports_host.py checks on them that the seed list reaches the shapes it is meant to
reach.  Bounded by a list of seeds; a failure names its seed, kind and row count.

The draw of a heterogeneity call leans towards the batch's alphabet (a context whose letters the batch holds in both
cases, a row filter that the batch as a whole passes), so that most calls compare windows with several patterns and not
two empty tables; the linkage and comparison calls take context, row filter, min_reads and the cap from the same lean.
The lean reads the input bytes only.  On the deliberate batches the arguments of the two newer calls are fixed."""
import time

import numpy as np
import pytest

import helpers as H
import synth_np
import test_gpu_fuzz as F
import test_gpu_heterogeneity as HT
import test_gpu_heterogeneity_compare as HC
import test_gpu_linkage as LK
import test_gpu_patterns_bed as PB
import test_gpu_summarise_patterns as SP
import test_gpu_vcf as V
import test_extract_patterns as TP
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

NAMED = ("CG", "CHG", "CHH", "CxG", "CX")
MAX_OO = (1.0, float("nan"), 0.3, 0.1, 0.0)
MIN_READS = (1, 1, 2, 5)
PASSES = ("none", "oracle", "random", "false", "na")
PAT_CTX = ("Zz", "ZzXx", "HhXxZz", "Hh")
TOP = 2 ** 31 - 1
NA = -2 ** 31
COUNTER_CAP = 64 << 20                                 # bytes of counters (sites x 2^k x 4) above which a call is skipped
LINK_D = (1, 2, 3, 5, 8, 15, 16)
MIN_R2 = (0.0, 0.1, 0.5, 1.0)
MIN_SITES = (2, 3, 5)
FLIP = (0.1, 0.3, 0.5)


# ---- the deliberate batches ---------------------------------------------------------------------------------------------

def near_top(rng, below):
    """300 to 2000 rows of 2 to 400 bytes on two sequences, CpG calls only, shifted so that the last row ends at 2^31 - 1 -
    below: start + length = 2^31 - 1 - below, and below = 0 is the last batch the library takes (its rows keep start +
    length within int32; test_a_row_over_the_last_int32_position_is_refused has the next one)"""
    t = synth_np.random_templates(rng, int(rng.integers(300, 2001)), 2, 400, 2, 3000, alphabet="zZ.")
    end = int((t["start"].astype(np.int64) + np.diff(t["off"])).max())
    t["start"] = (t["start"].astype(np.int64) + (TOP - below - end)).astype(np.int32)
    assert int((t["start"].astype(np.int64) + np.diff(t["off"])).max()) == TOP - below and t["start"].min() > 0
    return t


def pile_up(rng):
    """600 rows of 40 to 120 bytes that start within 30 positions of each other (every window of the pile is covered by
    more than 255 rows: the CX report under the heterogeneity report runs its general kernel), 200 sparse rows on a
    second and a third sequence"""
    pile = synth_np.random_templates(rng, 600, 40, 120, 1, 31, alphabet="zzzzZ....")
    rest = synth_np.random_templates(rng, 200, 40, 120, 2, 20000, alphabet="zzzzZ....")
    rest["rname"] = rest["rname"] + 1
    t = PB.merge([pile, rest])
    assert int(pile["start"].max()) <= 30 and int(np.count_nonzero((t["rname"] == 1) & (t["start"] <= 30))) == 600
    return t


def deep_pile(rng):
    """1000 rows of 40 to 120 bytes within 30 positions, a CpG call at every byte: windows of more than 255 READS on either
    strand (the pile above, with calls at five bytes in nine, stays below 200), counters that many rows of a wave add to"""
    return synth_np.random_templates(rng, 1000, 40, 120, 1, 31, alphabet="zZ")


def empty_rows_and_garbage(rng):
    """three tenths of the bytes raw garbage, a tenth of the rows of length 0"""
    t = synth_np.random_templates(rng, 1500, 1, 300, 3, 8000, p_garbage=0.3)
    lens = np.diff(t["off"])
    empty = rng.random(lens.size) < 0.1
    t["xm"] = t["xm"][np.repeat(~empty, lens)]
    t["off"] = np.concatenate(([0], np.cumsum(np.where(empty, 0, lens)))).astype(np.int64)
    assert 100 < int(np.count_nonzero(np.diff(t["off"]) == 0)) < 220
    return t


DELIBERATE = {9001: ("top", lambda rng: near_top(rng, 0)), 9002: ("below_top", lambda rng: near_top(rng, int(rng.integers(200, 600)))),
              9003: ("pile", pile_up), 9004: ("empty", empty_rows_and_garbage), 9005: ("deep_pile", deep_pile)}
DROPPED = (1001, 1017, 1041)                            # three of the eight benchmark-model batches (kind 5), the slowest seeds
SEEDS = [s for s in range(1000, 1055) if s not in DROPPED] + sorted(DELIBERATE)
# Groups of about equal time (the restatement's loop over the rows is most of it), set from the seeds' measured times: the
# four slowest seeds have a group each.  No group may take longer than the slowest group of test_gpu_fuzz.test_fuzz_seeds.
SEED_GROUPS = ([1031], [1020], [1021], [1000], [1009, 1016, 1035, 1037, 9004], [1015, 1023, 1036, 1042, 1054],
               [1002, 1006, 1007, 1012, 1019, 1039, 1049], [1025, 1028, 1034, 1048, 1050, 1053],
               [1003, 1004, 1008, 1024, 1030, 1033, 1051], [1010, 1011, 1014, 1022, 1044, 9002, 9003],
               [1005, 1018, 1026, 1027, 1032, 1046, 1047, 1052], [1013, 1029, 1038, 1040, 1043, 1045, 9001, 9005])
GROUPS = len(SEED_GROUPS)
assert sorted(s for g in SEED_GROUPS for s in g) == sorted(SEEDS)
# The linkage calls (with their blocks) and the comparisons (both orders) have groups of their own, by the same rule and set
# in the same way: most of the time is the restatements' loop over the rows.
LINK_GROUPS = ([1021], [1020], [1004, 1007, 1019, 1031], [1032, 1034, 1043, 1052], [1000, 1033, 1042, 1051], [1028, 1049, 1054, 9002],
               [1003, 1018, 1024, 1044, 1045, 1047, 1050, 9001], [1006, 1008, 1015, 1022, 1029, 1037, 1038, 1039, 1046, 1053, 9005],
               [1002, 1005, 1009, 1010, 1011, 1012, 1013, 1014, 1016, 1023, 1025, 1026, 1027, 1030, 1035, 1036, 1040, 1048, 9003, 9004])
CMP_GROUPS = ([1020], [1021], [1031], [1033, 9002], [1000, 1011, 1028], [1022, 1024, 1034], [1003, 1032, 1049, 9001],
              [1005, 1010, 1014, 1018, 1023], [1002, 1004, 1008, 1016, 1029, 1050, 1053],
              [1006, 1015, 1019, 1026, 1036, 1039, 1052, 9003, 9005],
              [1007, 1009, 1012, 1013, 1025, 1027, 1030, 1035, 1037, 1038, 1040, 1042, 1043, 1044, 1045, 1046, 1047, 1048, 1051, 1054, 9004])
assert sorted(s for g in LINK_GROUPS for s in g) == sorted(s for g in CMP_GROUPS for s in g) == sorted(SEEDS)
# (No call alone passes the bar: none is shrunk.  The per-seed times that the tests print are there for the next regrouping.)


# ---- what a seed draws --------------------------------------------------------------------------------------------------

def both_cases(nib, name):
    """the batch holds some letter of the named context methylated and unmethylated"""
    c = H.CONTEXT_TO_BASES[name]
    return any(nib[H.ctx_to_idx(m)] > 0 and nib[H.ctx_to_idx(u)] > 0 for m, u in zip(c["ctx_meth"], c["ctx_unmeth"]))


def draw_het(rng, t, ctx=None, k=None, max_oo=None):
    """One heterogeneity call: (context name, k, max_ooctx_meth_frac, min_reads, max_window_span).  The context leans
    16 : 1 towards those the batch has in both cases; a max_oo under which the read rule drops more than half of the rows
    gives way to 1.0 or NaN three times out of four."""
    nib = np.bincount(t["xm"][:int(t["off"][-1])] & 15, minlength=16)
    w = np.asarray([16.0 if both_cases(nib, name) else 1.0 for name in NAMED])
    name = ctx or str(rng.choice(NAMED, p=w / w.sum()))
    kk = int(rng.integers(2, 7))
    mo = float(rng.choice(MAX_OO))
    c = H.CONTEXT_TO_BASES[name]
    kept = H.mhl_keep_np(t["xm"], t["off"], c["ctx_meth"] + c["ctx_unmeth"], 0, mo)
    redraw = float(rng.choice((1.0, float("nan")))), rng.random() < 0.75
    if 2 * np.count_nonzero(kept) < kept.size and redraw[1]:
        mo = redraw[0]
    min_reads = int(rng.choice(MIN_READS))
    L = np.diff(t["off"])
    span = int(rng.choice([0, max(int(np.median(L[L > 0])) if np.any(L > 0) else 1, 2)]))
    return (name, k or kk, mo if max_oo is None else max_oo, min_reads, span)


def draw_het_pair(rng, t, kind):
    """Two calls with different (context, k); on the batches at the top of the coordinate range CG, every row kept, k = 2
    and 6; on the deep pile CG and CX, every row kept."""
    if kind in ("top", "below_top"):
        return [draw_het(rng, t, "CG", 2, 1.0), draw_het(rng, t, "CG", 6, 1.0)]
    if kind == "deep_pile":
        return [draw_het(rng, t, "CG", None, 1.0), draw_het(rng, t, "CX", None, 1.0)]
    a = draw_het(rng, t)
    b = draw_het(rng, t)
    while b[:2] == a[:2]:
        b = draw_het(rng, t)
    return [a, b]


def pick_pass(rng, t, kind, c4=None, thr=None):
    """A pass vector of the named kind for the templates t (test_gpu_sequences.pick_pass is this)"""
    n = t["start"].size
    if kind == "none":
        return None
    if kind == "oracle":
        return orc.threshold_reads(t["xm"], t["off"], *c4, *thr)
    if kind == "random":
        return rng.integers(0, 2, size=n).astype(np.int32)
    if kind == "false":
        return np.zeros(n, np.int32)
    p = rng.integers(0, 2, size=n).astype(np.int32)
    p[rng.random(n) < 0.3] = NA                        # R's NA: non-zero, so TRUE
    return p


def draw_pass(rng, t):
    """(kind, pass vector or None)"""
    kind = str(rng.choice(PASSES))
    c4 = H.cls4(str(rng.choice(NAMED)))
    thr = (int(rng.choice(F.MN)), float(rng.choice(F.MB)), float(rng.choice(F.MO)))
    return kind, pick_pass(rng, t, kind, c4, thr)


def draw_freqs(rng, t):
    """Base-frequency sites over the batch's own span and sequences (test_gpu_vcf._sites: sorted, a tenth of the positions
    twice), a pass vector, the sites to NA-code (a tenth) and the caller's order."""
    L = np.diff(t["off"])
    lo = int(t["start"].min())
    span = max(int((t["start"].astype(np.int64) + L).max()) - lo, 1)
    chr_, p = V._sites(rng, int(t["rname"].max()), span, max(span // 1500, 2))
    pos = np.minimum(p.astype(np.int64) + (lo - 1), TOP).astype(np.int32)
    kind, pass_ = draw_pass(rng, t)
    na = rng.random(chr_.size) < 0.1
    return {"chr": chr_, "pos": pos, "pass_kind": kind, "pass": pass_, "na": na, "perm": rng.permutation(chr_.size)}


def draw_patterns(rng, t):
    """1 to 8 targets anchored at rows of the batch and one on a sequence the batch lacks, with the arguments of
    test_gpu_patterns_bed.test_random_batches_and_arguments; bin: the context of the summaries' beta."""
    n = t["start"].size
    targets = []
    for _ in range(int(rng.integers(1, 9))):
        x = int(rng.integers(0, n))
        ts = min(int(t["start"][x]) + int(rng.integers(0, 50)), TOP)
        targets.append((int(t["rname"][x]), ts, min(ts + int(rng.integers(0, 601)), TOP)))
    ts = int(t["start"][int(rng.integers(0, n))])
    targets.insert(int(rng.integers(0, len(targets) + 1)), (int(t["rname"].max()) + 1, ts, min(ts + 300, TOP)))
    hl = [sorted({int(p) for p in rng.integers(a, b + 1, size=int(rng.integers(0, 4)))}) for _, a, b in targets]
    return {"targets": targets, "mo": int(rng.integers(1, 30)), "ctx": str(rng.choice(PAT_CTX)), "freq": float(rng.choice([0.0, 0.01, 0.2])),
            "clip": bool(rng.integers(0, 2)), "ro": int(rng.integers(0, 3)), "hl": hl if rng.random() < 2 / 3 else None,
            "bin": str(rng.choice(NAMED))}


def sibling(rng, t):
    """A second sample of the same library, from the input arrays alone: between half and all of the rows, drawn with
    replacement and kept in batch order; every call byte (low nibble & 7 in {2, 5, 6, 7}) changes its methylation bit with
    one probability per sibling; a salted tenth of the genomic positions shows '.' in every row, so that the sibling lacks
    sites that the original has."""
    n = t["start"].size
    rows = np.sort(rng.integers(0, n, size=int(rng.integers((n + 1) // 2, n + 1))))
    p_flip, salt = float(rng.choice(FLIP)), int(rng.integers(0, 2 ** 31))
    lens = np.diff(t["off"])[rows]
    off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    i = np.arange(int(off[-1]), dtype=np.int64)
    xm = t["xm"][np.repeat(t["off"][:-1][rows] - off[:-1], lens) + i].copy()
    pos = np.repeat(t["start"][rows].astype(np.int64) - off[:-1], lens) + i
    flip = np.isin(xm & 7, (2, 5, 6, 7)) & (rng.random(xm.size) < p_flip)
    xm[flip] ^= 8
    gone = ((pos + salt).astype(np.uint64) * np.uint64(2654435761) % np.uint64(2 ** 32)) % np.uint64(10) == 0
    xm[gone] = (xm[gone] & 0xF0) | 12
    return {"xm": xm, "off": off, "rname": t["rname"][rows].copy(), "strand": t["strand"][rows].copy(), "start": t["start"][rows].copy()}


def draw_link(rng, t, ctx=None):
    """One linkage call and the block call on it: ((context name, D, max_ooctx_meth_frac, min_reads, max_distance),
    (min_r2, min_sites)).  Context, row filter, min_reads and the distance cap (0 or the median row length) are draw_het's
    lean (its k is not used)."""
    name, _, mo, min_reads, dist = draw_het(rng, t, ctx=ctx)
    return (name, int(rng.choice(LINK_D)), mo, min_reads, dist), draw_blocks(rng)


def draw_blocks(rng):
    return float(rng.choice(MIN_R2)), int(rng.choice(MIN_SITES))


def draw_link_calls(rng, t, kind):
    """The seed's linkage calls: one.  On the deliberate batches the arguments are fixed: at the top of the coordinate range CG,
    every row kept, D = 1 without and D = 16 with a distance cap (16: about half of the pairs eleven and more sites apart
    pass it); on the piles CG, every row kept, every pair reported, D drawn."""
    if kind in ("top", "below_top"):
        return [(("CG", 1, 1.0, int(rng.choice(MIN_READS)), 0), draw_blocks(rng)),
                (("CG", 16, 1.0, int(rng.choice(MIN_READS)), 16), draw_blocks(rng))]
    if kind in ("deep_pile", "pile"):
        return [(("CG", int(rng.choice(LINK_D)), 1.0, 1, 0), draw_blocks(rng))]
    return [draw_link(rng, t)]


def draw_cmp(rng, t):
    """(the sibling, a heterogeneity call for the pair)"""
    return sibling(rng, t), draw_het(rng, t)


def draw_cmp_calls(rng, t, kind):
    """(the sibling, the seed's comparison calls): one.  On the deliberate batches the arguments are fixed: at the top of the
    coordinate range CG, every row kept, k = 2 and 6; on the piles CX, every row kept, min_reads 1, k drawn."""
    if kind in ("top", "below_top"):
        return sibling(rng, t), [("CG", 2, 1.0, int(rng.choice(MIN_READS)), 0), ("CG", 6, 1.0, int(rng.choice(MIN_READS)), 0)]
    if kind in ("deep_pile", "pile"):
        return sibling(rng, t), [("CX", int(rng.integers(2, 7)), 1.0, 1, 0)]
    sib, call = draw_cmp(rng, t)
    return sib, [call]


def plan(seed):
    """The seed's batch and every argument: the batch and the calls of the first five reports from default_rng(seed), the
    linkage calls, the sibling and the comparison calls from a generator of their own (the older draws do not move)"""
    rng = np.random.default_rng(seed)
    if seed in DELIBERATE:
        kind = DELIBERATE[seed][0]
        t = DELIBERATE[seed][1](rng)
    else:
        kind, t = F.make_batch(rng, seed)
    p = {"seed": seed, "kind": kind, "t": t, "het": draw_het_pair(rng, t, kind), "freqs": draw_freqs(rng, t),
         "patterns": draw_patterns(rng, t)}
    rng2 = np.random.default_rng([seed, 1])
    p["link"] = draw_link_calls(rng2, t, kind)
    p["sibling"], p["cmp"] = draw_cmp_calls(rng2, t, kind)
    return p


# ---- what the restatements and the oracle make of the draws ----------------------------------------------------------------

def het_want(t, call):
    """The restatement's report, or None where the counters of the call (sites x 2^k x 4 bytes) pass COUNTER_CAP"""
    want = HT.restate(t, *call)
    return want if (int(want["sites"]["pos"].size) << call[1]) * 4 <= COUNTER_CAP else None


def freqs_want(t, f):
    """(the caller's site codes, positions, the matrix in the caller's order)"""
    pass_ = f["pass"] if f["pass"] is not None else np.ones(t["start"].size, np.int32)
    want = V.restated_base_freqs_fast(t, pass_, f["chr"], f["pos"])
    return np.where(f["na"], NA, f["chr"])[f["perm"]].astype(np.int32), f["pos"][f["perm"]], np.where(f["na"][:, None], 0, want)[f["perm"]]


def as_report(tab):
    """A table of test_extract_patterns.table_from as the mapping summary_np reads: pattern and a column per position"""
    if not tab["pattern"]:
        return {}
    rep = {"pattern": tab["pattern"]}
    for p, col in zip(tab["positions"], tab["cells"]):
        rep[str(p)] = col
    assert len(rep) == 1 + len(tab["positions"]) > 1
    return rep


def pattern_wants(t, p):
    """per target: (the oracle's table, the plain summary of that table)"""
    out = []
    for k, tg in enumerate(p["targets"]):
        tab = PB.oracle_table(t, tg, p["mo"], p["ctx"], p["freq"], p["clip"], p["ro"], p["hl"][k] if p["hl"] is not None else ())
        out.append((tab, SP.summary_np(as_report(tab), p["bin"])))
    return out


def link_want(t, call):
    """test_gpu_linkage.restate's pair table, or None where the counters of the call (sites x D x 16 bytes) pass COUNTER_CAP"""
    nsite = int(HC.site_table(t, call[0])["pos"].size)
    return LK.restate(t, *call) if nsite * call[1] * 16 <= COUNTER_CAP else None


def blocks_want(want, bcall):
    return LK.restate_blocks(want, *bcall)


def site_codes(s):
    """(rname, strand, pos, context) of a site table as one int64 per row"""
    return ((s["rname"].astype(np.int64) << 36) | (s["pos"].astype(np.int64) << 4) | (s["context"].astype(np.int64) << 1)
            | (s["strand"].astype(np.int64) - 1))


def cmp_want(ta, tb, call):
    """test_gpu_heterogeneity_compare.restate's comparison, or None where the counters of one side (common sites x 2^k x 4
    bytes) pass COUNTER_CAP"""
    sa, sb = HC.site_table(ta, call[0]), HC.site_table(tb, call[0])
    ncommon = int(np.count_nonzero(np.isin(site_codes(sa), site_codes(sb))))
    if (ncommon << call[1]) * 4 > COUNTER_CAP:
        return None
    want = HC.restate(ta, tb, *call)
    assert want["ncommon"] == ncommon
    return want


# ---- the checks -----------------------------------------------------------------------------------------------------------

def check_het(ea, bam, t, call, want=None):
    """-> the restatement's report (None: skipped for size)"""
    want = het_want(t, call) if want is None else want
    if want is not None:
        HT.assert_same(HT.gpu_report(ea, bam, *call), want, ("het",) + tuple(call))
    return want


def check_freqs(ea, bam, t, f):
    c2, p2, want = freqs_want(t, f)
    got = ea.rcpp_get_base_freqs(bam, f["pass"], c2, p2)
    assert got.shape == want.shape and np.array_equal(got, want), ("base freqs", f["pass_kind"], int(np.count_nonzero(got != want)))
    return want


def same_summary(got, want):
    """test_gpu_summarise_patterns.same_summary, with the yardstick made from the oracle's table"""
    if want is None:
        assert not got and got.nrow == 0
        return
    assert list(got.keys()) == want["columns"]
    assert list(got["pattern"]) == want["pattern"]
    for k, col in zip(SP.position_columns(got), want["cells"]):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], col), k
    assert np.array_equal(got["count"], want["count"])
    assert got["beta"].dtype == np.float64 and np.array_equal(got["beta"].view(np.uint64), want["beta"].view(np.uint64))


def check_multi(ea, bam, t, p, wants=None):
    wants = pattern_wants(t, p) if wants is None else wants
    reps = ea.rcpp_extract_patterns_multi(bam, p["targets"], p["mo"], p["ctx"], p["freq"], p["clip"], p["ro"], p["hl"])
    assert len(reps) == len(wants)
    for k, (rep, (tab, _)) in enumerate(zip(reps, wants)):
        try:
            PB.same_table(TP.table_from_report(rep), tab)
        except AssertionError as e:
            raise AssertionError("patterns of target %d %r: %s" % (k, p["targets"][k], e)) from e
    return wants


def check_summ(ea, bam, t, p, wants=None):
    wants = pattern_wants(t, p) if wants is None else wants
    c = H.CONTEXT_TO_BASES[p["bin"]]
    reps = ea.rcpp_summarise_patterns_multi(bam, p["targets"], p["mo"], p["ctx"], p["freq"], p["clip"], p["ro"], p["hl"],
                                            (c["ctx_meth"], c["ctx_unmeth"]))
    assert len(reps) == len(wants)
    for k, (rep, (_, summ)) in enumerate(zip(reps, wants)):
        try:
            same_summary(rep, summ)
        except AssertionError as e:
            raise AssertionError("summary of target %d %r: %s" % (k, p["targets"][k], e)) from e
    return wants


def fetch_pairs(ea, bam, nrow):
    """the pair table of the linkage report that the batch holds, fetched (again)"""
    return ea.api._fetch_table(bam, ea._lib.load().epi_batch_linkage_fetch_dev, nrow, 11, ea.api.LINKAGE_COLUMNS, False)


def check_link(ea, bam, t, call, want=None):
    """-> the restatement's pair table (None: skipped for size)"""
    want = link_want(t, call) if want is None else want
    if want is not None:
        LK.assert_same(LK.gpu_report(ea, bam, *call), want, ("link",) + tuple(call))
    return want


def check_blocks(ea, bam, call, bcall, want):
    """The blocks of a call whose pair table `want` is, through rcpp_linkage_blocks (the report again, then the blocks), and the
    pair table fetched after them"""
    got = LK.gpu_blocks(ea, bam, call[0], call[1], bcall[0], bcall[1], *call[2:])
    wb = blocks_want(want, bcall)
    LK.assert_table(got, wb, LK.BLOCK_INT_COLS, LK.BLOCK_FLOAT_COLS, ("blocks",) + tuple(call) + tuple(bcall))
    LK.assert_same(fetch_pairs(ea, bam, int(want["pos"].size)), want, ("pairs after blocks",) + tuple(call))
    return wb


def check_cmp(ea, bam_a, bam_b, ta, tb, call, want=None):
    """-> the restatement's comparison of (a, b) (None: skipped for size)"""
    want = cmp_want(ta, tb, call) if want is None else want
    if want is not None:
        HC.assert_same(HC.gpu_compare(ea, bam_a, bam_b, *call), want, ("cmp",) + tuple(call))
    return want


@pytest.fixture(scope="module")
def ea():
    import epialleler_amd
    return epialleler_amd


def run_seed(ea, seed):
    p = plan(seed)
    t = p["t"]
    n = t["start"].size
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"])
    skipped = 0
    try:
        for call in p["het"]:
            skipped += check_het(ea, bam, t, call) is None
        check_freqs(ea, bam, t, p["freqs"])
        wants = check_multi(ea, bam, t, p["patterns"])
        check_summ(ea, bam, t, p["patterns"], wants)
    except AssertionError as e:
        raise AssertionError("seed %d (kind %s, %d rows): %s" % (seed, p["kind"], n, e)) from e
    finally:
        bam.close()
    return skipped


@pytest.mark.parametrize("group", range(GROUPS))
def test_fuzz_report_seeds(ea, group):
    seeds = SEED_GROUPS[group]
    skipped = sum(run_seed(ea, seed) for seed in seeds)
    print("group %d: %d seeds, %d heterogeneity calls skipped for size" % (group, len(seeds), skipped))


def run_link_seed(ea, seed):
    """-> (calls skipped for size, calls run)"""
    p = plan(seed)
    t = p["t"]
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"])
    skipped = 0
    try:
        for call, bcall in p["link"]:
            want = check_link(ea, bam, t, call)
            if want is None:
                skipped += 1
                continue
            check_blocks(ea, bam, call, bcall, want)
    except AssertionError as e:
        raise AssertionError("seed %d (kind %s, %d rows): %s" % (seed, p["kind"], t["start"].size, e)) from e
    finally:
        bam.close()
    return skipped, len(p["link"])


def run_cmp_seed(ea, seed):
    """Both orders, each against its own restatement -> (calls skipped for size, calls run)"""
    p = plan(seed)
    ta, tb = p["t"], p["sibling"]
    bams = [ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"]) for t in (ta, tb)]
    skipped = 0
    try:
        for call in p["cmp"]:
            skipped += check_cmp(ea, bams[0], bams[1], ta, tb, call) is None
            skipped += check_cmp(ea, bams[1], bams[0], tb, ta, call) is None
    except AssertionError as e:
        raise AssertionError("seed %d (kind %s, %d and %d rows): %s" % (seed, p["kind"], ta["start"].size, tb["start"].size, e)) from e
    finally:
        for b in bams:
            b.close()
    return skipped, 2 * len(p["cmp"])


def timed(run, ea, seed):
    t0 = time.perf_counter()
    out = run(ea, seed)
    print("seed %d: %.2f s" % (seed, time.perf_counter() - t0))
    return out


@pytest.mark.parametrize("group", range(len(LINK_GROUPS)))
def test_fuzz_linkage_seeds(ea, group):
    ran = [timed(run_link_seed, ea, seed) for seed in LINK_GROUPS[group]]
    print("group %d: %d seeds, %d of %d linkage calls skipped for size" % (group, len(ran), sum(r[0] for r in ran), sum(r[1] for r in ran)))


@pytest.mark.parametrize("group", range(len(CMP_GROUPS)))
def test_fuzz_compare_seeds(ea, group):
    ran = [timed(run_cmp_seed, ea, seed) for seed in CMP_GROUPS[group]]
    print("group %d: %d seeds, %d of %d comparisons skipped for size" % (group, len(ran), sum(r[0] for r in ran), sum(r[1] for r in ran)))


def test_a_row_over_the_last_int32_position_is_refused(ea):
    """start + length = 2^31, one more than the batches of the seed list reach: an argument error from every report, no table;
    the comparison refuses it on either side, and the good batch it was compared with is fit for a comparison afterwards"""
    t = near_top(np.random.default_rng(9001), -1)
    good = plan(9001)["t"]
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"])
    ok = ea.ProcessedBam.from_arrays(good["xm"], good["off"], good["rname"], good["strand"], good["start"])
    try:
        for call in (lambda: HT.gpu_report(ea, bam, "CG", 2, 1.0), lambda: ea.rcpp_cx_report(bam, None, "Z"),
                     lambda: LK.gpu_report(ea, bam, "CG", 4, 1.0),
                     lambda: HC.gpu_compare(ea, bam, ok, "CG", 3, 1.0), lambda: HC.gpu_compare(ea, ok, bam, "CG", 3, 1.0),
                     lambda: ea.rcpp_extract_patterns_multi(bam, [(1, TOP - 500, TOP)], 1, "Zz", 0.0, False, 0),
                     lambda: ea.rcpp_get_base_freqs(bam, None, np.asarray([1], np.int32), np.asarray([TOP], np.int32))):
            with pytest.raises(ea.EpihipError) as ei:
                call()
            assert ei.value.code == 1 and "exceeds int32" in str(ei.value)
        want = HC.restate(good, good, "CG", 3, 1.0)
        assert want["pos"].size > 0 and np.any(want["npatterns_a"] > 1)
        HC.assert_same(HC.gpu_compare(ea, ok, ok, "CG", 3, 1.0), want, "the good batch with itself, after the refusal")
    finally:
        bam.close()
        ok.close()
