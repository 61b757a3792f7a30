"""The fuzz generator's batches (test_gpu_fuzz.make_batch) and a few deliberate ones through the reports that came after
it: the heterogeneity report against its restatement (test_gpu_heterogeneity.restate), base frequencies against the
reference's loop restated (test_gpu_vcf.restated_base_freqs_fast), the multi-target pattern tables against the CPU
oracle, and the pattern summaries against a plain group-by of the ORACLE's table (no GPU report enters it).  Every
argument is drawn from the seed's generator; the draws of a seed (`plan`) and what the oracle and the restatements make
of them (`het_want`, `freqs_want`, `pattern_wants`) need no GPU: test_fuzz_reports_host.py checks on them that the seed
list reaches the shapes it is meant to reach.  Bounded by a list of seeds; a failure names its seed, kind and row count.

The draw of a heterogeneity call leans towards the batch's alphabet (a context whose letters the batch holds in both
cases, a row filter that the batch as a whole passes), so that most calls compare windows with several patterns and not
two empty tables.  The lean reads the input bytes only."""
import numpy as np
import pytest

import helpers as H
import synth_np
import test_gpu_fuzz as F
import test_gpu_heterogeneity as HT
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


def plan(seed):
    """The seed's batch and every argument, all from default_rng(seed)"""
    rng = np.random.default_rng(seed)
    if seed in DELIBERATE:
        kind = DELIBERATE[seed][0]
        t = DELIBERATE[seed][1](rng)
    else:
        kind, t = F.make_batch(rng, seed)
    return {"seed": seed, "kind": kind, "t": t, "het": draw_het_pair(rng, t, kind), "freqs": draw_freqs(rng, t),
            "patterns": draw_patterns(rng, t)}


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


def test_a_row_over_the_last_int32_position_is_refused(ea):
    """start + length = 2^31, one more than the batches of the seed list reach: an argument error from every report, no table"""
    t = near_top(np.random.default_rng(9001), -1)
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"])
    try:
        for call in (lambda: HT.gpu_report(ea, bam, "CG", 2, 1.0), lambda: ea.rcpp_cx_report(bam, None, "Z"),
                     lambda: ea.rcpp_extract_patterns_multi(bam, [(1, TOP - 500, TOP)], 1, "Zz", 0.0, False, 0),
                     lambda: ea.rcpp_get_base_freqs(bam, None, np.asarray([1], np.int32), np.asarray([TOP], np.int32))):
            with pytest.raises(ea.EpihipError) as ei:
                call()
            assert ei.value.code == 1 and "exceeds int32" in str(ei.value)
    finally:
        bam.close()
