"""generateFdrpReport on the host side: the exported symbols, the functions' signatures, argument checks before any I/O,
the pair list's limit as a function of its own, the loud failure without a device (the pairs are compared on the GPU; there
is no CPU path), and the restatement of the definitions (tests/fdrp_np.py) against the closed form that FDRP has without
flanking sites."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import fdrp_np
import helpers as H
import epialleler_amd as ea
from epialleler_amd import _lib

NEW_SYMBOLS = ("epi_batch_fdrp_report_dev", "epi_batch_fdrp_fetch_dev", "epi_fdrp_pair_bytes")
EMPTY = inspect.Parameter.empty


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_symbols_declared_exported_and_listed():
    _lib.build()
    with open(os.path.join(H.GOLDEN, "..", "..", "include", "epihip.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(_lib.load(), name)
        assert re.search(r"\bint %s\(" % name, hdr)
    assert ea.FDRP_COLUMNS == ("rname", "strand", "pos", "context", "coverage", "nreads", "npairs", "ndiscordant", "fdrp", "qfdrp")


def test_signatures_and_defaults():
    p = inspect.signature(ea.generateFdrpReport).parameters
    assert [(k, v.default) for k, v in p.items() if v.kind is not v.VAR_KEYWORD] == [
        ("bam", EMPTY), ("report_file", None), ("fdrp_context", None), ("flank_sites", 8), ("max_reads", 40), ("min_overlap", 1),
        ("max_distance", 0), ("min_reads", 2), ("max_outofcontext_beta", 0.1), ("gzip", False), ("verbose", False), ("as_device", False)]
    assert [k for k, v in p.items() if v.kind is v.VAR_KEYWORD] == ["preprocess_args"]
    q = inspect.signature(ea.rcpp_fdrp_report).parameters
    assert [(k, v.default) for k, v in q.items()] == [
        ("df", EMPTY), ("ctx", EMPTY), ("flank_sites", EMPTY), ("max_reads", EMPTY), ("min_overlap", EMPTY), ("max_distance", EMPTY),
        ("max_ooctx_meth_frac", EMPTY), ("min_reads", 2), ("as_device", False)]


BAD = [dict(flank_sites=-1), dict(flank_sites=32), dict(flank_sites=2.5), dict(max_reads=1), dict(max_reads=65),
       dict(min_overlap=0), dict(min_overlap=18), dict(flank_sites=0, min_overlap=2), dict(flank_sites=31, min_overlap=64),
       dict(max_distance=-1), dict(fdrp_context="CpG"), dict(fdrp_context="cg")]
R_NAME = {"flank_sites": "flank.sites", "max_reads": "max.reads", "min_overlap": "min.overlap", "max_distance": "max.distance"}


@pytest.mark.parametrize("kw", BAD)
def test_bad_arguments_raise_before_io(kw):
    with pytest.raises(ValueError) as ei:
        ea.generateFdrpReport("no-such-file.bam", **kw)      # (opening it would raise "Unable to open BAM file")
    msg = str(ei.value)
    name = list(kw)[-1]                                      # (min_overlap 2W + 2: the last key is the one that is wrong)
    if name == "fdrp_context":
        assert "'fdrp.context' should be one of 'CG', 'CHG', 'CHH', 'CxG', 'CX'" in msg
    else:
        assert "'%s' should be" % R_NAME[name] in msg
    assert "no-such-file" not in msg and "open" not in msg


def test_good_arguments_reach_the_file():
    for kw in (dict(flank_sites=0), dict(flank_sites=31, min_overlap=63), dict(max_reads=2), dict(max_reads=64, fdrp_context="CX"),
               dict(min_overlap=17), dict(max_distance=0), dict(max_distance=500)):
        with pytest.raises(Exception) as ei:
            ea.generateFdrpReport("no-such-file.bam", **kw)
        assert not isinstance(ei.value, ValueError) or "should be" not in str(ei.value)


def test_pair_bytes():
    """24 bytes per call for the two (key, row) buffers; 2^32 calls or more do not fit the sort's 32-bit indices."""
    lib = _lib.load()
    out = C.c_int64(-1)
    for ncalls in (0, 1, 2 ** 32 - 1):
        assert lib.epi_fdrp_pair_bytes(ncalls, C.byref(out)) == _lib.EPI_OK and out.value == 24 * ncalls
    for ncalls in (2 ** 32, 2 ** 40, -1):
        assert lib.epi_fdrp_pair_bytes(ncalls, C.byref(out)) == _lib.EPI_ERR_ARG and out.value == 0, ncalls
    assert b"calls" in lib.epi_last_error()
    assert lib.epi_fdrp_pair_bytes(1, None) == _lib.EPI_ERR_ARG


def test_fails_loudly_without_gpu():
    if _has_gpu():
        pytest.skip("GPU present")
    t = H.templates_from_xm(["Z.z.Z.z", "z.Z.z.Z"], [1, 1], [1, 1])
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"])
    for call in (lambda: ea.generateFdrpReport(bam, flank_sites=2), lambda: ea.rcpp_fdrp_report(bam, "Zz", 2, 40, 1, 0, 0.1)):
        with pytest.raises(ea.EpihipError) as ei:
            call()
        assert ei.value.code == 5 and "no CPU fallback" in str(ei.value)


def closed_form_templates(seed=5, nrow=60, length=40):
    """Reads of Z, z and '.' only (no out-of-context call: the read rule keeps every row, so the cytosine report's counts
    are the coverage), both strands, ragged starts."""
    rng = np.random.default_rng(seed)
    xms, starts, strands = [], [], []
    for _ in range(nrow):
        L = int(rng.integers(5, length))
        st = int(rng.integers(1, 30))
        # CpG positions are the even ones: a position has one context whatever read covers it
        xms.append("".join(("Z" if rng.random() < 0.5 else "z") if (st + j) % 2 == 0 and rng.random() < 0.8 else "." for j in range(L)))
        starts.append(st)
        strands.append(int(rng.integers(1, 3)))
    return H.templates_from_xm(xms, starts, strands)


def test_restatement_matches_closed_form_without_flanks():
    """flank_sites = 0: a pair is discordant when its two calls at the site differ, so npairs = c (c - 1) / 2,
    ndiscordant = meth * unmeth of the cytosine report's row, and qfdrp == fdrp (o = 1 for every pair)."""
    t = closed_form_templates()
    m = 64
    rep = fdrp_np.restate(t, "CG", flank_sites=0, max_reads=m, min_overlap=1, min_reads=2)
    s = rep["sites"]
    cov = (s["meth"] + s["unmeth"]).astype(np.int64)
    assert cov.max() <= m and (cov >= 2).sum() > 10 and len(set(s["strand"].tolist())) == 2
    want = cov >= 2
    for q in ("rname", "strand", "pos", "context"):
        assert np.array_equal(rep[q], s[q][want])
    c = cov[want]
    assert np.array_equal(rep["coverage"], c) and np.array_equal(rep["nreads"], c)
    assert np.array_equal(rep["npairs"], c * (c - 1) // 2)
    assert np.array_equal(rep["ndiscordant"], s["meth"][want].astype(np.int64) * s["unmeth"][want])
    assert rep["ndiscordant"].max() > 0
    assert np.array_equal(rep["qfdrp"], rep["fdrp"])
    assert np.array_equal(rep["fdrp"], rep["ndiscordant"].astype(np.float64) / rep["npairs"].astype(np.float64))


def test_selection_ranks():
    """floor(j c / m): all rows when c <= m, otherwise m distinct ranks spread from the first row on."""
    assert fdrp_np.selected_ranks(5, 7) == [0, 1, 2, 3, 4] and fdrp_np.selected_ranks(7, 7) == list(range(7))
    assert fdrp_np.selected_ranks(8, 7) == [0, 1, 2, 3, 4, 5, 6]
    assert fdrp_np.selected_ranks(100, 7) == [0, 14, 28, 42, 57, 71, 85]
    r = fdrp_np.selected_ranks(65, 64)
    assert r[0] == 0 and r[-1] == 63 and len(set(r)) == 64
    r = fdrp_np.selected_ranks(100, 40)
    assert r == [(5 * j) // 2 for j in range(40)] and len(set(r)) == 40


# ---- the indexed restatement, the seam batches and what the fuzz list reaches (no GPU) -------------------------------------------

def same_restatement(a, b, label):
    for q in fdrp_np.INT_COLS + fdrp_np.FLOAT_COLS:
        assert a[q].dtype == b[q].dtype and np.array_equal(a[q], b[q]), (label, q)
    assert a["used"] == b["used"], (label, "used")
    for q in a["sites"]:
        assert np.array_equal(a["sites"][q], b["sites"][q]), (label, "sites", q)


def test_indexed_restatement_equals_the_loop():
    """fdrp_np.restate_indexed (the covering rows of a site looked up, a row's calls counted from the row's first site)
    against fdrp_np.restate, column for column and in `used`: on the batches of test_gpu_fdrp.py with their arguments, on
    its five fuzz seeds and on five batches of the fuzz generator with the calls test_gpu_fuzz_fdrp.py draws for them"""
    import test_gpu_fdrp as TF
    import test_gpu_fuzz_fdrp as FF
    rng = np.random.default_rng
    cases = [("by hand", H.templates_from_xm(["Z.Z.Z", "Z.z.Z", "z.z.Z", "..Z.z"], [1, 1, 1, 1], [1, 1, 1, 1]), "CG", dict(flank_sites=1)),
             ("selection 100 / 7", TF.selection_batch(100), "CG", dict(max_reads=7)),
             ("selection 65 / 64", TF.selection_batch(65), "CG", dict(max_reads=64)),
             ("packing", TF.packing_batch(17), "CG", dict(flank_sites=31, max_reads=64)),
             ("packing, long rows", TF.packing_batch(19, step=9), "CG", dict(flank_sites=5, max_reads=9, min_overlap=3)),
             ("segments", TF.ragged(rng(29), 240, span=40, lmin=6, lmax=30, rnames=(1, 2), p_site=0.8), "CG", dict(flank_sites=3, max_reads=64)),
             ("gaps", TF.ragged(rng(31), 160, span=50, lmin=6, lmax=40, p_site=0.95, p_gap=0.25, other="xh-", p_other=0.3), "CG",
              dict(flank_sites=4, max_reads=64, min_overlap=5)),
             ("max_distance", TF.ragged(rng(37), 120, span=40, lmin=10, lmax=40, p_site=0.9), "CG", dict(flank_sites=4, max_reads=64, max_distance=4)),
             ("min_reads", TF.ragged(rng(41), 60, span=80, lmin=6, lmax=30, p_site=0.8), "CG", dict(flank_sites=3, max_reads=5, min_reads=3)),
             ("no kept row", H.templates_from_xm(["Z.z.HH", "z.Z.HH"], [1, 1], [1, 1]), "CG", {}),
             ("empty", H.templates_from_xm([], [], []), "CG", {})]
    names = {"W": "flank_sites", "m": "max_reads"}
    for seed in TF.FUZZ_SEEDS:
        t, ctx, kw = TF.fuzz_case(seed)
        cases.append(("fuzz %d" % seed, t, ctx, {names.get(k, k): v for k, v in kw.items()}))
    for seed in (1003, 1007, 1028, 1033, 9004):             # a pile, three sequences, long rows, flank_sites = 0, garbage and empty rows
        kind, t, calls = FF.plan(seed)
        cases.append(("fuzz batch %d" % seed, t, calls[0][0], dict(zip(("flank_sites", "max_reads", "min_overlap", "max_distance", "max_oo", "min_reads"),
                                                                      calls[0][1:]))))
    nonempty = 0
    for label, t, ctx, kw in cases:
        a, b = fdrp_np.restate(t, ctx, **kw), fdrp_np.restate_indexed(t, ctx, **kw)
        same_restatement(a, b, label)
        nonempty += a["pos"].size > 0
    assert nonempty >= len(cases) - 3


def test_seam_batches_hold_what_they_are_built_for():
    """The counts that test_gpu_fdrp_seams.py pins, on the cases whose restatement is quick (each *_want asserts its own:
    the site count, the coverage, the first and the last ordinal, the pair count, the deep site, the top of int32)"""
    import test_gpu_fdrp_seams as S
    for N in (1, 2, 256, 257):
        t, want = S.table_want(N, 8, 40)
        assert want["pos"].size == N
    for n in (4095, 4096, 4097):
        t, want = S.rows_want(n, False, 8, 40)
        assert t["start"].size == n and int(t["off"][-1]) <= 512 * n
    t, want = S.rows_want(5, True, 8, 40)
    assert int(t["off"][-1]) > 512 * 5 and want["pos"].size > 50
    for nc in (4095, 4096, 4097, 8193):
        S.pairs_want(nc)
    t, want, i = S.deep_want(4097, 40)
    assert want["coverage"][i] == 4097
    for which in ("pos", "rname"):
        S.end_want(which, 3)


def test_fuzz_fdrp_inputs_cover_the_shapes():
    """What the calls of test_gpu_fuzz_fdrp.py reach, from the restatement alone"""
    import test_gpu_fuzz_fdrp as FF
    TOP = 2 ** 31 - 1
    n = dict.fromkeys(("calls", "skipped", "discordant", "deep", "high", "long_row", "wide", "three_both", "capped"), 0)
    Ws, ms = set(), set()
    for seed in FF.SEEDS:
        kind, t, calls = FF.plan(seed)
        L = np.diff(t["off"])
        for call in calls:
            ctx, W, m, min_overlap, max_distance, max_oo, min_reads = call
            assert ctx in H.CONTEXT_TO_BASES and 0 <= W <= 31 and 2 <= m <= 64 and 1 <= min_overlap <= 2 * W + 1
            assert max_distance in FF.MAX_DISTANCE and 0 <= min_reads <= 5
            n["calls"] += 1
            Ws.add(W); ms.add(m)
            want = FF.fdrp_want(t, call)
            if want is None:
                n["skipped"] += 1
                continue
            nrow = want["pos"].size
            n["discordant"] += bool(nrow and want["ndiscordant"].max() > 0)
            n["deep"] += bool(nrow and want["coverage"].max() >= 256)
            n["high"] += bool(nrow and want["pos"].max() > TOP - 1000)
            n["long_row"] += bool(L.max() > 4000)
            n["wide"] += bool(int(t["off"][-1]) > 512 * L.size)
            n["three_both"] += bool(np.unique(t["rname"]).size == 3 and np.unique(want["rname"]).size == 3 and set(want["strand"].tolist()) >= {1, 2})
            n["capped"] += bool(nrow and np.any(want["nreads"] < want["coverage"]))
    print("FDRP calls %(calls)d: %(discordant)d with a discordant pair, %(deep)d with a site of 256 rows or more, %(high)d with a pos above "
          "2^31 - 1000, %(long_row)d on a batch with a row above 4000 bytes, %(wide)d on a batch with a mean row above 512 bytes, "
          "%(three_both)d on three sequences with both strands, %(capped)d with nreads < coverage, %(skipped)d skipped for size" % n,
          "flank_sites drawn %s, max_reads drawn %s" % (sorted(Ws), sorted(ms)))
    assert 20 * n["skipped"] <= n["calls"]
    assert 3 * n["discordant"] >= 2 * n["calls"]
    assert n["deep"] >= 1 and n["high"] >= 1 and n["long_row"] >= 1 and n["wide"] >= 1 and n["three_both"] >= 1 and n["capped"] >= 1
    assert {0, 31} <= Ws and {2, 64} <= ms
