"""Who owns the library's device buffers (csrc/common.hpp: DevBuf frees itself; include/epihip.h:
epi_device_allocations).  Every case reads the process-wide counter of live allocations and their bytes, does its work,
closes what it opened and finds both figures exactly where they were: a batch that is freed, a communicator that is freed
and a call that has returned -- with a result or with an error -- hold nothing.  torch's tensors and the engines' staging
buffers are not the library's device buffers and are not counted."""
import contextlib
import ctypes as C
import gc
import os

import numpy as np
import pytest

import cx_compare_np as X
import helpers as H
import padjust_np as P
import synth_np

pytestmark = pytest.mark.gpu

BAMS = os.path.join(H.GOLDEN, "bam")
LEVELS = ("chrA", "chrB")
C2B = H.CONTEXT_TO_BASES


@pytest.fixture(scope="module")
def ea():
    import epialleler_amd
    return epialleler_amd


def allocations(ea):
    live, nbytes = C.c_int64(-1), C.c_int64(-1)
    ea._lib.check(ea._lib.load().epi_device_allocations(C.byref(live), C.byref(nbytes)))
    return live.value, nbytes.value


@contextlib.contextmanager
def nothing_left(ea):
    """The counter behind the block is the counter in front of it, exactly.  (Batches that earlier tests dropped without
    closing are collected first, so that none of them goes inside the block.)"""
    gc.collect()
    before = allocations(ea)
    yield before
    gc.collect()
    assert allocations(ea) == before


def rows(seed=5, n=400):
    """A few hundred ragged templates on two sequences, any XM letters"""
    return synth_np.random_templates(np.random.default_rng(seed), n, 20, 200, 2, 3000)


def cpg_rows(seed):
    """300 templates of 80 bases with a CpG every 6 bases: windows, pairs and read pairs for the site-table reports"""
    rng = np.random.default_rng(seed)
    xms, starts = [], []
    for _ in range(300):
        st = int(rng.integers(1, 800))
        xms.append("".join(("Z" if rng.random() < 0.4 else "z") if pos % 6 == 0 else "." for pos in range(st, st + 80)))
        starts.append(st)
    return H.templates_from_xm(xms, starts, rng.integers(1, 3, 300).tolist(), rng.integers(1, 3, 300).tolist())


def make(ea, t):
    return ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"], LEVELS)


@contextlib.contextmanager
def batch_of(ea, t):
    """batch(), the block, close() -- with the counter checked around all three"""
    with nothing_left(ea) as before:
        bam = make(ea, t)
        bam.batch()
        assert allocations(ea)[0] > before[0]              # (the counter does count: the batch's columns)
        try:
            yield bam
        finally:
            bam.close()


# ---- batch lifecycle, one case per family ---------------------------------------------------------------------------------

def test_cx_report_pool_then_direct(ea):
    import test_gpu_cx_direct as D
    t = D.segments_batch(3, [(1, 2, 3), (2, 0, 2)], 1024)
    with batch_of(ea, t) as bam:
        first, w1 = D.report(ea, bam, "CG", False)
        second, w2 = D.report(ea, bam, "CG", False)
        assert (w1, w2) == (False, True) and first["pos"].size > 0
        H.assert_reports_equal(first, second)


def test_fused_cytosine_report_with_pass(ea):
    c = C2B["CG"]
    with batch_of(ea, rows()) as bam:
        rep, p = ea.cytosine_report_fused(bam, c["ctx_meth"], c["ctx_unmeth"], c["ooctx_meth"], c["ooctx_unmeth"], 2, 0.5, 0.1, "Z",
                                          return_pass=True)
        assert p.shape == (bam.n,) and rep.nrow > 0


@pytest.mark.parametrize("ctx", ["Zz", "ZzXx"])
def test_mhl_report(ea, ctx):
    """"Zz": the one-pass kernel; "ZzXx": the two-kernel path"""
    with batch_of(ea, cpg_rows(8)) as bam:
        assert ea.rcpp_mhl_report(bam, ctx, 0, 0, 0.1).nrow > 0


def test_heterogeneity_with_counts(ea):
    with batch_of(ea, cpg_rows(1)) as bam:
        rep = ea.rcpp_heterogeneity_report(bam, "Zz", 3, 0.1, with_counts=True)
        assert rep.nrow > 0 and rep.counts.shape == (rep.nrow, 8)


def test_linkage_and_blocks(ea):
    with batch_of(ea, cpg_rows(2)) as bam:
        assert ea.rcpp_linkage_report(bam, "Zz", 3, 0, 0.1).nrow > 0
        ea.rcpp_linkage_blocks(bam, "Zz", 3, 0, 0.1, 2, 0.0, 2)


def test_heterogeneity_compare(ea):
    with nothing_left(ea):
        a, b = make(ea, cpg_rows(3)), make(ea, cpg_rows(4))
        try:
            assert ea.rcpp_heterogeneity_compare(a, b, "Zz", 3, 0.1).nrow > 0
        finally:
            a.close()
            b.close()


def test_fdrp(ea):
    with batch_of(ea, cpg_rows(5)) as bam:
        assert ea.rcpp_fdrp_report(bam, "Zz", 4, 40, 1, 0, 0.1).nrow > 0


def test_per_read_calls(ea):
    c = C2B["CG"]
    with batch_of(ea, rows()) as bam:
        assert np.asarray(ea.rcpp_get_xm_beta(bam, "Z", "z")).shape == (bam.n,)
        p = ea.rcpp_threshold_reads(bam, c["ctx_meth"], c["ctx_unmeth"], c["ooctx_meth"], c["ooctx_unmeth"], 2, 0.5, 0.1)
        assert np.asarray(p).shape == (bam.n,)


def test_base_frequencies(ea):
    """epi_batch_base_freqs_dev keeps the sites' sortedness verdict in epi_batch::bf_flag, which the hand-kept list of
    buffers that epi_batch_free released before DevBuf had a destructor did not name: there, this case ends one
    allocation above where it began."""
    t = rows()
    with batch_of(ea, t) as bam:
        freqs = ea.rcpp_get_base_freqs(bam, None, np.asarray([1, 1, 2], np.int32), np.asarray([500, 1500, 1000], np.int32))
        assert freqs.shape == (3, 20) and freqs.sum() > 0


def test_match_target(ea):
    from epialleler_amd import bed as B
    with batch_of(ea, rows()) as bam:
        bed = ea.Bed(["chrA", "chrB", "chrZ"], [100, 1000, 1], [900, 2500, 10])
        m = B._match_target(bam, bed, "capture", -7, 1)
        assert m.shape == (bam.n,)


def test_patterns_multi(ea):
    with batch_of(ea, rows()) as bam:
        targets = [(1, 200, 900), (2, 1000, 1800)]
        assert len(ea.rcpp_extract_patterns_multi(bam, targets, 1, "Zz", 0.0, False, 0)) == 2
        assert len(ea.rcpp_summarise_patterns_multi(bam, targets, 1, "Zz", 0.0, False, 0)) == 2


def test_sharded_reports_world_of_one(ea):
    """A communicator of world size 1 (no id: nothing to exchange, RCCL is not loaded) with the test hook that treats five
    tiles in the middle of the batch as shared: slabs, shard plans, both halves of the reports, in this process."""
    from epialleler_amd import distributed as D
    t = synth_np.generate(n_total=600, read_len=300, n_chr=2)
    with nothing_left(ea):
        bam = make(ea, t)
        eng = D.HipShardEngine(bam)
        h = C.c_void_p()
        ea._lib.check(eng.lib.epi_comm_create(ea.api._engine(bam.device), None, 0, 1, C.byref(h)))
        eng.comm = h
        eng.lib.epi_comm_set_test_shared(h, 5)
        try:
            for _ in range(2):                              # (the second round runs on the remembered plans)
                assert D.sharded_cx_report(eng, None, "Z", gather=False)["pos"].numel() > 0
                assert D.sharded_mhl_report(eng, "Zz", 0, 0, 0.1, gather=False)["pos"].numel() > 0
                assert D.sharded_mhl_report(eng, "ZzXx", 0, 0, 0.1, gather=False)["pos"].numel() > 0
        finally:
            eng.close_comm()
            bam.close()


# ---- adopted batches --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("realign", [True, False])
def test_adopted_batch(ea, realign):
    import torch
    t = rows()
    nb = int(t["off"][-1])
    xm = torch.full(((nb + 15) // 16 * 16 + 64,), 0xFB, dtype=torch.uint8, device="cuda:0")
    xm[:nb] = torch.from_numpy(t["xm"]).cuda()
    dev = {k: torch.from_numpy(t[k]).cuda() for k in ("off", "rname", "strand", "start")}
    with nothing_left(ea):
        bam = ea.ProcessedBam.from_device(xm, nb, dev["off"], dev["rname"], dev["strand"], dev["start"], realign=realign)
        try:
            assert ea.rcpp_cx_report(bam, None, "Z").nrow > 0
            assert ea._lib.load().epi_batch_layout(bam.batch()) == (16 if realign else 0)
        finally:
            bam.close()


# ---- call-scoped scratch ----------------------------------------------------------------------------------------------------

def dev_report(ea, t, names):
    import torch
    return ea.Report({k: torch.from_numpy(np.ascontiguousarray(t[k])).cuda() for k in names}, LEVELS)


def test_cx_compare_and_regions(ea):
    rng = np.random.default_rng(8)
    a, b = (dev_report(ea, X.random_cx(rng, 300, 400), X.CX) for _ in range(2))
    table = dev_report(ea, X.random_comparison(np.random.default_rng(5), 300), X.CMP_INT + X.CMP_FLOAT)
    with nothing_left(ea):
        assert ea.rcpp_cx_compare(a, b, 1, as_device=True).ncommon > 0
        assert ea.rcpp_cx_compare_regions(table, 0.05, 0.1, 300, 1).nrow > 0


def test_cx_compare_of_two_batches(ea):
    with nothing_left(ea):
        a, b = make(ea, cpg_rows(6)), make(ea, cpg_rows(7))
        try:
            reps = [ea.rcpp_cx_report(x, None, "Z", as_device=True) for x in (a, b)]
            cmp_ = ea.rcpp_cx_compare(reps[0], reps[1], 1, as_device=True)
            assert cmp_.nrow > 0
            ea.rcpp_cx_compare_regions(cmp_, 0.5, 0.0, 300, 1)
        finally:
            a.close()
            b.close()


def test_adjust_p_values_and_fisher(ea):
    rng = np.random.default_rng(9)
    with nothing_left(ea):
        assert ea.adjustPValues(rng.random(500), "BH").shape == (500,)
        t = rng.integers(0, 12, (200, 4))
        assert ea.fisherExact(t[:, 0], t[:, 1], t[:, 2], t[:, 3]).shape == (200,)


def test_simulate_bam(ea, tmp_path):
    with nothing_left(ea):
        n = ea.simulateBam(str(tmp_path / "s.bam"), seed=1, pos=1, cigar="100M", tlen=100, XM=["z" * 50 + "Z" * 50] * 20)
        assert n == 20


def test_preprocess_mates_anywhere(ea):
    with nothing_left(ea):
        assert ea.preprocessBam(os.path.join(BAMS, "dragen-pe-unsort-xg-xm.bam"), mates="anywhere").n > 0


def test_preprocess_with_genome(ea):
    with nothing_left(ea):
        bam = ea.preprocessBam(os.path.join(BAMS, "dragen-pe-namesort-xg.bam"), genome=os.path.join(BAMS, "reference.fasta.gz"))
        assert bam.n > 0 and bam.ncalled > 0


# ---- error returns after scratch exists ---------------------------------------------------------------------------------------

def test_error_in_p_adjust(ea):
    """(the value outside [0, 1] is found by the first kernel, after the call's arena has been allocated)"""
    with nothing_left(ea):
        with pytest.raises(ea.EpihipError) as ei:
            ea.adjustPValues([0.1, 2.0])
        assert ei.value.code == ea._lib.EPI_ERR_ARG


def test_error_in_cx_compare(ea):
    base = X.cx_table([(1, 1, 10 * i, 3, 4, 4) for i in range(1, 7)])
    swapped = {k: v[[0, 2, 1, 3, 4, 5]] for k, v in base.items()}
    a, b = dev_report(ea, swapped, X.CX), dev_report(ea, base, X.CX)
    with nothing_left(ea):
        with pytest.raises(ea.EpihipError) as ei:
            ea.rcpp_cx_compare(a, b, 1)
        assert ei.value.code == ea._lib.EPI_ERR_ARG


def test_error_on_unsorted_rows(ea):
    t = rows()
    t = dict(t, start=t["start"][::-1].copy())
    with batch_of(ea, t) as bam:
        with pytest.raises(ea.EpihipError) as ei:
            ea.rcpp_cx_report(bam, None, "Z")
        assert ei.value.code == ea._lib.EPI_ERR_UNSORTED


# ---- the view form ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 255, 256, 257, 70000])
def test_p_adjust_on_views(ea, n):
    """adjustPValues is the one user of DevBuf::view: the scratch of its sort's scan and of its scan of doubles are pieces of
    the call's arena.  A piece smaller than what the callee asks for would come back as EPI_ERR_STATE; the results agree bit
    for bit with the restatement, as in test_gpu_p_adjust.py."""
    rng = np.random.default_rng(1000 + n)
    p = np.where(rng.random(n) < 0.1, np.nan, rng.random(n))
    with nothing_left(ea):
        for method in P.METHODS:
            np.testing.assert_array_equal(ea.adjustPValues(p, method), P.adjust_np(p, method)[0], err_msg=method)
