"""generateAsmReport on the GPU (epi_batch_asm_report_dev, epi_batch_asm_fetch_dev) against the loop restatement of its
definitions (tests/asm_np.py): every integer column equal, beta_ref, beta_alt and delta_beta bit for bit, p bit-equal to
fisherExact on the cells and within the project's device-against-host bound of the host test -- on the hand cases, at the
seams of the workgroups and of a row, on both counter paths, on a deep pile-up, on the reference's fixtures end to end, under
every row layout, over several groups of sites, with errors, state and ownership pinned."""
import contextlib
import csv
import ctypes as C
import functools
import gc
import os

import numpy as np
import pytest

import asm_np as A
import cx_compare_np as X
import helpers as H
import test_asm_host as HOST
import test_gpu_cx_compare as T
import test_gpu_vcf as V

pytestmark = pytest.mark.gpu
LEVELS = ("chrA", "chrB", "chrC")
RTOL = T.RTOL                                              # profiles/cx_compare.txt: device against host Fisher p


@pytest.fixture(scope="module")
def ea():
    import epialleler_amd
    return epialleler_amd


@pytest.fixture
def hook_env(ea, monkeypatch):
    """EPIHIP_* test hooks inside this process (the library re-reads them after every change and after the restore)."""
    lib = ea._lib.load()

    def setenv(name, value):
        monkeypatch.setenv(name, value)
        lib.epi_options_reload()
    yield setenv
    monkeypatch.undo()
    lib.epi_options_reload()


def make(ea, t):
    return ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"], LEVELS)


def host_fisher(a, b, c, d):
    import epialleler_amd as ea
    return ea.rcpp_fep({"a": a, "b": b, "c": c, "d": d}, ("a", "b", "c", "d"), nthreads=4)


def same_tables(ea, got, want, label=""):
    """(pairs, snvs) of the GPU against the restatement's (with the host's p)"""
    for g, w, cols in zip(got, want, (A.PAIR_COLUMNS, A.SNV_COLUMNS)):
        assert list(g.keys()) == list(cols), label
        A.same(g, w, label)
        cells = np.stack([w[k] for k in A.CELLS], axis=1)
        na = np.isnan(w["p"])                                # (the SNV row of an NA site)
        dev = ea.fisherExact(*[w[k] for k in A.CELLS], as_device=True).cpu().numpy() if len(na) else np.zeros(0)
        assert np.array_equal(np.where(na, 0, g["p"]).view(np.uint64), np.where(na, 0, dev).view(np.uint64)), label
        X.compare_p(g["p"], w["p"], cells, RTOL)


def check(ea, t, sites, bam=None, label="", ctx="Zz", max_distance=0, min_coverage=1, max_oo=0.1, events=None):
    """rcpp_asm_report on the batch of t against the restatement -> the restatement's (pairs, snvs)"""
    own = bam is None
    bam = make(ea, t) if own else bam
    try:
        got = ea.rcpp_asm_report(bam, *sites, ctx, max_distance, min_coverage, max_oo)
    finally:
        if own:
            bam.close()
    want = A.restate(t, *sites, ctx, max_distance=max_distance, min_coverage=min_coverage, max_oo=max_oo, fisher=host_fisher, events=events)
    same_tables(ea, got, want, label)
    return want


# ---- 1. the hand cases ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(A.hand_cases()))
def test_hand_cases(ea, name):
    t, sites, kw = A.hand_cases()[name]
    pairs, snvs = check(ea, t, sites, label=name, **kw)
    assert len(pairs["snv"]) == {"coverage_1": 2, "coverage_2": 1, "coverage_3": 0, "two_alts": 4}.get(name, 2)


def test_site_at_a_rows_first_and_last_byte(ea):
    rows = [A.hand_row("zZ........Z", "A", at=0), A.hand_row("ZZ........z", "T", at=0), A.hand_row("Z.........Z", "A", at=10),
            A.hand_row("z........Zz", "T", at=10), A.hand_row("Z", "A", start=100, at=0), A.hand_row("z", "T", start=110, at=0)]
    sites = (np.asarray([1, 1, 1, 1], np.int32), np.asarray([99, 100, 110, 111], np.int32), np.asarray([A.A_T] * 4, np.int32))
    pairs, snvs = check(ea, A.hand_templates(rows), sites)
    assert snvs["reads_ref"].tolist() == [0, 2, 1, 0] and snvs["reads_alt"].tolist() == [0, 1, 2, 0]
    assert snvs["reads_other"].tolist() == [0, 2, 2, 0]      # (the rows whose C is at the other end)
    assert pairs["snv"].tolist().count(1) >= 1 and pairs["snv"].tolist().count(2) >= 1


# ---- 2. seams, both counter paths, a pile-up ---------------------------------------------------------------------------------

def random_case(seed, nrow, length, span, site_pos, nseq=1, long_rows=0, call_share=0.4):
    """nrow rows of `length` bases with ragged starts in [1, span] (long_rows of them 10 kb), letters Z z and '.', the bases at
    the sites mostly REF or ALT of the site's pair"""
    rng = np.random.default_rng(seed)
    starts = np.sort(rng.integers(1, span + 1, nrow))
    rn = np.sort(rng.integers(1, nseq + 1, nrow))
    pairs_ = [A.REF_ALT[int(k)] for k in rng.integers(0, 12, len(site_pos))]
    chr_ = np.sort(rng.integers(1, nseq + 1, len(site_pos)))
    letters, bases = np.frombuffer(b"Zz.", np.uint8), np.frombuffer(b"ACGT", np.uint8)
    xms, seqs = [], []
    for x in range(nrow):
        n = 10000 if x < long_rows else length
        share = 0.1 if x < long_rows else call_share
        xm = letters[rng.choice(3, n, p=(share / 2, share / 2, 1 - share))]
        sq = bases[rng.integers(0, 4, n)].copy()
        for k, p in enumerate(site_pos):
            i = int(p) - int(starts[x])
            if chr_[k] == rn[x] and 0 <= i < n and rng.random() < 0.9:
                sq[i] = ord(pairs_[k][int(rng.integers(0, 2))])
        xms.append(xm.tobytes().decode())
        seqs.append(sq.tobytes().decode())
    t = A.templates(xms, seqs, starts.tolist(), rng.integers(1, 3, nrow).tolist(), rn.tolist())
    masks = np.asarray([A.mask_of(r, a) for r, a in pairs_], np.int32)
    return t, (chr_.astype(np.int32), np.asarray(site_pos, np.int32), masks)


@pytest.mark.parametrize("nrow", [257, 513])
def test_sites_on_workgroup_seams(ea, nrow):
    """Rows 255 / 256 (and 511 / 512) of the batch cover the same sites: neighbouring workgroups add to one site's counters"""
    t, sites = random_case(nrow, nrow, 40, 60, [20, 45, 45, 61, 70, 99])
    assert t["start"][254] <= 61 <= t["start"][257 - 1] + 39
    pairs, snvs = check(ea, t, sites, max_oo=1.0)
    assert len(pairs["snv"]) > 20 and (snvs["reads_ref"] + snvs["reads_alt"]).max() > 100
    check(ea, t, sites, max_oo=1.0, max_distance=7, min_coverage=3)


def test_window_beyond_the_lds_counters(ea):
    """Three 10 kb rows over 400 sites among 60 short ones: the workgroup's window holds more than 256 sites"""
    pos = np.sort(np.random.default_rng(5).choice(np.arange(30, 9900), 400, replace=False))
    t, sites = random_case(77, 63, 50, 30, pos, long_rows=3)
    assert np.diff(t["off"]).max() == 10000
    pairs, snvs = check(ea, t, sites, max_oo=1.0)
    assert (snvs["reads_ref"] + snvs["reads_alt"] > 0).sum() > 256 and len(pairs["snv"]) > 1000
    check(ea, t, sites, max_oo=1.0, max_distance=100)


def test_deep_pile_up_on_one_snv(ea):
    t, sites = random_case(9, 5000, 60, 50, [55])
    pairs, snvs = check(ea, t, sites, max_oo=1.0)
    assert snvs["reads_ref"][0] + snvs["reads_alt"][0] > 2000 and snvs["npairs"][0] > 80 and pairs["meth_ref"].max() > 100


def test_row_layouts(ea):
    t, sites = random_case(21, 700, 90, 400, [50, 120, 121, 300, 444], nseq=2)
    want = A.restate(t, *sites, "Zz", max_oo=1.0, fisher=host_fisher)
    assert len(want[0]["snv"]) > 50
    seen = []
    for layout, bam in V._bams(ea, t):
        same_tables(ea, ea.rcpp_asm_report(bam, *sites, "Zz", 0, 1, 1.0), want, layout)
        seen.append((layout, ea._lib.load().epi_batch_layout(bam.batch())))
        bam.close()
    assert seen == [("uploaded", 16), ("adopted", 0), ("realigned", 16)]


def test_sites_in_any_order_with_na(ea):
    """rcpp_asm_report sorts the sites for the device: the pair rows come in (rname, snv_pos) order of the sites, equal
    positions in the order given, and `snv` and the SNV rows follow the order given"""
    t, (chr_, pos, masks) = random_case(22, 300, 80, 200, [40, 90, 90, 150, 222])
    perm = np.asarray([3, 0, 4, 1, 2])
    sites = (chr_[perm].copy(), pos[perm], masks[perm])
    sites[0][2] = A.NA_INT
    want_p, want_s = A.restate(t, *sites, "Zz", max_oo=1.0, fisher=host_fisher)      # rows by the index given
    order = np.lexsort((want_p["context"], want_p["strand"], want_p["pos"], want_p["snv"], want_p["snv_pos"], want_p["rname"]))
    want_p = {k: v[order] for k, v in want_p.items()}
    bam = make(ea, t)
    try:
        got = ea.rcpp_asm_report(bam, *sites, "Zz", 0, 1, 1.0)
    finally:
        bam.close()
    same_tables(ea, got, (want_p, want_s), "any order")
    assert want_s["rname"][2] == A.NA_INT and want_s["npairs"].tolist()[2] == 0 and min(want_s["npairs"][[0, 1, 3, 4]]) > 40
    assert [s for i, s in enumerate(want_p["snv"].tolist()) if i == 0 or s != want_p["snv"][i - 1]] == [1, 3, 4, 0]


# ---- 3. the fixtures, end to end ----------------------------------------------------------------------------------------------

FIXTURES = {"amplicon": dict(bam="amplicon010meth.bam", vcf="amplicon.vcf.gz", bed="amplicon.bed", vcf_style="NCBI"),
            "capture": dict(bam="capture.bam", vcf="capture.vcf.gz", bed="capture.bed", vcf_style=None)}


@functools.lru_cache(maxsize=None)
def fixture_want(which):
    t, sites, v = HOST.fixture_sites(which)
    return A.restate(t, *sites, "Zz", fisher=host_fisher), v


@pytest.mark.parametrize("which", ["amplicon", "capture"])
def test_fixtures(ea, which, tmp_path):
    f = FIXTURES[which]
    arg = dict(vcf_style=f["vcf_style"], bed=os.path.join(H.GOLDEN, "bam", f["bed"]))
    bam, vcf = os.path.join(H.GOLDEN, "bam", f["bam"]), os.path.join(H.GOLDEN, "vcf", f["vcf"])
    pb = ea.preprocessBam(bam)
    (want_p, want_s), v = fixture_want(which)
    pairs = ea.generateAsmReport(pb, vcf, **arg)
    snvs = ea.generateAsmSnvReport(pb, vcf, **arg)
    assert list(pairs.keys()) == list(ea.ASM_COLUMNS) and list(snvs.keys()) == list(ea.ASM_SNV_COLUMNS)
    same_tables(ea, ({k: pairs[k] for k in A.PAIR_COLUMNS}, {k: snvs[k] for k in A.SNV_COLUMNS}), (want_p, want_s), which)
    assert snvs["name"].tolist() == v.names.tolist() and snvs["REF"].tolist() == v.ref.tolist() and snvs["ALT"].tolist() == v.alt.tolist()
    assert pairs["name"].tolist() == v.names[want_p["snv"]].tolist() and pairs["ALT"].tolist() == v.alt[want_p["snv"]].tolist()
    assert pairs.levels["rname"] == pb.levels
    assert pairs.nrow == (181 if which == "amplicon" else 0) and snvs.nrow == (56 if which == "amplicon" else 26292)
    dev = ea.generateAsmReport(pb, vcf, as_device=True, **arg)
    assert list(dev.keys()) == list(A.PAIR_COLUMNS) and all(c.is_cuda for c in dev.values())
    A.same({k: c.cpu().numpy() for k, c in dev.items()}, want_p, "device table")
    out = tmp_path / "asm.tsv"
    assert ea.generateAsmReport(pb, vcf, report_file=str(out), **arg) is None
    with open(out) as fh:
        rows = list(csv.reader(fh, delimiter="\t"))
    assert rows[0] == list(ea.ASM_COLUMNS) and len(rows) == 1 + pairs.nrow
    if which == "amplicon":
        assert [r[0] for r in rows[1:]] == pairs["name"].tolist() and [int(r[7]) for r in rows[1:]] == pairs["pos"].tolist()
        assert rows[1][4] == pb.levels[pairs["rname"][0] - 1] and rows[1][6] in "+-" and rows[1][8] == "CG"
        adj = ea.adjustReport(pairs, column="p")
        assert np.allclose(adj["q"], ea.adjustPValues(pairs["p"])) and list(adj.keys()) == list(ea.ASM_COLUMNS) + ["q"]
        loose = ea.generateAsmReport(pb, vcf, asm_context="CX", max_outofcontext_beta=1.0, min_coverage=0, **arg)
        assert loose.nrow == 991
        assert ea.generateAsmReport(pb, vcf, max_distance=10, **arg).nrow == int((np.abs(want_p["pos"] - want_p["snv_pos"]) <= 10).sum())
        with pytest.raises(ValueError, match="seqlevels styles"):        # generateVcfReport's error: the VCF says 17, the BAM chr17
            ea.generateAsmReport(pb, vcf, vcf_style="NCBI", bed=None)


# ---- 4. groups of sites ---------------------------------------------------------------------------------------------------------

def test_site_groups(ea, hook_env):
    """A cap under the largest site's events: that site runs alone, its neighbours form groups (at least three); and a cap of
    one event: every site alone.  The tables are those of the ungrouped run."""
    t, sites = random_case(31, 600, 70, 500, [30, 80, 81, 140, 200, 260, 300, 301, 390, 450, 520])
    events = []
    want = check(ea, t, sites, max_oo=1.0, events=events)
    lib = ea._lib.load()
    nbytes = C.c_int64(0)
    assert lib.epi_asm_event_bytes(max(events) - 1, C.byref(nbytes)) == 0
    groups, cur = [], None                                   # the grouping rule of the header, restated
    for s, e in enumerate(events):
        if cur is not None and 24 * (cur[1] + e) <= nbytes.value:
            cur[0].append(s)
            cur[1] += e
        else:
            cur = [[s], e]
            groups.append(cur)
    big = int(np.argmax(events))
    assert len(groups) >= 3 and [big] in [g[0] for g in groups] and 24 * events[big] > nbytes.value and max(len(g[0]) for g in groups) >= 2
    bam = make(ea, t)
    try:
        for cap in (nbytes.value, 24):
            hook_env("EPIHIP_ASM_GROUP_BYTES", str(cap))
            same_tables(ea, ea.rcpp_asm_report(bam, *sites, "Zz", 0, 1, 1.0), want, "cap %d" % cap)
    finally:
        bam.close()


# ---- 5. errors, state and ownership -------------------------------------------------------------------------------------------

def allocations(ea):
    live, nbytes = C.c_int64(-1), C.c_int64(-1)
    ea._lib.check(ea._lib.load().epi_device_allocations(C.byref(live), C.byref(nbytes)))
    return live.value, nbytes.value


@contextlib.contextmanager
def nothing_left(ea):
    gc.collect()
    before = allocations(ea)
    yield
    gc.collect()
    assert allocations(ea) == before


def raw_report(ea, bam, sites, max_distance=0, min_coverage=1, fill=-7):
    """epi_batch_asm_report_dev on SNV columns filled with a sentinel -> (return code, pair rows, the columns)"""
    import torch
    from epialleler_amd.api import _ptr_array, _stream
    dev = "cuda:%d" % bam.device
    d = [torch.tensor(np.asarray(a, np.int32), device=dev) for a in sites]
    n = len(sites[0])
    icols = list(torch.full((10, n), fill, dtype=torch.int32, device=dev).unbind(0))
    dcols = list(torch.full((4, n), float(fill), dtype=torch.float64, device=dev).unbind(0))
    npair = C.c_int64(-1)
    rc = ea._lib.load().epi_batch_asm_report_dev(bam.batch(), *[C.c_void_p(x.data_ptr()) if n else None for x in d], n, b"Zz", max_distance,
                                                 min_coverage, 1.0, _ptr_array(icols), _ptr_array(dcols), _stream(bam.device), C.byref(npair))
    torch.cuda.synchronize()
    return rc, npair.value, [c.cpu().numpy() for c in icols + dcols]


def raw_fetch(ea, bam, n):
    import torch
    from epialleler_amd.api import _ptr_array, _stream
    dev = "cuda:%d" % bam.device
    icols = list(torch.empty((10, n), dtype=torch.int32, device=dev).unbind(0))
    dcols = list(torch.empty((4, n), dtype=torch.float64, device=dev).unbind(0))
    rc = ea._lib.load().epi_batch_asm_fetch_dev(bam.batch(), _ptr_array(icols), _ptr_array(dcols), _stream(bam.device))
    torch.cuda.synchronize()
    return rc, dict(zip(A.PAIR_COLUMNS, [c.cpu().numpy() for c in icols + dcols]))


def test_errors_state_and_ownership(ea):
    E = ea._lib
    with nothing_left(ea):
        t, sites = random_case(41, 300, 80, 300, [40, 90, 90, 150, 222, 305])
        want_p, want_s = A.restate(t, *sites, "Zz", max_oo=1.0)
        assert len(want_p["snv"]) > 30
        bam = make(ea, t)
        unsorted = make(ea, dict(t, start=t["start"][::-1].copy()))
        empty = make(ea, A.templates([], [], [], []))
        try:
            for x in (bam, unsorted, empty):
                x.batch()
            rc, _ = raw_fetch(ea, bam, 1)                    # a fetch before any report
            assert rc == E.EPI_ERR_STATE and b"no allele-specific methylation report" in E.load().epi_last_error()
            rc, npair, cols = raw_report(ea, bam, sites)
            assert rc == E.EPI_OK and npair == len(want_p["snv"]) and not np.any(cols[0] == -7)
            A.same(dict(zip(A.SNV_COLUMNS, cols)), want_s)
            rc, got = raw_fetch(ea, bam, npair)
            assert rc == E.EPI_OK
            A.same(got, want_p)
            # the sites out of order; a mask with a bit above 15; REF and ALT of '-' sharing a base: nothing is counted or written
            swapped = tuple(a[[1, 0, 2, 3, 4, 5]] for a in sites)
            rc, npair, cols = raw_report(ea, bam, swapped)
            assert rc == E.EPI_ERR_UNSORTED and b"VCF sites are not sorted" in E.load().epi_last_error() and all(np.all(c == -7) for c in cols)
            for bad in (1 << 16, 0x2200):
                masks = sites[2].copy()
                masks[3] = bad
                rc, npair, cols = raw_report(ea, bam, (sites[0], sites[1], masks))
                assert rc == E.EPI_ERR_ARG and b"site 3" in E.load().epi_last_error() and all(np.all(c == -7) for c in cols)
            for kw in (dict(max_distance=-1), dict(min_coverage=-1)):
                rc, npair, cols = raw_report(ea, bam, sites, **kw)
                assert rc == E.EPI_ERR_ARG and list(kw)[0].encode() in E.load().epi_last_error() and all(np.all(c == -7) for c in cols)
            rc, npair, cols = raw_report(ea, unsorted, sites)
            assert rc == E.EPI_ERR_UNSORTED and b"PRE-SORTED" in E.load().epi_last_error() and all(np.all(c == -7) for c in cols)
            # no site: an empty pair table, also for the fetch; no row: SNV rows of zeros
            rc, npair, cols = raw_report(ea, bam, (sites[0][:0], sites[1][:0], sites[2][:0]))
            assert rc == E.EPI_OK and npair == 0 and raw_fetch(ea, bam, 0)[0] == E.EPI_OK
            rc, npair, cols = raw_report(ea, empty, sites)
            assert rc == E.EPI_OK and npair == 0 and np.array_equal(cols[1], sites[1]) and all(np.all(c == 0) for c in cols[2:10])
            assert all(np.all(np.isnan(c)) for c in cols[10:13]) and np.all(cols[13] == 1.0)
            p, s = ea.rcpp_asm_report(empty, *sites, "Zz", 0, 1, 0.1)
            assert p["snv"].shape == (0,) and s["reads_ref"].tolist() == [0] * 6
            p, s = ea.rcpp_asm_report(bam, [], [], [], "Zz", 0, 1, 0.1)
            assert list(p.keys()) == list(A.PAIR_COLUMNS) and p["p"].shape == (0,) and s["rname"].shape == (0,)
        finally:
            bam.close()
            unsorted.close()
            empty.close()


def test_other_reports_are_left_alone(ea):
    """CX -> ASM -> CX fetch -> lMHL -> ASM -> lMHL fetch: every fetch reads what its report left"""
    import torch
    from epialleler_amd.api import _ptr_array, _stream
    lib = ea._lib.load()
    t, sites = random_case(51, 400, 80, 300, [40, 90, 150, 222])
    fresh = make(ea, t)
    want_cx = ea.rcpp_cx_report(fresh, None, "Z")
    want_mhl = ea.rcpp_mhl_report(fresh, "Zz", 0, 0, 1.0)
    fresh.close()
    want_asm = A.restate(t, *sites, "Zz", max_oo=1.0, fisher=host_fisher)
    with nothing_left(ea):
        bam = make(ea, t)
        b, st = bam.batch(), _stream(bam.device)
        nrow = C.c_int64(0)
        ea._lib.check(lib.epi_batch_cx_report_dev(b, None, b"Z", st, C.byref(nrow)))
        same_tables(ea, ea.rcpp_asm_report(bam, *sites, "Zz", 0, 1, 1.0), want_asm, "after CX")
        assert nrow.value == want_cx.nrow
        cols = list(torch.empty((6, nrow.value), dtype=torch.int32, device="cuda:0").unbind(0))
        ea._lib.check(lib.epi_batch_cx_fetch_dev(b, _ptr_array(cols), st))
        for k, c in zip(ea.api.CX_COLUMNS, cols):
            assert np.array_equal(c.cpu().numpy(), want_cx[k]), k
        ea._lib.check(lib.epi_batch_mhl_report_dev(b, b"Zz", 0, 0, 1.0, st, C.byref(nrow)))
        rc, got = raw_fetch(ea, bam, len(want_asm[0]["snv"]))     # the pair table outlives the lMHL report
        assert rc == 0
        A.same(got, want_asm[0])
        same_tables(ea, ea.rcpp_asm_report(bam, *sites, "Zz", 0, 1, 1.0), want_asm, "after lMHL")
        icols = list(torch.empty((5, nrow.value), dtype=torch.int32, device="cuda:0").unbind(0))
        dcols = list(torch.empty((2, nrow.value), dtype=torch.float64, device="cuda:0").unbind(0))
        ea._lib.check(lib.epi_batch_mhl_fetch_dev(b, _ptr_array(icols), _ptr_array(dcols), st))
        for k, c in zip(ea.api.MHL_COLUMNS, icols + dcols):
            assert np.array_equal(c.cpu().numpy(), want_mhl[k], equal_nan=True), k
        bam.close()
