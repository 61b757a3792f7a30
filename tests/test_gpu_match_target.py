"""k_match_target (csrc/match_target.hip) behind bed._match_target and the C ABI, against the plain restatement
helpers.match_target_np (src/rcpp_match_target.cpp:16-81 in int64 numpy) on a synthetic batch of 3001 templates and an
unsorted BED of 2500 rows -- more rows than one LDS chunk of 1024, so the staging loop runs three times with a partial
last chunk, and many reads fit several rows, so 'the first fitting row' differs from 'a fitting row'.  Every comparison is
exact.  tests/test_bed_host.py checks the restatement itself (against the two nested loops) and the synthetic case
(matches in all three chunks, reads that fit several rows) without a device."""
import ctypes as C

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu
NA = H.NA_INT
GRID = [(False, p) for p in H.MATCH_AMPLICON] + [(True, p) for p in H.MATCH_CAPTURE]
EDGE = ((False, 2), (True, 1))                             # one interior parameter per kernel for the size sweeps


@pytest.fixture(scope="module")
def ea():
    import epialleler_amd
    return epialleler_amd


def _layouts(ea, t, levels=H.MATCH_LEVELS):
    """The batch uploaded from host arrays, adopted from device tensors, and adopted + realigned (as _bams in
    test_gpu_vcf.py)."""
    import torch
    yield "uploaded", ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"], levels)
    nb = int(t["off"][-1])
    for realign in (False, True):
        xm = torch.full(((nb + 15) // 16 * 16 + 16,), 0xFB, dtype=torch.uint8, device="cuda:0")
        xm[:nb] = torch.from_numpy(t["xm"]).cuda()
        yield ("realigned" if realign else "adopted"), ea.ProcessedBam.from_device(
            xm, nb, torch.from_numpy(t["off"]).cuda(), torch.from_numpy(t["rname"]).cuda(),
            torch.from_numpy(t["strand"]).cuda(), torch.from_numpy(t["start"]).cuda(), levels, realign=realign)


@pytest.fixture(scope="module")
def bams(ea):
    out = dict(_layouts(ea, H.match_templates()))
    yield out
    for b in out.values():
        b.close()


def _bed(ea, nbed=None):
    names, _, start, end = H.match_bed()
    nbed = len(names) if nbed is None else nbed
    return ea.Bed(names[:nbed], start[:nbed], end[:nbed])


def _match(bam, bed, capture, param):
    from epialleler_amd import bed as B
    # (the parameter of the other bed type gets a value that would change the result if it were the one used)
    got = B._match_target(bam, bed, "capture" if capture else "amplicon", -7 if capture else param, param if capture else 77)
    got = got.cpu().numpy()
    assert got.dtype == np.int32
    return got


def _want(t, bed, capture, param):
    return H.match_target_np(t, (H.match_codes(bed.chrom), bed.start, bed.end), capture, param)


def test_design_holds_for_the_restatement():
    H.assert_match_design()


@pytest.mark.parametrize("capture,param", GRID)
def test_grid_on_every_layout(ea, bams, capture, param):
    want = H.match_want(capture, param)[0]
    if param in H.MATCH_INTERIOR[capture]:
        assert 0 < np.mean(want > 0) < 1
    bed = _bed(ea)
    for layout, bam in bams.items():
        got = _match(bam, bed, capture, param)
        assert np.array_equal(got, want), (layout, int(np.sum(got != want)), np.flatnonzero(got != want)[:5])


@pytest.mark.parametrize("nbed", (0, 1, 1023, 1024, 1025, 2047, 2048, 2049))
def test_bed_sizes_around_the_lds_chunk(ea, bams, nbed):
    bed = _bed(ea, nbed)
    for capture, param in EDGE:
        want = H.match_want(capture, param, nbed)[0]
        assert want.max() <= nbed and ((want > 0).any() or nbed <= 1)
        if nbed == 0:
            assert (want == NA).all()
        for layout in ("uploaded", "realigned"):
            assert np.array_equal(_match(bams[layout], bed, capture, param), want), (capture, layout)


@pytest.mark.parametrize("capture,param", EDGE)
def test_row_2049_alone_and_behind_row_1(ea, bams, capture, param):
    """A read whose only fitting row is the first of the third chunk gets 2049; with a fitting row 1 as well it gets 1."""
    t = H.match_templates()
    lens = np.diff(t["off"])
    x = int(np.flatnonzero((lens > 50) & (t["rname"] == 2))[7])
    rs, re_ = int(t["start"][x]), int(t["start"][x]) + int(lens[x]) - 1
    names, _, start, end = H.match_bed()
    names, start, end = list(names[:2048]), start[:2048].copy(), end[:2048].copy()
    one = {k: t[k][x:x + 1] for k in ("rname", "strand", "start")}
    one["off"] = np.asarray([0, lens[x]], np.int64)
    fits = H._bed_hits(one, (H.match_codes(names), start, end), capture, param, 0, 1)[0]
    for i in np.flatnonzero(fits):
        names[i] = "chrUn"                                              # no row of the first two chunks fits read x
    alone = ea.Bed(names + ["c2"], np.append(start, rs), np.append(end, re_))
    both = ea.Bed(["c2"] + names[1:] + ["c2"], np.append(np.append(rs, start[1:]), rs), np.append(np.append(re_, end[1:]), re_))
    for bed, answer in ((alone, 2049), (both, 1)):
        want = _want(t, bed, capture, param)
        assert len(bed) == 2049 and want[x] == answer
        assert np.array_equal(_match(bams["uploaded"], bed, capture, param), want), answer


@pytest.mark.parametrize("n", (1, 255, 256, 257, 512, 513))
def test_row_counts_around_the_block(ea, n):
    """The first n templates as a batch of their own: full blocks, one row more, one row less."""
    t = H.subset(H.match_templates(), np.arange(3001) < n)
    bed = _bed(ea)
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"], H.MATCH_LEVELS)
    for capture, param in EDGE:
        want = H.match_want(capture, param)[0][:n]
        assert np.array_equal(_want(t, bed, capture, param), want)
        got = _match(bam, bed, capture, param)
        assert got.shape == (n,) and np.array_equal(got, want), capture
    bam.close()


def test_positions_above_2_30(ea):
    """Every coordinate moved up by 2^30: the same rows match (start + len + |param| stays below 2^31 - 1)."""
    t = dict(H.match_templates())
    shift = 2 ** 30
    t["start"] = (t["start"].astype(np.int64) + shift).astype(np.int32)
    names, _, start, end = H.match_bed()
    bed = ea.Bed(names, start + shift, end + shift)
    assert int(t["start"].max()) + 300 + 1000 < 2 ** 31 - 1 and int(bed.end.max()) + 1000 < 2 ** 31 - 1
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"], H.MATCH_LEVELS)
    for capture, param in GRID:
        want = H.match_want(capture, param)[0]
        if (capture, param) in EDGE:
            assert np.array_equal(_want(t, bed, capture, param), want)
        assert np.array_equal(_match(bam, bed, capture, param), want), (capture, param)
    bam.close()


def test_rname_and_bed_codes_that_never_meet(ea, bams):
    """The C ABI with raw codes: BED rows on code 4 (a level no template is on) and on NA match nothing, a template on a
    code no BED row carries matches nothing, and the result is the restatement's for the codes as given."""
    import torch
    from epialleler_amd import api
    lib = ea._lib.load()
    t = dict(H.match_templates())
    t["rname"] = np.where(t["rname"] == 3, 7, t["rname"]).astype(np.int32)      # still sorted; no BED row has code 7
    _, code, start, end = H.match_bed()
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()
    d_chr, d_s, d_e = dev(code), dev(start), dev(end)
    for capture, param in EDGE:
        want = H.match_target_np(t, (code, start, end), capture, param)
        assert (want[t["rname"] == 7] == NA).all() and (want > 0).any()
        assert not np.isin(want[want > 0] - 1, np.flatnonzero((code == 4) | (code == NA))).any()
        out = torch.full((bam.n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
        rc = lib.epi_batch_match_target_dev(bam.batch(), C.c_void_p(d_chr.data_ptr()), C.c_void_p(d_s.data_ptr()),
                                            C.c_void_p(d_e.data_ptr()), len(code), int(capture), param,
                                            C.c_void_p(out.data_ptr()), api._stream(bam.device))
        assert rc == ea._lib.EPI_OK
        assert np.array_equal(out.cpu().numpy(), want), capture
    bam.close()


def test_c_abi_argument_checks_and_empty_bed(ea, bams):
    import torch
    from epialleler_amd import api
    lib = ea._lib.load()
    bam = bams["uploaded"]
    b, s = bam.batch(), api._stream(bam.device)
    z = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    zp = C.c_void_p(z.data_ptr())
    out = torch.full((bam.n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    op = C.c_void_p(out.data_ptr())
    for capture in (0, 1):
        assert lib.epi_batch_match_target_dev(b, zp, zp, zp, -1, capture, 1, op, s) == ea._lib.EPI_ERR_ARG
        for ptrs in ((None, zp, zp), (zp, None, zp), (zp, zp, None), (None, None, None)):
            assert lib.epi_batch_match_target_dev(b, ptrs[0], ptrs[1], ptrs[2], 4, capture, 1, op, s) == ea._lib.EPI_ERR_ARG
        assert lib.epi_batch_match_target_dev(b, zp, zp, zp, 4, capture, 1, None, s) == ea._lib.EPI_ERR_ARG
        assert lib.epi_batch_match_target_dev(None, zp, zp, zp, 4, capture, 1, op, s) == ea._lib.EPI_ERR_ARG
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x5A5A5A5A).all()                      # a refused call writes nothing
    for capture in (0, 1):
        out.fill_(0x5A5A5A5A)
        assert lib.epi_batch_match_target_dev(b, None, None, None, 0, capture, 1, op, s) == ea._lib.EPI_OK
        got = out.cpu().numpy()
        assert got.shape == (3001,) and (got == NA).all()              # every row written, none left as it was
    # the wrapper with an empty Bed, behind a dirty allocator: torch.empty's garbage must not show through
    H.dirty_allocator(bam)
    assert (_match(bam, ea.Bed([], [], []), True, 1) == NA).all()
    H.dirty_allocator(bam)
    assert (_match(bam, ea.Bed([], [], []), False, 1) == NA).all()
