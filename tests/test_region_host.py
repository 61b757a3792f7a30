"""generateRegionReport on the host side: the exported symbols, the functions' signatures, argument checks before any I/O,
the counters' size as a function of its own, the loud failure without a device (there is no CPU path), and the restatement
of the definitions (tests/region_np.py) against closed forms that do not come from it."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import helpers as H
import region_np as RN
import epialleler_amd as ea
from epialleler_amd import _lib

NEW_SYMBOLS = ("epi_batch_region_report_dev", "epi_region_counter_bytes")
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
    assert ea.REGION_COLUMNS == ("rname", "start", "end", "nreads", "nlong", "kreads", "tbase", "mbase", "cbase", "ndiscordant",
                                 "nmethylated", "n_u", "n_x", "n_m", "maxsites", "beta", "pdr", "chalm", "mcr", "mbs", "mhl")
    assert ea.REGION_COLUMNS == RN.COLUMNS


def test_signatures_and_defaults():
    p = inspect.signature(ea.generateRegionReport).parameters
    assert [(k, v.default) for k, v in p.items() if v.kind is not v.VAR_KEYWORD] == [
        ("bam", EMPTY), ("bed", EMPTY), ("report_file", None), ("zero_based_bed", False), ("region_context", None), ("min_sites", 4),
        ("max_sites", 64), ("strand_offset", None), ("uxm_thresholds", (0.25, 0.75)), ("max_outofcontext_beta", 0.1), ("gzip", False),
        ("verbose", False), ("as_device", False)]
    assert [k for k, v in p.items() if v.kind is v.VAR_KEYWORD] == ["preprocess_args"]
    q = inspect.signature(ea.rcpp_region_report).parameters
    assert [(k, v.default) for k, v in q.items()] == [
        ("df", EMPTY), ("regions", EMPTY), ("ctx", EMPTY), ("min_sites", EMPTY), ("max_sites", EMPTY), ("reverse_offset", EMPTY),
        ("u_max", EMPTY), ("m_min", EMPTY), ("max_ooctx_meth_frac", EMPTY), ("as_device", False)]


BAD = [dict(min_sites=0), dict(min_sites=65), dict(min_sites=2.5), dict(min_sites=True), dict(max_sites=0), dict(max_sites=257),
       dict(max_sites=3), dict(max_sites=1.5), dict(strand_offset=-1), dict(strand_offset=0.5),
       dict(uxm_thresholds=(0.5, 0.5)), dict(uxm_thresholds=(0.75, 0.25)), dict(uxm_thresholds=(-0.1, 0.5)), dict(uxm_thresholds=(0.2, 1.1)),
       dict(uxm_thresholds=(0.2,)), dict(uxm_thresholds=(0.1, 0.2, 0.3)), dict(uxm_thresholds=(float("nan"), 0.5)), dict(uxm_thresholds=None),
       dict(region_context="CpG"), dict(region_context="cg")]
R_NAME = {"min_sites": "min.sites", "max_sites": "max.sites", "strand_offset": "strand.offset", "uxm_thresholds": "uxm.thresholds"}


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: ",".join("%s=%s" % it for it in kw.items()))
def test_bad_arguments_raise_before_io(kw):
    with pytest.raises(ValueError) as ei:
        ea.generateRegionReport("no-such-file.bam", "no-such-file.bed", **kw)    # (opening either would raise another error)
    msg = str(ei.value)
    name = list(kw)[-1]
    if kw == dict(max_sites=3):                              # (the default min_sites = 4 is what no longer fits)
        assert "'min.sites' should be an integer from 1 to 3" in msg
    elif name == "region_context":
        assert "'region.context' should be one of 'CG', 'CHG', 'CHH', 'CxG', 'CX'" in msg
    else:
        assert "'%s' should be" % R_NAME[name] in msg
    assert "no-such-file" not in msg and "open" not in msg


def test_good_edge_values_reach_the_file():
    for kw in (dict(min_sites=1), dict(min_sites=64), dict(min_sites=1, max_sites=1), dict(min_sites=256, max_sites=256), dict(strand_offset=0),
               dict(strand_offset=7), dict(uxm_thresholds=(0, 1)), dict(uxm_thresholds=(0.0, 1e-9)), dict(region_context="CX"),
               dict(min_sites=np.int64(3), max_sites=5.0)):
        with pytest.raises(Exception) as ei:
            ea.generateRegionReport("no-such-file.bam", "chr1:10-20", **kw)
        assert not isinstance(ei.value, ValueError) or "should be" not in str(ei.value), kw
    with pytest.raises(Exception) as ei:                     # the BED is read before the BAM
        ea.generateRegionReport("no-such-file.bam", "no-such-file.bed")
    assert "should be" not in str(ei.value)


def test_counter_bytes():
    """(3 max_sites + 16) 64-bit counters per region; 0 .. 2^31 - 1 regions of 1 .. 256 sites"""
    lib = _lib.load()
    out = C.c_int64(-1)
    for nreg, ms in ((0, 64), (1, 1), (1, 64), (1, 256), (565, 64), (2 ** 31 - 1, 256)):
        assert lib.epi_region_counter_bytes(nreg, ms, C.byref(out)) == _lib.EPI_OK and out.value == nreg * (3 * ms + 16) * 8, (nreg, ms)
    for nreg, ms in ((-1, 64), (2 ** 31, 64), (2 ** 40, 1), (1, 0), (1, 257), (1, -4)):
        assert lib.epi_region_counter_bytes(nreg, ms, C.byref(out)) == _lib.EPI_ERR_ARG and out.value == 0, (nreg, ms)
    assert b"regions" in lib.epi_last_error()
    assert lib.epi_region_counter_bytes(1, 64, None) == _lib.EPI_ERR_ARG


def test_fails_loudly_without_gpu():
    if _has_gpu():
        pytest.skip("GPU present")
    t = H.templates_from_xm(["Z.z.Z.z", "z.Z.z.Z"], [1, 1], [1, 1])
    bam = ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"], levels=["chr1"])
    for call in (lambda: ea.generateRegionReport(bam, "chr1:1-7"), lambda: ea.rcpp_region_report(bam, ([1], [1], [7]), "Zz", 4, 64, 1, 0.25, 0.75, 0.1)):
        with pytest.raises(ea.EpihipError) as ei:
            call()
        assert ei.value.code == 5 and "no CPU fallback" in str(ei.value)


# ---- the restatement against closed forms -----------------------------------------------------------------------------------

def one_region(xms, end, **kw):
    t = H.templates_from_xm(xms, [1] * len(xms), [1] * len(xms))
    return RN.restate(t, ([1], [1], [end]), "Zz", with_acc=True, **kw)


def test_every_call_methylated():
    r = one_region(["Z.Z.Z.Z", "ZZZZZ", "Z..Z.Z.Z..Z.Z"], 20)
    assert r["kreads"][0] == 3 and r["maxsites"][0] == 6
    assert r["mhl"][0] == 1.0 and r["mbs"][0] == 1.0 and r["chalm"][0] == 1.0 and r["pdr"][0] == 0.0 and r["mcr"][0] == 0.0 and r["beta"][0] == 1.0
    assert (r["n_u"][0], r["n_x"][0], r["n_m"][0]) == (0, 0, 3)


def test_no_call_methylated():
    r = one_region(["z.z.z.z", "zzzzz", "z..z.z.z..z.z"], 20)
    assert r["kreads"][0] == 3
    for k in ("mhl", "mbs", "chalm", "pdr", "mcr", "beta"):
        assert r[k][0] == 0.0, k
    assert (r["n_u"][0], r["n_x"][0], r["n_m"][0]) == (3, 0, 0)


def test_half_and_half():
    r = one_region(["ZZZZ", "zzzz"] * 5, 4)
    assert r["mhl"][0] == 0.5 and r["pdr"][0] == 0.0 and r["mbs"][0] == 0.5 and r["chalm"][0] == 0.5 and r["beta"][0] == 0.5


def test_one_read_mmum():
    r = one_region(["ZZzZ"], 4)
    acc = r["acc"][0]
    assert acc["M"][1:5] == [3, 1, 0, 0] and acc["T"][1:5] == [4, 3, 2, 1]
    assert r["mhl"][0] == (np.float64(3) / 4 + 2 * (np.float64(1) / 3)) / 10
    assert r["mbs"][0] == 5 / 16 and r["mcr"][0] == 1 / 4
    assert (r["nreads"][0], r["kreads"][0], r["tbase"][0], r["mbase"][0], r["cbase"][0], r["ndiscordant"][0], r["nmethylated"][0]) == (1, 1, 4, 3, 1, 1, 1)
    assert (r["n_u"][0], r["n_x"][0], r["n_m"][0]) == (0, 0, 1)                     # 3 of 4 at 0.75: on the threshold is M


def test_restatement_rules():
    """Clipping, the reverse strand's offset, the read rule, long rows and the thresholds, by hand"""
    t = H.templates_from_xm(["Z.Z.z.Z", "Z.Z.z.Z", "ZzZzH", "zZzz", "ZZZZZ"], [10, 11, 10, 12, 10], [1, 2, 1, 1, 1])
    r = RN.restate(t, ([1, 1, 2, 1], [10, 12, 10, 30], [16, 14, 16, 40]), "Zz", min_sites=2, max_sites=4, reverse_offset=1, with_acc=True)
    # region 1 = 10-16: row "Z.Z.z.Z"+ has 4 calls, the '-' row at 11 is at 10 .. 16 after its offset: 4 calls; "ZzZzH" is dropped
    # (1 of 1 out-of-context calls is methylated), "zZzz" at 12 has 4 calls, "ZZZZZ" has 5 > max_sites
    assert (r["nreads"][0], r["nlong"][0], r["kreads"][0], r["maxsites"][0]) == (4, 1, 3, 4)
    assert (r["tbase"][0], r["mbase"][0], r["cbase"][0]) == (12, 7, 5)
    # region 2 = 12-14: "Z.Z.z.Z"+ has z at 14 and Z at 12; the '-' row: bytes at 10, 12, 14, 16 -> Z at 12, z at 14; "zZzz": z, Z, z; "ZZZZZ": 3
    assert (r["nreads"][1], r["kreads"][1], r["tbase"][1], r["mbase"][1]) == (4, 4, 10, 6)
    assert (r["n_u"][1], r["n_x"][1], r["n_m"][1]) == (0, 3, 1)
    assert r["nreads"][2] == 0 and np.isnan(r["beta"][2]) and np.isnan(r["mhl"][2]) and r["nreads"][3] == 0
    assert r["rname"].tolist() == [1, 1, 2, 1] and r["rname"].dtype == np.int32 and r["mhl"].dtype == np.float64
