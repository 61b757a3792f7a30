"""simulateBam's table (R/simulateBam.R, .simulateBam in R/internal.R:296-403): what it returns without an output file,
which needs no device.  Record count, recycling and defaults, factor codes, the length of random bases, tag groups and
array subtypes."""
import numpy as np
import pytest

import epialleler_amd as ea
from epialleler_amd import simulate as sim


def col(rep, k):
    return list(np.asarray(rep[k]).tolist())


def test_exported():
    assert callable(ea.simulateBam) and callable(ea.rcpp_simulate_bam)


def test_nrecs_recycling_and_defaults():
    r = ea.simulateBam(pos=[1, 2, 3], mapq=[5, 6], seq="ACGTA", seed=1)
    assert r.nrow == 3
    assert col(r, "qname") == ["q0001", "q0002", "q0003"]
    assert col(r, "flag") == [0, 0, 0] and col(r, "tid") == [0, 0, 0] and col(r, "mtid") == [0, 0, 0]
    assert col(r, "pos") == [0, 1, 2] and col(r, "mpos") == [0, 0, 0]
    assert col(r, "mapq") == [5, 6, 5]
    assert col(r, "cigar") == ["5M"] * 3 and col(r, "isize") == [5] * 3 and col(r, "qual") == ["FFFFF"] * 3
    assert r.levels["rname"] == ("chrS",) and r.levels["rnext"] == ("chrS",)
    assert ea.simulateBam(seed=1).nrow == 1                       # nothing supplied: one record
    # the longest argument sets the count, tags included
    assert ea.simulateBam(pos=1, XG=["CT", "AG"], NM=list(range(5)), seed=1).nrow == 5
    assert ea.simulateBam(Ml=[[1, 2], [3], [4]], seed=1).nrow == 3   # an array tag: one element per array


def test_qname_past_9999():
    r = ea.simulateBam(pos=np.arange(1, 10002), seq="A", seed=3)
    q = col(r, "qname")
    assert q[0] == "q0001" and q[998] == "q0999" and q[9998] == "q9999" and q[9999] == "q10000" and q[10000] == "q10001"


def test_rname_and_rnext_have_their_own_factors():
    r = ea.simulateBam(rname=["b", "a", "b", "c"], rnext=["z", "b"], seq="AC", seed=1)
    assert r.levels["rname"] == ("a", "b", "c") and col(r, "tid") == [1, 0, 1, 2]
    assert r.levels["rnext"] == ("b", "z") and col(r, "mtid") == [1, 0, 1, 0]
    # code-point order: upper case before lower case
    assert ea.simulateBam(rname=["chr1", "Chr2", "chr10"], seq="A", seed=1).levels["rname"] == ("Chr2", "chr1", "chr10")


def test_random_seq_lengths_from_xm_then_tlen_then_ten():
    r = ea.simulateBam(XM=["Z" * 3, "z" * 7], tlen=[100, 200, 300], seed=5)
    assert [len(s) for s in col(r, "seq")] == [3, 7, 3]                # XM first
    assert col(r, "isize") == [100, 200, 300] and col(r, "cigar") == ["3M", "7M", "3M"]
    r = ea.simulateBam(tlen=[4, 6], seed=5)
    assert [len(s) for s in col(r, "seq")] == [4, 6]                  # then tlen
    r = ea.simulateBam(pos=[1, 2, 3, 4], seed=5)
    s = col(r, "seq")
    assert len(s[0]) == 10 and len(set(s)) == 1                       # one 10-mer recycled to every record
    for x in s:
        assert set(x) <= set("ACGT")


def test_random_seq_is_the_documented_function_of_the_seed():
    seed = 0x1234_5678_9ABC_DEF0
    r = ea.simulateBam(tlen=[20, 33], seed=seed)
    for j, s in enumerate(col(r, "seq")):
        want = "".join("ACTG"[int(sim.hash3(seed, 0x53494D, (j << 32) | k)) >> 62] for k in range(len(s)))
        assert s == want
    assert col(ea.simulateBam(tlen=[20, 33], seed=seed), "seq") == col(r, "seq")
    assert col(ea.simulateBam(tlen=[20, 33], seed=seed + 1), "seq") != col(r, "seq")


def test_xm_and_random_seq_from_different_indices():
    # seq is recycled from the XM lengths (len 2) per record, XM itself by its group (the s group's longest is 3)
    r = ea.simulateBam(pos=[1, 2, 3, 4], XM=["Z" * 2, "z" * 5], XG=["CT", "AG", "CT"], seed=1)
    assert col(r, "XM") == ["ZZ", "zzzzz", "ZZ", "ZZ"]
    assert [len(s) for s in col(r, "seq")] == [2, 5, 2, 5]


def test_tags_recycle_within_group_then_to_nrecs():
    r = ea.simulateBam(pos=list(range(1, 8)), XA=[1, 2, 3], XB=[10, 20], XF=[0.5, 1.5], XS=["a", "b", "c", "d"], seed=1)
    assert col(r, "XA") == [1, 2, 3, 1, 2, 3, 1]
    assert col(r, "XB") == [10, 20, 10, 10, 20, 10, 10]               # (i % 3) % 2, not i % 2
    assert col(r, "XF") == [0.5, 1.5, 0.5, 1.5, 0.5, 1.5, 0.5]        # alone in its group
    assert col(r, "XS") == ["a", "b", "c", "d", "a", "b", "c"]
    assert list(r.keys())[11:] == ["XA", "XB", "XF", "XS"]           # group order i, f, s, a


def test_tag_groups_by_python_type():
    r = ea.simulateBam(XS="s", XF=1.5, XI=7, XA=[[1, 2]], XN=np.array([1, 2], dtype=np.int16), XD=np.array([0.5]), seed=1)
    assert list(r.keys())[11:] == ["XI", "XN", "XF", "XD", "XS", "XA"]
    assert r.array_types == {"XA": "C"}


@pytest.mark.parametrize("vals,want", [
    ([-127, 127], "c"), ([-128, 0], "s"), ([-1, 128], "s"), ([0, 255], "C"), ([0, 256], "S"), ([-32767, 32767], "s"),
    ([-32768, 0], "i"), ([-1, 32768], "i"), ([0, 65535], "S"), ([0, 65536], "I"), ([1, 2.0], "f"), ([-5, 0.5], "f"),
    ([], "C"),
])
def test_array_subtype_table(vals, want):
    assert sim.array_subtype(vals) == want
    if vals:
        r = ea.simulateBam(XA=[vals[:1], vals[1:]], seed=1)
        assert r.array_types["XA"] == want


def test_array_subtype_uses_every_array():
    r = ea.simulateBam(zS=[list(range(240, 261))], zs=[list(range(-260, -239))], zI=[[1], [65540]], seed=1)
    assert r.array_types == {"zS": "S", "zs": "s", "zI": "I"}


def test_non_numeric_array_is_an_error():
    with pytest.raises(ValueError, match="BAM file format does not support non-numeric arrays"):
        ea.simulateBam(pos=1, AB=list(range(1, 11)), Ze=[list("ABCDEFGHI")])


def test_reference_second_call_returns_the_table():
    r = ea.simulateBam(qname="a", flag=2, rname="chrQ", pos=[1, 3], mapq=45, cigar="5M", rnext="chrQ", pnext=[3, 1],
                       tlen=8, seq=["CCCC", "TTTTTTTT"], qual=["FFFF", "DDDDDDDD"], verbose=False,
                       XM=["zzZZ", "ZZzzZZzz"])
    assert list(r.keys()) == ["qname", "flag", "tid", "pos", "mapq", "cigar", "mtid", "mpos", "isize", "seq", "qual", "XM"]
    assert r.nrow == 2
    assert col(r, "qname") == ["a", "a"] and col(r, "flag") == [2, 2] and col(r, "tid") == [0, 0]
    assert col(r, "pos") == [0, 2] and col(r, "mapq") == [45, 45] and col(r, "cigar") == ["5M", "5M"]
    assert col(r, "mtid") == [0, 0] and col(r, "mpos") == [2, 0] and col(r, "isize") == [8, 8]
    assert col(r, "seq") == ["CCCC", "TTTTTTTT"] and col(r, "qual") == ["FFFF", "DDDDDDDD"]
    assert col(r, "XM") == ["zzZZ", "ZZzzZZzz"]
    assert r.levels["rname"] == ("chrQ",)


def test_header_lines():
    p = sim._prepare(None, None, ["b", "a"], [1, 7], None, None, None, [3, 12], [5, 9], None, None, {}, 1,
                     [["b", "a"], [1, 7], [3, 12], [5, 9]])
    assert p["header"] == ["@SQ\tSN:a\tLN:20", "@SQ\tSN:b\tLN:20",
                           "@PG\tID:epialleleR\tPN:epialleleR\tVN:%s\tCL:rcpp_simulate_bam()" % sim.VERSION]


@pytest.mark.parametrize("kw", [dict(flag=65536), dict(mapq=256), dict(flag=-1), dict(pos=2 ** 31 + 1), dict(NM=2 ** 31),
                                dict(XA=[[2 ** 31]]), dict(XM=[1, "a"])])
def test_out_of_range_values(kw):
    with pytest.raises(ValueError):
        ea.simulateBam(**kw)


def test_writing_without_device_fails_loudly(tmp_path):
    # with no usable device the library refuses (EpihipError), there is no CPU path; on a GPU machine it writes
    import ctypes as C
    from epialleler_amd import _lib
    lib = _lib.load()
    eng = C.c_void_p()
    if lib.epi_default_engine(C.byref(eng)) == _lib.EPI_OK:
        assert ea.simulateBam(str(tmp_path / "x.bam"), seed=1) == 1
    else:
        with pytest.raises(ea.EpihipError):
            ea.simulateBam(str(tmp_path / "x.bam"), seed=1)
        assert not (tmp_path / "x.bam").exists()
