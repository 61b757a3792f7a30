"""The BED path without a device: readBed (R/internal.R:205-222) on small files, and the restatements that the GPU
tests of k_match_target, generateBedReport and generateBedEcdf compare with (helpers.match_target_np, bed_report_np,
ecdf_np, beta_np) -- the vectorised matcher against the two nested loops, and the synthetic case against the conditions
that make it worth running."""
import numpy as np
import pytest

import helpers as H
from epialleler_amd import bed as B


def _write(tmp_path, text, name="t.bed"):
    p = tmp_path / name
    p.write_bytes(text.encode())
    return str(p)


def test_bed_module_imports_without_a_device():
    assert callable(B.readBed) and B.NA_INTEGER == H.NA_INT


def test_read_bed_without_header(tmp_path):
    bd = B.readBed(_write(tmp_path, "chr1\t10\t20\nchr2\t5\t7\n"))
    assert len(bd) == 2 and bd.chrom == ["chr1", "chr2"] and bd.extra == {}
    assert bd.start.dtype == np.int64 and bd.end.dtype == np.int64
    assert bd.start.tolist() == [10, 5] and bd.end.tolist() == [20, 7]
    assert bd.names() == ["chr1:10-20", "chr2:5-7"]


def test_read_bed_extra_columns_are_v4_v5_without_header(tmp_path):
    bd = B.readBed(_write(tmp_path, "chr1\t10\t20\tA\t0.5\nchr2\t5\t7\tB\t1\n"))
    assert list(bd.extra.keys()) == ["V4", "V5"]
    assert bd.extra["V4"] == ["A", "B"] and bd.extra["V5"] == ["0.5", "1"]
    assert bd.start.tolist() == [10, 5] and bd.names() == ["chr1:10-20", "chr2:5-7"]


def test_read_bed_header_names_the_extra_columns(tmp_path):
    # (whatever the header calls the first three columns, they are chr / start / end: R/internal.R:215)
    bd = B.readBed(_write(tmp_path, "#chrom\tchromStart\tchromEnd\tamplicon\tscore\nchr1\t10\t20\tA\t3\nchr2\t5\t7\tB\t4\n"))
    assert len(bd) == 2 and bd.chrom == ["chr1", "chr2"]
    assert list(bd.extra.keys()) == ["amplicon", "score"]
    assert bd.extra["amplicon"] == ["A", "B"] and bd.extra["score"] == ["3", "4"]
    assert bd.start.tolist() == [10, 5] and bd.end.tolist() == [20, 7]
    plain = B.readBed(_write(tmp_path, "chr\tstart\tend\nchr1\t10\t20\n", "h3.bed"))
    assert len(plain) == 1 and plain.extra == {} and plain.names() == ["chr1:10-20"]


def test_read_bed_skips_blank_lines(tmp_path):
    bd = B.readBed(_write(tmp_path, "\nchr1\t10\t20\tA\n\n   \nchr2\t5\t7\tB\n\n\n"))
    assert bd.chrom == ["chr1", "chr2"] and bd.extra == {"V4": ["A", "B"]}
    assert bd.start.tolist() == [10, 5] and bd.end.tolist() == [20, 7]
    hdr = B.readBed(_write(tmp_path, "\n\nchr\tstart\tend\tname\n\nchr1\t10\t20\tA\n\n", "h.bed"))
    assert hdr.chrom == ["chr1"] and hdr.extra == {"name": ["A"]}


def test_read_bed_crlf(tmp_path):
    bd = B.readBed(_write(tmp_path, "chr\tstart\tend\tname\r\nchr1\t10\t20\tA\r\n\r\nchr2\t5\t7\tB\r\n"))
    assert bd.chrom == ["chr1", "chr2"] and bd.end.tolist() == [20, 7]
    assert bd.extra == {"name": ["A", "B"]}                            # no '\r' left on the last field
    assert bd.names() == ["chr1:10-20", "chr2:5-7"]


def test_read_bed_zero_based_shifts_starts_only(tmp_path):
    path = _write(tmp_path, "chr1\t0\t20\tA\nchr2\t5\t7\tB\n")
    one, zero = B.readBed(path), B.readBed(path, zero_based_bed=True)
    assert one.start.tolist() == [0, 5] and zero.start.tolist() == [1, 6]
    assert one.end.tolist() == zero.end.tolist() == [20, 7]
    assert zero.chrom == one.chrom and zero.extra == one.extra
    assert zero.names() == ["chr1:1-20", "chr2:6-7"]


def test_read_bed_ragged_extra_columns(tmp_path):
    bd = B.readBed(_write(tmp_path, "chr1\t10\t20\nchr2\t5\t7\tB\t9\nchr3\t1\t2\tC\n"))
    assert list(bd.extra.keys()) == ["V4", "V5"]
    assert bd.extra["V4"] == ["", "B", "C"] and bd.extra["V5"] == ["", "9", ""]
    assert bd.chrom == ["chr1", "chr2", "chr3"] and bd.start.tolist() == [10, 5, 1]


def test_read_bed_negative_coordinate(tmp_path):
    # (a first line with a negative start is data, not a header)
    bd = B.readBed(_write(tmp_path, "chr1\t-5\t20\nchr2\t3\t-1\n"))
    assert bd.chrom == ["chr1", "chr2"] and bd.start.tolist() == [-5, 3] and bd.end.tolist() == [20, -1]
    assert bd.names() == ["chr1:-5-20", "chr2:3--1"]
    assert B.readBed(_write(tmp_path, "chr1\t-5\t20\n", "z.bed"), zero_based_bed=True).start.tolist() == [-4]


def test_read_bed_empty_and_header_only(tmp_path):
    for text in ("", "\n\n", "chr\tstart\tend\n"):
        bd = B.readBed(_write(tmp_path, text))
        assert len(bd) == 0 and bd.start.size == 0 and bd.end.size == 0 and bd.extra == {} and bd.names() == []


# ---- the restatements ---------------------------------------------------------------------------------------------------

def _case_bed():
    names, _, start, end = H.match_bed()
    return H.match_codes(names), start, end


@pytest.mark.parametrize("capture,param", [(False, -1), (False, 0), (False, 2), (False, 1000), (True, -50), (True, 0), (True, 1),
                                           (True, 150)])
def test_vectorised_matcher_equals_the_loops(capture, param):
    t = H.match_templates()
    rows = np.arange(0, len(t["start"]), 10)                           # ~300 reads over all three rnames
    want = H.match_target_loop(t, _case_bed(), capture, param, rows)
    got = H.match_want(capture, param)[0] if param in H.MATCH_INTERIOR[capture] else H.match_target_np(t, _case_bed(), capture, param)
    assert got.dtype == np.int32 and np.array_equal(got[rows], want)


def test_matcher_restatement_small_known_answers():
    t = H.templates_from_xm(["z" * 10, "", "z" * 5, "z" * 10], [100, 200, 300, 100], [1, 2, 1, 2], rnames=[1, 1, 1, 2])
    # rows sorted by (rname, start): [1:100-109], [1:200-199] (empty), [1:300-304], [2:100-109]
    bed = (np.asarray([1, 1, 2, H.NA_INT, 1]), np.asarray([98, 100, 105, 100, 190]), np.asarray([250, 109, 120, 109, 304]))
    assert H.match_target_np(t, bed, False, 0).tolist() == [2, H.NA_INT, 5, H.NA_INT]          # exact start or exact end
    assert H.match_target_np(t, bed, False, 2).tolist() == [1, H.NA_INT, 5, H.NA_INT]          # row 1 fits first now
    assert H.match_target_np(t, bed, False, -1).tolist() == [H.NA_INT] * 4
    assert H.match_target_np(t, bed, True, 1).tolist() == [1, H.NA_INT, 5, 3]                  # an empty read overlaps by 0
    assert H.match_target_np(t, bed, True, 0).tolist() == [1, 1, 5, 3]
    assert H.match_target_np(t, bed, True, 6).tolist() == [1, H.NA_INT, H.NA_INT, H.NA_INT]    # 2:100-109 on 105-120: 5
    assert H.match_target_np(t, bed, True, -49).tolist() == [1, 1, 1, 3]                       # 300-304 is 49 past 250
    assert H.match_target_np(t, (bed[0][:0], bed[1][:0], bed[2][:0]), True, 1).tolist() == [H.NA_INT] * 4
    for capture, param in ((False, 0), (False, 2), (True, 1), (True, 0), (True, -49)):
        assert np.array_equal(H.match_target_np(t, bed, capture, param), H.match_target_loop(t, bed, capture, param))


def test_synthetic_case_meets_its_design():
    t = H.match_templates()
    lens = np.diff(t["off"])
    assert len(t["start"]) == 3001 and (lens == 0).any() and set(np.unique(t["rname"])) == {1, 2, 3}
    assert 10 <= np.count_nonzero(t["strand"] == 0) <= 60
    names, code, start, end = H.match_bed()
    assert len(names) == 2500 and (start > end).any() and (code == 4).any() and (code == H.NA_INT).any()
    assert np.array_equal(H.match_codes(names), np.where(code == 4, H.NA_INT, code))
    assert np.any(np.diff(np.asarray(code, np.int64) * 2 ** 32 + start) < 0)                    # unsorted
    H.assert_match_design()
    for capture, param in ((False, -1), (True, 400)):
        assert not (H.match_target_np(t, _case_bed(), capture, param) > 0).any()
    assert (H.match_target_np(t, _case_bed(), False, 1000) > 0).mean() > 0.5


def test_report_restatement_known_answers():
    t = {"strand": np.asarray([1, 2, 0, 1, 2, 1, 0], np.int32)}
    match = np.asarray([1, 1, 2, H.NA_INT, 3, 3, H.NA_INT])
    r = H.bed_report_np(t, [1, 0, 1, 1, 1, 1, 0], match, 4)
    assert r["has_na"] is True
    np.testing.assert_array_equal(r["nreads+"], [1, np.nan, 1, np.nan, 1])                     # row 2: only a strand-0 read
    np.testing.assert_array_equal(r["nreads-"], [1, np.nan, 1, np.nan, 0])
    np.testing.assert_array_equal(r["VEF"], [0.5, np.nan, 1.0, np.nan, 1.0])
    r = H.bed_report_np(t, np.zeros(7), np.where(match < 0, 4, match), 4)
    assert r["has_na"] is False and np.isnan(r["VEF"][4]) and r["nreads+"][3] == 1 and r["VEF"][0] == 0


def test_ecdf_and_beta_restatements_known_answers():
    x = [0.5, 0.25, 0.5, 1.0]
    assert H.ecdf_np(x, [0.0, 0.25, np.nextafter(0.5, 0), 0.5, 0.75, 1.0, 2.0]).tolist() == [0, 0.25, 0.25, 0.75, 0.75, 1, 1]
    e = B.Ecdf(x)
    assert e.x.tolist() == [0.25, 0.5, 0.5, 1.0] and e(0.5) == 0.75 and isinstance(e(0.5), float)
    assert np.array_equal(e(np.asarray([0.0, 0.5, 2.0])), [0.0, 0.75, 1.0])
    t = H.templates_from_xm(["ZZz.x", "", "xh", "Z"], [1, 2, 3, 4], [1, 1, 1, 1])
    assert H.beta_np(t["xm"], t["off"], "Z", "z").tolist() == [2 / 3, 0.0, 0.0, 1.0]
    assert H.beta_np(t["xm"], t["off"], "XH", "xh").tolist() == [0.0, 0.0, 0.0, 0.0]
