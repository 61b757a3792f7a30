"""The device scan of csrc/scan.hpp at the seam that no other test reaches: the row offsets of csrc/layout.hip (a 64-bit
sum with a seed, 4 rows per thread, 1024 per workgroup) on a batch of more than 256 x 1024 rows, so that the one workgroup
that scans the workgroups' aggregates goes round twice.  (The 32-bit sum and the min / max of doubles go round twice in
test_gpu_cx_compare_seams.py and test_gpu_p_adjust.py.)"""
import numpy as np
import pytest

from test_gpu_layout import _check_layout, _view

pytestmark = pytest.mark.gpu


def _short_rows(n, seed):
    """n rows of 1 to 3 bytes; starts that step by 0 to 20 with runs of repeats, and one rname change"""
    rng = np.random.default_rng(seed)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(rng.integers(1, 4, size=n), out=off[1:])
    step = rng.integers(0, 21, size=n)
    step[rng.random(n) < 0.25] = 0
    second = n // 2 if n > 1 else n                                  # rows [second, n) are on the next rname
    start = np.concatenate([1003 + np.cumsum(step[:second]), 7 + np.cumsum(step[second:])]).astype(np.int32)
    rname = np.where(np.arange(n) < second, 1, 2).astype(np.int32)
    return {"xm": rng.integers(0, 256, size=int(off[-1])).astype(np.uint8), "off": off, "rname": rname,
            "strand": rng.integers(1, 3, size=n).astype(np.int32), "start": start}


def _want_offsets(t, modulus):
    """layout.hip's ly_item restated: a row adds its bytes and the filler that makes the next row start congruent to its
    start position; the sum is seeded with the filler in front of row 0"""
    ln = np.diff(t["off"])
    start = t["start"].astype(np.int64)
    item = ln.copy()
    item[:-1] += (start[1:] - (start[:-1] + ln[:-1])) % modulus
    want = np.empty(ln.size + 1, np.int64)
    want[0] = start[0] % modulus
    want[1:] = want[0] + np.cumsum(item)
    return want


@pytest.mark.parametrize("n", [1, 1025, 256 * 1024 + 1025])
def test_layout_offsets_against_cumsum(n):
    import torch
    import epialleler_amd as ea
    t = _short_rows(n, 5)
    nb = int(t["off"][-1])
    assert nb < 1 << 20
    xm = torch.full(((nb + 15) // 16 * 16 + 64,), 0xFB, dtype=torch.uint8, device="cuda:0")
    xm[:nb] = torch.from_numpy(t["xm"]).cuda()
    bam = ea.ProcessedBam.from_device(xm, nb, torch.from_numpy(t["off"]).cuda(), torch.from_numpy(t["rname"]).cuda(),
                                      torch.from_numpy(t["strand"]).cuda(), torch.from_numpy(t["start"]).cuda(), realign=True)
    try:
        got_xm, off, ln, layout = _view(ea, bam)                     # (creates the batch: epi_batch_adopt, epi_batch_realign)
        assert layout == 16
        want = _want_offsets(t, 16)
        assert np.array_equal(off, want)                             # every offset, and off[n] = the end of the data
        assert got_xm.size == want[-1]
        _check_layout(t, got_xm, off, ln, 16)
    finally:
        bam.close()
