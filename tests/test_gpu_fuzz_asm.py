"""generateAsmReport on fixed-seed fuzz batches (tests/asm_np.py, fuzz_batch): random bases, ragged lengths, mate gaps, both
strands and a strand-0 row, all twelve REF / ALT pairs, max_distance in {0, 1, 50} and min_coverage in {1, 3}, against the
loop restatement.  The generator's conditions -- every batch reports a pair row; across the run every REF / ALT pair is
reported and every cell is zero in some row and non-zero in another; no batch is skipped -- were checked with the restatement
on the CPU and are asserted here."""
import numpy as np
import pytest

import asm_np as A
import test_gpu_asm as G

pytestmark = pytest.mark.gpu
SEEN = {"pairs": set(), "zero": set(), "nonzero": set(), "seeds": set(), "distance": set(), "coverage": set()}


@pytest.fixture(scope="module")
def ea():
    import epialleler_amd
    return epialleler_amd


@pytest.mark.parametrize("seed", A.FUZZ_SEEDS)
def test_fuzz(ea, seed):
    t, sites, ref_alt, args = A.fuzz_batch(seed)
    assert len(t["start"]) <= 2000
    pairs, snvs = G.check(ea, t, sites, label="seed %d" % seed, **args)
    assert len(pairs["snv"]) >= 1
    SEEN["seeds"].add(seed)
    SEEN["distance"].add(args["max_distance"])
    SEEN["coverage"].add(args["min_coverage"])
    SEEN["pairs"].update(ref_alt[s] for s in set(pairs["snv"].tolist()))
    for k in A.CELLS:
        if np.any(pairs[k] == 0):
            SEEN["zero"].add(k)
        if np.any(pairs[k] != 0):
            SEEN["nonzero"].add(k)


def test_fuzz_covered_the_cases():
    """(after the batches) about 40 of them, none skipped; every REF / ALT pair; both values of every cell being zero"""
    assert SEEN["seeds"] == set(A.FUZZ_SEEDS) and len(A.FUZZ_SEEDS) == 40
    assert SEEN["pairs"] == set(A.REF_ALT) and len(A.REF_ALT) == 12
    assert SEEN["zero"] == set(A.CELLS) and SEEN["nonzero"] == set(A.CELLS)
    assert SEEN["distance"] == {0, 1, 50} and SEEN["coverage"] == {1, 3}
