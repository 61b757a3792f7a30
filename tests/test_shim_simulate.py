"""simulateBam's half of the shim core (epialleler_amd/r/epihip_shim_core.hpp: sim_columns, simulate_bam), compiled
with g++ and driven from C++ (tests/cpp/test_shim_simulate.cpp), as tests/test_shim_call.py does for callMethylation.
The GPU case checks that the shim's mapping of R's recycled columns writes the same bytes as the Python path."""
import gzip
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from epialleler_amd import _lib
    _lib.build()
    out = str(tmp_path_factory.mktemp("shim_simulate") / "test_shim_simulate")
    csrc = os.path.join(ROOT, "epialleler_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "epialleler_amd", "r"),
                           os.path.join(ROOT, "tests", "cpp", "test_shim_simulate.cpp"), "-o", out, "-L", csrc, "-lepihip",
                           "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-lpthread"])
    return out


def test_shim_simulate_columns(exe):
    r = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "shim simulate cpu ok" in r.stdout


@pytest.mark.gpu
def test_shim_simulate_matches_python(exe, tmp_path):
    import epialleler_amd as ea
    shim_out = str(tmp_path / "shim.bam")
    r = subprocess.run([exe, "gpu", shim_out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "shim simulate gpu ok" in r.stdout
    assert not os.path.exists(shim_out + ".bad")
    py_out = str(tmp_path / "py.bam")
    n = ea.simulateBam(py_out, qname=["a", "bb", "ccc"], flag=[0, 16, 4], rname=["chr1", "chr2", "chr1"], pos=[1, 5, 9],
                       mapq=[60, 30, 0], cigar=["4M", "2M1I1M", "*"], rnext=["chr1", "chr2", "chr1"], pnext=1,
                       tlen=[4, -4, 0], seq=["ACGT", "acgn", "TTTT"], qual=["FFFF", "!!!!", "IIII"],
                       NM=[1, -200, 70000], XF=[0.5, -1.25, 0.1], XM=["zZ..", "....", ""],
                       ML=[[1, 2], [255], []], MF=[[1.5], [], [-2.0, 0.25]], seed=0)
    assert n == 3
    with open(shim_out, "rb") as a, open(py_out, "rb") as b:
        assert gzip.decompress(a.read()) == gzip.decompress(b.read())
