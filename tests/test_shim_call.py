"""preprocessGenome / callMethylation's half of the shim core (epialleler_amd/r/epihip_shim_core.hpp: read_genome_into,
call_methylation), compiled with g++ and driven from C++ (tests/cpp/test_shim_call.cpp), as tests/test_shim_vcf.py does
for the VCF report."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAMS = os.path.join(ROOT, "tests", "golden", "bam")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from epialleler_amd import _lib
    _lib.build()
    out = str(tmp_path_factory.mktemp("shim_call") / "test_shim_call")
    csrc = os.path.join(ROOT, "epialleler_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "epialleler_amd", "r"), os.path.join(ROOT, "tests", "cpp", "test_shim_call.cpp"),
                           "-o", out, "-L", csrc, "-lepihip", "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib",
                           "-lamdhip64", "-lpthread"])
    return out


def test_shim_read_genome_host(exe):
    r = subprocess.run([exe, "cpu", BAMS], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "shim call cpu ok" in r.stdout


@pytest.mark.gpu
def test_shim_call_methylation(exe, tmp_path):
    r = subprocess.run([exe, "gpu", BAMS, str(tmp_path / "out.bam")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "shim call gpu ok" in r.stdout
