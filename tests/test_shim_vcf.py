"""generateVcfReport's half of the shim core (epialleler_amd/r/epihip_shim_core.hpp: base_freqs_into, fep_into), compiled
with g++ and driven from C++ (tests/cpp/test_shim_vcf.cpp), as tests/test_shim_core.py does for the report shims."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from epialleler_amd import _lib
    _lib.build()
    out = str(tmp_path_factory.mktemp("shim_vcf") / "test_shim_vcf")
    csrc = os.path.join(ROOT, "epialleler_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "epialleler_amd", "r"), os.path.join(ROOT, "tests", "cpp", "test_shim_vcf.cpp"),
                           "-o", out, "-L", csrc, "-lepihip", "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib",
                           "-lamdhip64", "-lpthread"])
    return out


def test_shim_fep_host(exe):
    r = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "shim vcf cpu ok" in r.stdout


@pytest.mark.gpu
def test_shim_base_freqs(exe):
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "shim vcf gpu ok" in r.stdout
