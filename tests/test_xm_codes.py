"""The shared XM code header (csrc/xm_codes.hpp) on the CPU: tests/cpp/xm_codes_main.cpp, a program of its own built with
AddressSanitizer and UBSan and run as a child process -- the two table lookups over a host model of v_perm_b32, the code
of every XM letter, the class masks and the read rule's verdict on its seams.  Nothing sanitized is loaded into python;
that the hardware follows the model is what the GPU parity tests pin."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_xm_codes(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *SAN, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ has no sanitizer runtime")
    exe = str(tmp_path / "xm_codes_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", *SAN, "-Wall", "-D__HIP_PLATFORM_AMD__",
                    "-I/opt/rocm/include", "-I", os.path.join(ROOT, "epialleler_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "xm_codes_main.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    assert "xm_codes ok" in r.stdout
