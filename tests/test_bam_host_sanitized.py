"""The BAM reader, packers and call set under AddressSanitizer and UBSan, on the CPU: tests/cpp/bam_host_main.cpp, a
program of its own linked statically against the host-only build of the library's host sources (csrc/Makefile, `make
bam-host-test`), run as a child process over every golden BAM with three option sets and over 200 seeded crafted files
(tests/bam_craft.py; file k takes option set k % 3, so each set meets malformed records).  Every run must end with
status 0 and an empty stderr; where libepihip.so is built, its outcome -- the table or the error text -- must also be,
byte for byte, what the library returns for the same file and options.  Nothing sanitized is loaded into python."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import helpers as H
from bam_craft import crafted_files
from epialleler_amd import _lib

BAM = os.path.join(H.GOLDEN, "bam")
GOLDENS = sorted(f for f in os.listdir(BAM) if f.endswith(".bam"))
OPTION_SETS = (
    {},
    dict(trim5=2, trim3=5, min_baseq=20, min_mapq=30, nthreads=3, window_kib=1),
    dict(skip_duplicates=1, nthreads=16, window_kib=7),
)
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.fixture(scope="session")
def host_main(tmp_path_factory):
    if not shutil.which("g++") or not shutil.which("make"):
        pytest.skip("no g++ / make")
    d = tmp_path_factory.mktemp("bam_host")
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *SAN, str(probe), "-o", str(d / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ has no sanitizer runtime")
    subprocess.run(["make", "-C", _lib.CSRC, "-j8", "bam-host-test", "OUT=%s" % d], check=True, capture_output=True)
    return str(d / "bam_host_main")


def library_outcome(lib, path, kw):
    """What bam_host_main prints, made from the library's own answer."""
    o = dict(min_mapq=0, min_baseq=0, skip_duplicates=0, skip_secondary=1, skip_qcfail=1, skip_supplementary=1, trim5=0,
             trim3=0, paired=-1, nthreads=1, min_prob=-1, highest_prob=1, window_kib=0)
    o.update(kw)
    opt = _lib.BamOptions(**o)
    t = _lib.Templates()
    rc = lib.epi_preprocess_bam(path.encode(), C.byref(opt), C.byref(t))
    if rc != _lib.EPI_OK:
        return b"error %d %s\n" % (rc, lib.epi_last_error())
    n = t.n
    names = b",".join(t.target_names[i] for i in range(t.n_targets))
    out = b"ok n=%d nbytes=%d nrecs=%d npushed=%d paired=%d targets=%s\n" % (n, t.nbytes, t.nrecs, n, t.paired, names)
    for ptr, k in ((t.xm, t.nbytes), (t.off, n + 1), (t.rname, n), (t.strand, n), (t.start, n)):
        out += C.string_at(ptr, k * C.sizeof(ptr._type_)) if k else b""
    lib.epi_templates_free(C.byref(t))
    return out


def run_all(host_main, cases):
    lib = _lib.load() if os.path.exists(_lib.LIB_PATH) else None
    tables = errors = 0
    for path, kw in cases:
        what = "%s %r" % (os.path.basename(path), kw)
        r = subprocess.run([host_main, path] + ["%s=%d" % kv for kv in sorted(kw.items())], capture_output=True)
        assert r.returncode == 0 and r.stderr == b"", "%s: status %d\n%s" % (what, r.returncode, r.stderr.decode("utf-8", "replace"))
        assert r.stdout.startswith((b"ok ", b"error ")), what
        tables += r.stdout.startswith(b"ok ")
        errors += r.stdout.startswith(b"error ")
        if lib is not None:
            assert r.stdout == library_outcome(lib, path, kw), what
    print("%d runs: %d tables, %d errors" % (len(cases), tables, errors))
    return tables, errors


def test_goldens(host_main):
    tables, errors = run_all(host_main, [(os.path.join(BAM, name), kw) for name in GOLDENS for kw in OPTION_SETS])
    assert tables > 0


def test_crafted(host_main, tmp_path):
    paths = crafted_files(str(tmp_path), 200)
    tables, errors = run_all(host_main, [(p, OPTION_SETS[k % 3]) for k, p in enumerate(paths)])
    assert tables > 0 and errors > 0
