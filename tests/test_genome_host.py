"""preprocessGenome's FASTA reader (epi_read_genome) and the BGZF writer behind callMethylation (epi_bgzf_write_file):
host code, no GPU."""
import gzip
import os
import struct
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAMS = os.path.join(ROOT, "tests", "golden", "bam")

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")

# wrapped lines, lower case, IUPAC codes, an empty line, a header with a description, a CRLF line
FASTA = (">seq1 first sequence, with a description\n"
         "ACGTacgtNNnnRYKM\n"
         "SWBDHV-.*acg\n"
         "\n"
         ">seq2\tsecond\r\n"
         "TTTTGGGGCCCCAAAA\r\n"
         "gattaca\n"
         ">seq3\n"
         "N\n")
WANT = {"seq1": b"ACGTACGTNNNNNNNNNNNNNNNNNACG", "seq2": b"TTTTGGGGCCCCAAAAGATTACA", "seq3": b"N"}


@pytest.fixture(scope="module")
def ea():
    import epialleler_amd
    return epialleler_amd


def _bgzip(data, path):
    """A BGZF file as HTSlib's bgzip writes it (independent of the library's writer)."""
    with open(path, "wb") as f:
        for i in range(0, len(data), 0xff00):
            chunk = data[i:i + 0xff00]
            co = zlib.compressobj(6, zlib.DEFLATED, -15)
            comp = co.compress(chunk) + co.flush()
            f.write(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(comp) + 25) + comp +
                    struct.pack("<II", zlib.crc32(chunk) & 0xFFFFFFFF, len(chunk)))
        f.write(EOF_BLOCK)


def _genome_dict(g):
    return {g.rname[i]: g.sequence(i) for i in range(len(g))}


def test_reference_fasta(ea):
    g = ea.preprocessGenome(os.path.join(BAMS, "reference.fasta.gz"), verbose=False)
    assert g.rname == ["ChrA", "ChrB", "ChrC"]
    assert g.rlen.tolist() == [4900, 4900, 4900]
    assert g.rid.tolist() == [0, 1, 2]
    assert all(set(g.sequence(i)) <= set(b"ACGTN") for i in range(3))
    with gzip.open(os.path.join(BAMS, "reference.fasta.gz"), "rb") as f:        # this one is plain upper-case ACGTN
        lines = f.read().decode().split("\n")
    heads = [i for i, ln in enumerate(lines) if ln.startswith(">")]
    assert lines[heads[0]].startswith(">ChrA ")                                   # a header with a description
    first = "".join(lines[heads[0] + 1:heads[1]])
    assert g.sequence(0) == first.encode()
    assert ea.preprocessGenome(g) is g                                            # already a genome: unchanged


@pytest.mark.parametrize("form", ["plain", "gzip", "bgzf"])
def test_fasta_forms(ea, form, tmp_path):
    data = FASTA.encode()
    path = str(tmp_path / ("g.fa" + ("" if form == "plain" else ".gz")))
    if form == "plain":
        open(path, "wb").write(data)
    elif form == "gzip":
        with gzip.open(path, "wb") as f:
            f.write(data)
    else:
        _bgzip(data, path)
    g = ea.preprocessGenome(path, nthreads=2, verbose=False)
    assert _genome_dict(g) == WANT
    assert g.rname == ["seq1", "seq2", "seq3"]
    assert g.rlen.tolist() == [len(WANT[k]) for k in ("seq1", "seq2", "seq3")]


def test_fasta_errors(ea, tmp_path):
    dup = str(tmp_path / "dup.fa")
    open(dup, "w").write(">a\nACGT\n>b\nAC\n>a desc\nGG\n")
    with pytest.raises(ValueError, match="duplicate"):
        ea.preprocessGenome(dup, verbose=False)
    with pytest.raises(ValueError):
        ea.preprocessGenome(str(tmp_path / "missing.fa"), verbose=False)
    bad = str(tmp_path / "bad.fa")
    open(bad, "w").write("ACGT\n>a\nAC\n")
    with pytest.raises(ValueError):
        ea.preprocessGenome(bad, verbose=False)


@pytest.mark.parametrize("n,nthreads", [(0, 1), (1, 1), (0xff00, 2), (0xff00 + 1, 3), (1 << 20, 4), (3_000_001, 8)])
def test_bgzf_writer_round_trip(ea, n, nthreads, tmp_path):
    from epialleler_amd import _lib
    rng = np.random.default_rng(n)
    # half compressible text, half random bytes (blocks that do not shrink)
    data = (b"ACGTTGCA" * (n // 16 + 1))[:n // 2] + rng.integers(0, 256, n - n // 2, dtype=np.uint8).tobytes()
    buf = np.frombuffer(data, np.uint8) if n else np.zeros(1, np.uint8)
    path = str(tmp_path / "out.gz")
    _lib.check(_lib.load().epi_bgzf_write_file(path.encode(), buf.ctypes.data, n, nthreads))
    with gzip.open(path, "rb") as f:
        assert f.read() == data
    raw = open(path, "rb").read()
    assert raw.endswith(EOF_BLOCK)
    p, sizes = 0, []
    while p < len(raw):
        assert raw[p:p + 4] == b"\x1f\x8b\x08\x04"
        assert struct.unpack_from("<H", raw, p + 10)[0] == 6 and raw[p + 12:p + 16] == b"BC\x02\x00"
        bsize = struct.unpack_from("<H", raw, p + 16)[0] + 1
        crc, isize = struct.unpack_from("<II", raw, p + bsize - 8)
        body = zlib.decompress(raw[p + 18:p + bsize - 8], -15)
        assert len(body) == isize and zlib.crc32(body) & 0xFFFFFFFF == crc
        sizes.append(isize)
        p += bsize
    assert p == len(raw)
    assert all(s <= 0xff00 for s in sizes)
    assert sum(sizes) == n and sizes[-1] == 0                                     # ... and the EOF block last


def test_bgzf_writer_bad_path(ea):
    from epialleler_amd import _lib
    buf = np.zeros(4, np.uint8)
    assert _lib.load().epi_bgzf_write_file(b"", buf.ctypes.data, 4, 1) != _lib.EPI_OK
    assert _lib.load().epi_bgzf_write_file(b"/nonexistent-dir/x.gz", buf.ctypes.data, 4, 1) != _lib.EPI_OK
