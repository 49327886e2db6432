"""CPU tests of the BGZF (bgzip) writer sparrowhawk_amd.synth.bgzf_compress — the fixture the GPU tests of the device
inflater's BGZF path (tests/test_gpu_bgzf.py) rest on: its output is valid gzip for Python's reader and for the product's
host reader (shk_host_gunzip: csrc/fastq.cpp, inflate_bgzf), and has the container layout of the SAM specification 4.1."""
import ctypes as C
import gzip
import struct

import numpy as np
import pytest

from sparrowhawk_amd import synth

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")      # SAM specification 4.1.2


def _fastq(n_reads=4000, seed=3):
    g = synth.random_genome(50000, seed)
    codes, quals = synth.sample_reads(g, n_reads, 150, seed + 1, err=0.01)
    return bytes(synth.to_fastq_fixed(codes, quals))


def _host_gunzip(lib, z):
    out, n = C.c_void_p(), C.c_size_t()
    rc = lib.shk_host_gunzip(z, len(z), C.byref(out), C.byref(n), None, None)
    if rc:
        return rc, None
    got = C.string_at(out.value, n.value)
    lib.shk_host_free(out)
    return 0, got


def _blocks(z):
    """[(offset, BSIZE, ISIZE)] of a BGZF file, walked by the header fields alone"""
    out, p = [], 0
    while p < len(z):
        assert z[p:p + 4] == b"\x1f\x8b\x08\x04" and z[p + 10:p + 12] == b"\x06\x00" and z[p + 12:p + 16] == b"BC\x02\x00"
        bsize = struct.unpack_from("<H", z, p + 16)[0] + 1
        assert 26 <= bsize <= 65536 and p + bsize <= len(z)
        out.append((p, bsize, struct.unpack_from("<I", z, p + bsize - 4)[0]))
        p += bsize
    return out


@pytest.mark.parametrize("level", [0, 1, 6, 9])
@pytest.mark.parametrize("block", [65280, 30000, 1000])
@pytest.mark.parametrize("eof", [True, False])
def test_bgzf_writer_gives_valid_gzip_and_the_host_reader_reads_it(lib, level, block, eof):
    fq = _fastq()
    z = synth.bgzf_compress(fq, block=block, level=level, eof=eof)
    assert gzip.decompress(z) == fq
    assert _host_gunzip(lib, z) == (0, fq)
    bl = _blocks(z)
    n_data = (len(fq) + block - 1) // block
    assert len(bl) == n_data + (1 if eof else 0)
    assert [i for _, _, i in bl[:n_data]] == [block] * (n_data - 1) + [len(fq) - block * (n_data - 1)]
    assert z.endswith(EOF_BLOCK) == eof


def test_bgzf_writer_on_empty_and_incompressible_input(lib):
    assert synth.bgzf_compress(b"") == EOF_BLOCK and synth.bgzf_compress(b"", eof=False) == b""
    assert gzip.decompress(EOF_BLOCK) == b"" and _host_gunzip(lib, EOF_BLOCK) == (0, b"")
    # random bytes: zlib falls back to stored blocks, and a full block still fits BSIZE
    noise = np.random.default_rng(5).integers(0, 256, 200_000, dtype=np.uint8).tobytes()
    for level in (0, 6):
        z = synth.bgzf_compress(noise, level=level)
        assert max(b for _, b, _ in _blocks(z)) <= 65536
        assert gzip.decompress(z) == noise and _host_gunzip(lib, z) == (0, noise)
    # two files behind one another (an empty block in mid-file) and a last block of one byte
    fq = _fastq(500)
    z = synth.bgzf_compress(fq) + synth.bgzf_compress(fq[:65281])
    assert _blocks(z)[-2][2] == 1
    assert gzip.decompress(z) == fq + fq[:65281] and _host_gunzip(lib, z) == (0, fq + fq[:65281])
    with pytest.raises(ValueError):
        synth.bgzf_compress(fq, block=65281)
