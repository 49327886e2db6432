"""GPU tests of the device inflater's BGZF path (csrc/inflate_gpu.hip: k_bgzf_decode, one wave per block, and k_bgzf_crc):
a bgzip-compressed FASTQ is inflated on the device, alone (shk_device_gunzip) and through shk_preprocess; intact files are
all taken, damaged ones are declined or read as the host reader reads them, and the results equal those of the plain text
and of the oracle.  The files come from sparrowhawk_amd.synth.bgzf_compress (pinned by tests/test_bgzf_host.py)."""
import ctypes as C
import gzip
import struct

import numpy as np
import pytest

from sparrowhawk_amd import AssemblyHelper, ShkError, synth
from util import compare_all, run_oracle

pytestmark = pytest.mark.gpu

EOF_BLOCK = synth.bgzf_compress(b"")
_cache = {}


def fastq_text():
    """18.96 MB: 60 000 reads of 150 from a 200 kbp genome, one base in a hundred wrong and of low quality"""
    if "fq" not in _cache:
        g = synth.random_genome(200000, 15)
        codes, quals = synth.sample_reads(g, 60000, 150, 16, err=0.01)
        _cache["fq"] = bytes(synth.to_fastq_fixed(codes, quals))
    return _cache["fq"]


def bgzf(level=6, block=65280):
    key = ("z", level, block)
    if key not in _cache:
        _cache[key] = synth.bgzf_compress(fastq_text(), block=block, level=level)
    return _cache[key]


def blocks_of(z):
    """[(offset, BSIZE)] of an intact BGZF file"""
    out, p = [], 0
    while p < len(z):
        bsize = struct.unpack_from("<H", z, p + 16)[0] + 1
        out.append((p, bsize))
        p += bsize
    return out


def device_gunzip(lib, z):
    out, n, why = C.c_void_p(), C.c_size_t(), C.c_char_p()
    rc = lib.shk_device_gunzip(z, len(z), C.byref(out), C.byref(n), C.byref(why), None)
    if rc == 0:
        got = C.string_at(out.value, n.value)
        lib.shk_host_free(out)
        return 0, got, ""
    return rc, None, (why.value or b"").decode()


def host_gunzip(lib, z):
    out, n = C.c_void_p(), C.c_size_t()
    rc = lib.shk_host_gunzip(z, len(z), C.byref(out), C.byref(n), None, None)
    if rc:
        return rc, None
    got = C.string_at(out.value, n.value)
    lib.shk_host_free(out)
    return 0, got


def product(fq1, fq2=None, k=31, min_count=3, min_qual=20):
    h = AssemblyHelper.new(k, True, min_count, min_qual, 0, False, False, False, False)
    h.preprocess(fq1, fq2)
    h.assemble()
    return h


def outputs(h):
    return h.get_assembly(), h.get_preprocessing_info()


def outcome(*files):
    """what a user sees of a run: the error code, or the outputs"""
    try:
        return outputs(product(*files))
    except ShkError as e:
        return e.code


def test_intact_bgzf_files_are_all_taken(lib, monkeypatch):
    """Every intact file comes back from the device byte for byte: levels 0 (stored blocks), 1, 6, 9; blocks of 65 280,
    30 000 and 1 000 bytes of text; a text without a final newline; empty blocks in mid-file; no end-of-file block; two files
    behind one another; a last block of one byte.  This path has no speculative step: none may be declined."""
    monkeypatch.setenv("SHK_GUNZIP_DEVICE_MIN", "32768")
    fq = fastq_text()
    part = fq[:5_000_000]
    cut = 65280 * 20
    cases = [("level %d" % lv, bgzf(lv), fq) for lv in (0, 1, 6, 9)]
    cases += [("blocks of 30000", bgzf(6, 30000), fq), ("blocks of 1000", bgzf(6, 1000), fq)]
    cases += [("no final newline", synth.bgzf_compress(part[:-1]), part[:-1]),
              ("empty blocks in mid-file", synth.bgzf_compress(part[:cut], eof=False) + EOF_BLOCK + EOF_BLOCK + synth.bgzf_compress(part[cut:]), part),
              ("no end-of-file block", synth.bgzf_compress(part, eof=False), part),
              ("two files", synth.bgzf_compress(part[:cut], level=1) + synth.bgzf_compress(part[cut:], block=30000, level=9), part),
              ("a last block of one byte", synth.bgzf_compress(part[:cut + 1]), part[:cut + 1]),
              ("a first block of one byte", synth.bgzf_compress(part[:1], eof=False) + synth.bgzf_compress(part[1:]), part),
              ("blocks of 777, stored", synth.bgzf_compress(part[:1_000_000], block=777, level=0), part[:1_000_000])]
    for name, z, want in cases:
        assert gzip.decompress(z) == want, name
        rc, got, why = device_gunzip(lib, z)
        assert rc == 0, (name, rc, why)
        assert got == want, (name, len(got), len(want))


def test_damaged_bgzf_is_declined_or_read_as_the_host_reads_it(lib, monkeypatch):
    """The decline rules against the host reader: whatever is done to a file, the device inflater declines it (1) or gives
    the bytes shk_host_gunzip gives.  Never other bytes."""
    monkeypatch.setenv("SHK_GUNZIP_DEVICE_MIN", "32768")
    z = bgzf(6)
    bl = blocks_of(z)
    assert len(bl) == 292
    rng = np.random.default_rng(20261)

    def put(at, fmt, value):
        b = bytearray(z)
        struct.pack_into(fmt, b, at, value)
        return bytes(b)

    def trailer(i, field):                                   # offset of CRC-32 (0) / ISIZE (1) of block i
        return bl[i][0] + bl[i][1] - 8 + 4 * field
    isize3 = struct.unpack_from("<I", z, trailer(3, 1))[0]
    crc7 = struct.unpack_from("<I", z, trailer(7, 0))[0]
    cases = [("chain broken behind the first block", put(bl[1][0], "<B", 0x1E)),
             ("garbage appended", z + b"not a block at all, just bytes behind the last one"),
             ("a plain member appended", z + gzip.compress(b"@r\nACGT\n+\nIIII\n")),
             ("cut in mid-block", z[:bl[150][0] + bl[150][1] // 2]),
             ("cut inside the last trailer", z[:-len(EOF_BLOCK) - 3]),
             ("BSIZE one higher", put(bl[5][0] + 16, "<H", bl[5][1])),
             ("BSIZE one lower", put(bl[5][0] + 16, "<H", bl[5][1] - 2)),
             ("ISIZE above 65536", put(trailer(3, 1), "<I", 70000)),
             ("ISIZE one lower", put(trailer(3, 1), "<I", isize3 - 1)),
             ("ISIZE one higher", put(trailer(3, 1), "<I", isize3 + 1)),
             ("ISIZE one lower in the last block", put(trailer(290, 1), "<I", struct.unpack_from("<I", z, trailer(290, 1))[0] - 1)),
             ("CRC-32 flipped", put(trailer(7, 0), "<I", crc7 ^ 0x00010000)),
             ("a non-empty end-of-file block", put(trailer(291, 1), "<I", 1))]
    for j in range(12):
        pos = int(rng.integers(0, len(z))); bit = int(rng.integers(0, 8))
        b = bytearray(z); b[pos] ^= 1 << bit
        cases.append(("bit %d of byte %d flipped" % (bit, pos), bytes(b)))
    # ... and the same for stored blocks and tiny blocks, a few flips each
    for zz, tag in ((bgzf(0)[:blocks_of(bgzf(0))[30][0]], "level 0"), (synth.bgzf_compress(fastq_text()[:300_000], block=1000), "blocks of 1000")):
        assert host_gunzip(lib, zz)[0] == 0, tag
        for j in range(4):
            pos = int(rng.integers(0, len(zz))); bit = int(rng.integers(0, 8))
            b = bytearray(zz); b[pos] ^= 1 << bit
            cases.append(("%s: bit %d of byte %d flipped" % (tag, bit, pos), bytes(b)))
    declined = 0
    for name, bad in cases:
        rc, got, why = device_gunzip(lib, bad)
        assert rc in (0, 1), (name, rc, why)
        if rc == 0:
            assert (0, got) == host_gunzip(lib, bad), name
        declined += rc
    assert declined >= 10, declined                          # (the thirteen constructed cases leave the host nothing valid)


def test_bgzf_through_preprocess(monkeypatch):
    """shk_preprocess on BGZF input: inflated on the device block by block, parsed there (with masked bases: one base in
    a hundred has quality 10 < min_qual 20), results equal to those of the plain text and of the oracle; pairs of BGZF
    files and of a plain member and a BGZF file; SHK_GUNZIP_DEVICE=0 and damaged files give what the host reader gives."""
    monkeypatch.setenv("SHK_GUNZIP_DEVICE_MIN", "65536")
    fq = fastq_text()
    assert fq.count(b"+", 0, 100_000) > fq.count(b"\n", 0, 100_000) // 4      # low qualities ('+') beside the '+' lines: bases get masked
    z = bgzf(6)
    n_blocks = (len(fq) + 65279) // 65280
    a = product(fq)
    b = product(z)
    t = b.timings()
    assert t.get("gunzip_device_bgzf_blocks_x1", 0) == n_blocks, t
    assert t.get("gunzip_device_members_x1", 0) == 1 and "gunzip_host_clock" not in t, t
    assert outputs(b) == outputs(a)
    compare_all(b, run_oracle([fq], k=31, min_count=3, min_qual=20), check_graph=False)
    # pairs: two BGZF files; a plain member and a BGZF file, both orders
    recs = fq.decode().split("@r")[1:]
    half = len(recs) // 2
    f1 = ("@r" + "@r".join(recs[:half])).encode(); f2 = ("@r" + "@r".join(recs[half:])).encode()
    nb1, nb2 = (len(f1) + 65279) // 65280, (len(f2) + 29999) // 30000
    z1, z2 = synth.bgzf_compress(f1, level=1), synth.bgzf_compress(f2, block=30000, level=9)
    pairs = [(z1, z2, nb1 + nb2), (gzip.compress(f1, compresslevel=1), z2, nb2), (z1, gzip.compress(f2, compresslevel=9), nb1)]
    for p1, p2, nb in pairs:
        c = product(p1, p2)
        assert c.timings().get("gunzip_device_members_x1", 0) == 2, c.timings()
        assert c.timings().get("gunzip_device_bgzf_blocks_x1", 0) == nb, c.timings()
        assert outputs(c) == outputs(a)
    # damaged files: the device path on and off give the same outcome
    bl = blocks_of(z)
    broken = bytearray(z); broken[bl[100][0]] ^= 0xFF
    flipped = bytearray(z); flipped[bl[100][0] + bl[100][1] // 2] ^= 0x04
    on = [outcome(bytes(broken)), outcome(bytes(flipped))]
    assert on[0] == -3
    # the switch off: the host reader, the same outputs
    monkeypatch.setenv("SHK_GUNZIP_DEVICE", "0")
    d = product(z)
    assert "gunzip_device_bgzf_blocks_x1" not in d.timings() and "gunzip_host_clock" in d.timings(), d.timings()
    assert outputs(d) == outputs(a)
    e = product(z1, z2)
    assert "gunzip_device_bgzf_blocks_x1" not in e.timings()
    assert outputs(e) == outputs(a)
    assert [outcome(bytes(broken)), outcome(bytes(flipped))] == on


def test_bgzf_below_the_size_floor_is_read_on_the_host(monkeypatch):
    """SHK_GUNZIP_DEVICE_MIN unset: a BGZF file of less than 4 MiB goes to the host reader, as before."""
    monkeypatch.delenv("SHK_GUNZIP_DEVICE_MIN", raising=False)
    monkeypatch.delenv("SHK_GUNZIP_DEVICE", raising=False)
    fq = fastq_text()
    z = bgzf(6)
    assert len(z) < (4 << 20)
    a, b = product(fq), product(z)
    t = b.timings()
    assert "gunzip_device_bgzf_blocks_x1" not in t and t.get("gunzip_device_members_x1", 0) == 0 and "gunzip_host_clock" in t, t
    assert outputs(b) == outputs(a)
    # ... and the same file above the floor is inflated on the device
    monkeypatch.setenv("SHK_GUNZIP_DEVICE_MIN", str(len(z)))
    assert product(z).timings().get("gunzip_device_bgzf_blocks_x1", 0) == (len(fq) + 65279) // 65280
