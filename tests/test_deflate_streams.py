"""CPU tests of the host inflaters on DEFLATE streams written bit by bit (tests/deflate_writer.py, the catalogue of
tests/deflate_catalogue.py): 15-bit codes, blocks without a distance code or with one, HCLEN 5 and 19, repeat runs across
the literal/distance boundary, empty blocks, stored blocks from every bit phase, every length and distance symbol at both
ends of its class — and the streams that have to be refused.  zlib's inflater pins the writer (it is the reference, not the
product); the product's readers (shk_host_gunzip: zlib per BGZF block, csrc/inflate_mt.cpp for a large member) must hand
on zlib's bytes, and csrc/inflate_mt.cpp must TAKE its member: a decline would compare zlib with itself."""
import ctypes as C
import zlib

import pytest

import deflate_catalogue as dc
import deflate_writer as dw
from util import with_env

LEAD = b"@lead\nACGT\n+\nIIII\n"


def host_gunzip(lib, z, want_mt=False):
    out, n, mt = C.c_void_p(), C.c_size_t(), C.c_uint64()
    rc = lib.shk_host_gunzip(z, len(z), C.byref(out), C.byref(n), C.byref(mt), None)
    if rc:
        return (rc, None, mt.value) if want_mt else (rc, None)
    got = C.string_at(out.value, n.value)
    lib.shk_host_free(out)
    return (0, got, mt.value) if want_mt else (0, got)


def zlib_raw(d):
    """(bytes, ended in the final block, bytes left over) — or the error zlib raises"""
    o = zlib.decompressobj(-15)
    try:
        got = o.decompress(d)
    except zlib.error as e:
        return e
    return got, o.eof, len(o.unused_data)


def lead_block():
    return dw.bgzf_block(dw.Stream().fixed(list(LEAD), True).bytes(), LEAD)


def test_zlib_reads_every_legal_stream_and_refuses_every_other():
    """Every legal entry: zlib gives exactly the expansion of the tokens and the stream ends in its last byte.  Every other
    entry: zlib raises on the raw stream, or does not reach the final block, or gives a text that is not the trailer's
    (then it raises on the gzip member: `incorrect data check` / `incorrect length check`), or leaves a byte unused."""
    cat = dc.catalogue()
    assert len({name for name, _, _, _ in cat}) == len(cat)
    for name, d, text, legal in cat:
        r = zlib_raw(d)
        if legal:
            assert r == (text, True, 0), name
            assert zlib.decompress(dw.gzip_member(d, text), 31) == text, name
            continue
        if isinstance(r, zlib.error):
            continue
        if name == "a_byte_behind_the_final_block":
            assert r == (text, True, 1)
        else:
            assert not r[1] or r[0] != text, name
        with pytest.raises(zlib.error):
            zlib.decompress(dw.gzip_member(d, text), 31)


def test_the_catalogue_holds_what_its_names_say():
    """the properties the decoders' paths hang on, read back from the blocks: code lengths above the tables' widths, the
    header fields, the bit phases, the run symbols"""
    rec = dc.recipes()
    for m in (11, 12, 15):
        assert max(rec["dyn_literal_code_max_%d" % m][0][2]) == m > dc.LIT_PB
    assert dc.HOST_LIT_PB < 12
    for m in (10, 15):
        assert max(rec["dyn_distance_code_max_%d" % m][0][3]) == m > dc.DIST_PB
    b = rec["dyn_code_length_code_7_bits_hclen_19"][0]
    cl = b[4]["cl_plan"]["cl_lens"]
    assert max(cl) == 7 and cl[15] and dw.kraft(cl, 7) == 128                   # (15 is the last in the header's order: HCLEN = 19)
    assert max(b[2]) == 15
    assert rec["dyn_hlit_257_no_distance_code"][0][3] == [0] and max(i for i, l in enumerate(rec["dyn_hlit_257_no_distance_code"][0][2]) if l) == 256
    assert sum(1 for l in rec["dyn_one_distance_code_symbol_8"][0][3] if l) == 1 and rec["dyn_one_distance_code_symbol_8"][0][3][8] == 1
    assert rec["dyn_hdist_1_one_distance_code"][0][3] == [1]
    b = rec["dyn_end_of_block_is_the_one_bit_code"][0]
    assert b[2][256] == 1 and b[2].count(1) == 1
    phases = set()
    for k in range(8):
        v, n = dw.fixed_bits(dc.thirteen_bit_matches(k), False)
        assert n == 106 + 13 * k
        phases.add(n % 8)
    assert phases == set(range(8))
    for k, bit in ((4, 7), (1, 0)):
        name = "final_empty_fixed_block_ends_at_bit_%d" % bit
        d = next(d for n, d, _, _ in dc.catalogue() if n == name)
        total = 106 + 13 * k + 10
        assert len(d) == (total + 7) // 8 and (total - 1) % 8 == bit
    order = "".join(b[0][0] for b in rec["forty_blocks_of_alternating_types"])
    assert len(order) == 40 and {order[i:i + 2] for i in range(39)} == {a + b for a in "sfd" for b in "sfd"}
    # every length 3 .. 258 class end and every distance class end is there, by symbol
    lens = {dw.token_match(t)[0] for t in rec["fixed_every_length_symbol"][0][1] if not isinstance(t, int)}
    assert lens == {dw.LEN_BASE[c] for c in range(29)} | {dw.LEN_BASE[c] + (1 << dw.LEN_EXTRA[c]) - 1 for c in range(29)} and 258 in lens
    dists = {dw.token_match(t)[1] for t in rec["fixed_every_distance_symbol"][1][1] if not isinstance(t, int)}
    assert dists == {dw.DIST_BASE[c] for c in range(30)} | {dw.DIST_BASE[c] + (1 << dw.DIST_EXTRA[c]) - 1 for c in range(30)} and 32768 in dists
    # a stream of 2 MiB assembles in about a second (the blocks are ints joined by shift / or)
    s = dw.Stream()
    v, n = dw.fixed_bits(list(b"ACGT" * 64), False)
    for _ in range((2 << 20) * 8 // n + 1):
        s.raw(v, n)
    assert len(s.stored(b"", True).bytes()) >= 2 << 20


def test_host_reader_on_legal_streams_in_bgzf_blocks(lib):
    """every legal entry as a BGZF file of its own, and the whole catalogue as one file with an end-of-file block: the text
    comes back byte for byte"""
    legal = [(name, d, text) for name, d, text, ok in dc.catalogue() if ok]
    for name, d, text in legal:
        assert host_gunzip(lib, dw.bgzf_file([dw.bgzf_block(d, text)])) == (0, text), name
        assert host_gunzip(lib, dw.gzip_member(d, text)) == (0, text), name
    z = dw.bgzf_file([dw.bgzf_block(d, text) for _, d, text in legal])
    assert host_gunzip(lib, z) == (0, b"".join(text for _, _, text in legal))


def test_host_reader_refuses_what_zlib_refuses(lib):
    """every entry that is not legal, as the middle block of a BGZF file and as a gzip member: an error, never other bytes.
    (A byte behind the final block: zlib stops in front of it and has the text; the BGZF reader takes the block — its text
    is the trailer's — and the member reader refuses the shifted trailer.)"""
    for name, d, text, ok in dc.catalogue():
        if ok:
            continue
        rc, got = host_gunzip(lib, dw.bgzf_file([lead_block(), dw.bgzf_block(d, text), lead_block()]))
        if name == "a_byte_behind_the_final_block":
            assert (rc, got) == (0, LEAD + text + LEAD)
        else:
            assert rc != 0 and got is None, name
        rc, got = host_gunzip(lib, dw.gzip_member(d, text))
        assert rc != 0 and got is None, name


MT_DEFLATE = (2 << 20) + 4096
_member = {}


def mt_member():
    """One gzip member just above the multi-threaded reader's thresholds (csrc/fastq.cpp: 2 MiB of file; csrc/inflate_mt.cpp:
    1 MiB of deflate data, 512 KiB per chunk): tests/deflate_catalogue.py host_member, with a landing block whose first
    symbol is (258, 32768) right behind every cut the reader makes with 2, 3 and 8 threads (2, 3 and 4 chunks).  The entries
    of binary data are in it too: the reader's text check looks at the block a search lands on, and those are the landing
    blocks."""
    if not _member:
        dn = MT_DEFLATE + 8                                  # (the reader counts the trailer in)
        cuts = sorted({(dn // c) * i for c in (2, 3, 4) for i in range(1, c)})
        d, text, m = dc.host_member(MT_DEFLATE, cuts)
        assert len(cuts) == 5 and m.entries == set(dc.recipes())
        assert zlib_raw(d) == (text, True, 0)
        _member["m"] = (dw.gzip_member(d, text), text)
    return _member["m"]


@pytest.mark.parametrize("threads", [2, 3, 8])
def test_multi_threaded_host_reader_takes_the_member_of_odd_blocks(lib, threads):
    """SHK_GUNZIP_THREADS 2, 3, 8: the member is TAKEN by csrc/inflate_mt.cpp (mt_members goes up by one) and the bytes are
    zlib's.  Behind every cut stand markers at both ends of the unknown window (the landing block starts with a match of 258
    at distance 32 768; the block behind it reaches the chunk's first byte and the byte in front of it), matches at 32 767
    and 32 768 copy them on, and every legal catalogue entry follows with BFINAL cleared."""
    z, text = mt_member()
    assert len(z) >= 2 << 20
    before = host_gunzip(lib, dw.gzip_member(b"\x03\x00", b""), True)[2]

    def run():
        return host_gunzip(lib, z, True)
    rc, got, mt = with_env({"SHK_GUNZIP_THREADS": threads}, run)
    assert rc == 0 and got == text
    assert mt - before == 1, "declined by the multi-threaded reader"


def test_multi_threaded_host_reader_on_a_chunk_shorter_than_a_window(lib):
    """Three threads, three chunks, the middle one of less than 32 KiB of text (512 KiB of stored blocks in front of it hold
    no block start): the window in front of the last chunk is made of the middle chunk and of the tail of the window in
    front of THAT (csrc/inflate_mt.cpp, `have < WSIZE`), and matches at 32 767 and 32 768 read it.  Taken, zlib's bytes."""
    dn = MT_DEFLATE + 8
    d, text, m = dc.host_member_with_a_short_chunk(MT_DEFLATE, dn // 3, (dn // 3) * 2)
    assert 0 < m.short_chunk_text < 32768 - 258
    assert zlib_raw(d) == (text, True, 0)
    z = dw.gzip_member(d, text)
    before = host_gunzip(lib, dw.gzip_member(b"\x03\x00", b""), True)[2]
    rc, got, mt = with_env({"SHK_GUNZIP_THREADS": 3}, lambda: host_gunzip(lib, z, True))
    assert rc == 0 and got == text
    assert mt - before == 1, "declined by the multi-threaded reader"
