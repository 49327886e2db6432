"""GPU tests of the two device inflaters (csrc/inflate_gpu.hip: k_bgzf_decode; k_gz_find_starts, k_gz_decode, the window
rounds, k_gz_resolve) on DEFLATE streams written bit by bit — the catalogue of tests/deflate_catalogue.py, pinned against
zlib by tests/test_deflate_streams.py.  Legal streams must be TAKEN with zlib's bytes (the BGZF path has no speculative
step; the member constructions are laid out for the search); streams that are not legal must be declined, or read as the
host reader reads them — never an error, never other bytes.

Where each class of illegal stream is refused in csrc/inflate_gpu.hip, in front of every load or store that depends on the
bad value (k_bgzf_decode and k_gz_decode share read_dynamic, build_code, decode_sym and fixed_codes):
  BTYPE 3, a header behind the data's end     `if (b.overrun() || btype == 3)` at the head of both block loops
  NLEN                                        `if ((len ^ nlen) != 0xFFFFu || b.overrun())`, in front of the stored copy
  stored bytes beyond the block / its ISIZE   `if (at + len > in_end)`, `if (len > isize - pos)` (BZ_TOO_LONG)
  HLIT / HDIST fields 30, 31                  read_dynamic: `if (hlit > 286 || hdist > 30) return false`, in front of h.len
  16 as the first length, a run too long      read_dynamic: `if (i == 0) return false`, `if (i + rep > total) return false`
  a cut header                                read_dynamic: `if (s < 0 || b.overrun()) return false` per code-length symbol
  length sets over-subscribed / incomplete    build_code: `if (!used || over)`, `if (left > 0 && !(allow_single ...))`, in front
                                              of the symbol sort and the table (the code-length code of ONE code passes
                                              here, unlike in zlib; every such header is then refused for its literal set)
  no end-of-block code                        read_dynamic: `if (h.len[256] == 0) return false`
  length symbols 286, 287                     `if (s > 285)` in front of len_code
  distance symbols 30, 31, no distance code   decode_sym returns -1 (no table entry, maxlen 0); `if (ds < 0 || ds > 29)`
  a distance in front of the first byte       `if (dist > pos)` / `if ((dist > pos && known_window) || dist > pos + GZ_WSIZE)`
  more text than ISIZE                        `if (pos >= isize)` in front of the literal's ring store, `if (len > isize - pos)`
                                              in front of the copy (BZ_TOO_LONG); a member: room per flush (GZ_NO_ROOM), then
                                              "ISIZE mismatch" on the host
  less text, a byte behind the final block    BZ_TOO_SHORT, BZ_NOT_AT_END after the loop
"""
import ctypes as C
import zlib

import pytest

import deflate_catalogue as dc
import deflate_writer as dw
from sparrowhawk_amd import AssemblyHelper, synth
from util import with_env

pytestmark = pytest.mark.gpu

LEAD = b"@lead\nACGT\n+\nIIII\n"
BGZF_ENV = {"SHK_GUNZIP_DEVICE_MIN": 0, "SHK_GUNZIP_DEVICE_WINDOW": None, "SHK_GUNZIP_DEVICE": None}
_cache = {}


def device_gunzip(lib, z, env=BGZF_ENV):
    def run():
        out, n, why = C.c_void_p(), C.c_size_t(), C.c_char_p()
        rc = lib.shk_device_gunzip(z, len(z), C.byref(out), C.byref(n), C.byref(why), None)
        if rc == 0:
            got = C.string_at(out.value, n.value)
            lib.shk_host_free(out)
            return 0, got, ""
        return rc, None, (why.value or b"").decode()
    return with_env(env, run)


def host_gunzip(lib, z):
    out, n = C.c_void_p(), C.c_size_t()
    rc = lib.shk_host_gunzip(z, len(z), C.byref(out), C.byref(n), None, None)
    if rc:
        return rc, None
    got = C.string_at(out.value, n.value)
    lib.shk_host_free(out)
    return 0, got


def legal():
    return [(name, d, text) for name, d, text, ok in dc.catalogue() if ok]


def lead_block():
    return dw.bgzf_block(dw.Stream().fixed(list(LEAD), True).bytes(), LEAD)


def whole_file():
    if "whole" not in _cache:
        _cache["whole"] = (dw.bgzf_file([dw.bgzf_block(d, text) for _, d, text in legal()]), b"".join(text for _, _, text in legal()))
    return _cache["whole"]


def test_bgzf_every_legal_stream_is_taken(lib):
    """every legal entry as a BGZF file of its own, and the whole catalogue as one file: rc 0 and zlib's bytes.  (An entry
    without text — an empty stored or fixed block alone — stands behind a small block of text: a file without any text is
    declined by design, "empty or beyond 4 GiB".)"""
    for name, d, text in legal():
        blocks = [dw.bgzf_block(d, text)] if text else [lead_block(), dw.bgzf_block(d, text)]
        want = text if text else LEAD
        rc, got, why = device_gunzip(lib, dw.bgzf_file(blocks))
        assert rc == 0, (name, rc, why)
        assert got == want, (name, len(got), len(want))
    z, want = whole_file()
    rc, got, why = device_gunzip(lib, z)
    assert rc == 0, (rc, why)
    assert got == want


ALIGNED = ["match_at_the_ring_limits_gz", "match_at_the_ring_limits_bgzf", "match_258_runs_that_wrap_the_ring",
           "match_258_at_1_second_symbol_fixed", "forty_blocks_of_alternating_types"] + ["stored_from_bit_phase_%d" % p for p in range(8)]


@pytest.mark.parametrize("p", list(range(9)) + list(range(252, 261)))
def test_bgzf_blocks_at_every_alignment_of_the_text(lib, p):
    """The ring-limit matches, the 258-at-1 runs, the stream of alternating block types and the stored blocks from every bit
    phase behind a first block of p bytes of text: out_off takes every residue modulo 4 and both sides of a group of 256
    bytes (store_range shares dwords between neighbouring blocks' waves)."""
    by_name = {name: (d, text) for name, d, text in legal()}
    first = dc.fastq_text(p, 40 + p)
    blocks = ([dw.bgzf_block(dw.Stream().stored(first, True).bytes(), first)] if p else []) + [dw.bgzf_block(*by_name[n]) for n in ALIGNED]
    want = first + b"".join(by_name[n][1] for n in ALIGNED)
    rc, got, why = device_gunzip(lib, dw.bgzf_file(blocks))
    assert rc == 0, (rc, why)
    assert got == want


def test_bgzf_three_hundred_tiny_blocks(lib):
    """300 blocks of 1 .. 5 bytes of text each, stored, fixed and dynamic in turn: every wave's text lies inside a dword or
    two that it shares with its neighbours"""
    text = dc.fastq_text(2000, 77)
    blocks, at = [], 0
    for i in range(300):
        piece = text[at:at + 1 + i % 5]
        at += len(piece)
        s = dw.Stream()
        if i % 3 == 0:
            s.stored(piece, True)
        elif i % 3 == 1:
            s.fixed(list(piece), True)
        else:
            dc.emit(s, dc.dyn(list(piece)), True)
        assert zlib.decompress(s.bytes(), -15) == piece
        blocks.append(dw.bgzf_block(s.bytes(), piece))
    rc, got, why = device_gunzip(lib, dw.bgzf_file(blocks))
    assert rc == 0, (rc, why)
    assert got == text[:at]


def test_bgzf_whole_catalogue_through_the_windows(lib):
    """SHK_GUNZIP_DEVICE_WINDOW=65536: the same file window by window, the same bytes"""
    z, want = whole_file()
    rc, got, why = device_gunzip(lib, z, dict(BGZF_ENV, SHK_GUNZIP_DEVICE_WINDOW=65536))
    assert rc == 0, (rc, why)
    assert got == want


def test_bgzf_streams_that_are_not_legal_are_declined_or_read_as_the_host_reads_them(lib):
    """every entry that is not legal as the middle block among legal ones: declined (1), or taken with exactly
    shk_host_gunzip's bytes; never an error.  (The lines that refuse each class stand in this module's docstring.)"""
    declined = 0
    for name, d, text, ok in dc.catalogue():
        if ok:
            continue
        z = dw.bgzf_file([lead_block(), dw.bgzf_block(d, text), lead_block()])
        rc, got, why = device_gunzip(lib, z)
        assert rc in (0, 1), (name, rc, why)
        if rc == 0:
            assert (0, got) == host_gunzip(lib, z), name
        declined += rc
    assert declined >= 30, declined


MEMBER_ENV = {"SHK_GUNZIP_DEVICE_MIN": 32768, "SHK_GUNZIP_DEVICE_WINDOW": None, "SHK_GUNZIP_DEVICE": None, "SHK_GUNZIP_DEVICE_RATIO": None}


def odd_member():
    """250 KB of deflate data: a landing block (about 1 KB) in front of every catalogue entry, so that most cuts of 4096
    bytes have a block start behind them; the entries of more than 2500 bytes once (four of them hold no block start for
    several cuts), the block of 65 280 stored bytes left out"""
    if "odd" not in _cache:
        d, text, m = dc.device_member(250000)
        assert m.entries == set(dc.recipes()) - {"stored_len_65280"}
        assert zlib.decompress(d, -15) == text
        _cache["odd"] = (dw.gzip_member(d, text), text, m.landings)
    return _cache["odd"]


def text_of_three_chunks(landings, chunk):
    """An upper bound of the text of three consecutive chunks, the smallest there is: cuts k .. k + 3 each have a landing
    block behind them in their own range of `chunk` bytes, so chunks start in all four ranges, and chunks k, k + 1, k + 2
    lie between the last landing block in front of cut k and the first one in range k + 3.  None: no such k."""
    first = {}
    for at, text in landings:
        first.setdefault(at // chunk, text)
    spans = [first[k + 3] - max(t for at, t in landings if at < k * chunk)
             for k in range(1, max(first)) if all(j in first for j in range(k, k + 4))]
    return min(spans) if spans else None


@pytest.mark.parametrize("chunk", [4096, 16384])
def test_member_of_odd_blocks_is_taken(lib, chunk):
    """The member decoder on every legal catalogue entry, BFINAL cleared, between landing blocks: in chunk 0 with its window
    known, in later chunks in marker mode — stored and fixed blocks decoded into 16-bit symbols, 15-bit codes, matches that
    copy markers, markers at window positions 0 and 32 767 (landing blocks that start with (258, 32768) and (3, 1)).  Cut
    every 4096 bytes, three consecutive chunks hold less than a window of text, so a window chains through at least three
    chunks in front of it (k_gz_win_init's short-chunk branch, several k_gz_win_round steps), and chunk 0 is shorter than a
    window: the window in front of chunk 1 keeps entries for bytes in front of the stream's first, which no symbol uses.
    A decline fails."""
    z, text, landings = odd_member()
    assert text_of_three_chunks(landings, 4096) < 32768
    assert min(t for at, t in landings if at >= 4096) < 32768          # chunk 1 starts at or before this landing block
    rc, got, why = device_gunzip(lib, z, dict(MEMBER_ENV, SHK_GUNZIP_DEVICE_CHUNK=chunk))
    assert rc == 0, (rc, why)
    assert got == text


def test_member_of_258_at_1_runs_needs_its_room(lib):
    """A member that is mostly matches of 258 at distance 1 inflates 16-fold: declined at the default room of 10 symbols per
    byte with that reason, taken with zlib's bytes once SHK_GUNZIP_DEVICE_RATIO is twice the stream's own ratio."""
    d, text, _ = dc.runs_member(150000, 80)
    assert zlib.decompress(d, -15) == text
    ratio = -(-len(text) // len(d))
    assert 10 < ratio < 32                                   # (ISIZE stays under 64 times the stream: no "ISIZE out of proportion")
    z = dw.gzip_member(d, text)
    env = dict(MEMBER_ENV, SHK_GUNZIP_DEVICE_CHUNK=4096)
    rc, got, why = device_gunzip(lib, z, env)
    assert (rc, why) == (1, "a chunk inflates beyond its room")
    rc, got, why = device_gunzip(lib, z, dict(env, SHK_GUNZIP_DEVICE_RATIO=2 * ratio))
    assert rc == 0, (rc, why)
    assert got == text


@pytest.mark.parametrize("refuse", ["first", "symbol 30"])
def test_member_with_a_bad_block_is_declined_by_its_chunk(lib, refuse):
    """a fixed block with a distance in front of the stream's first byte as the member's first block (chunk 0: the window is
    known), and one with distance symbol 30 in a later chunk: the chunk's decoder stops there (the reason is the chunk's, in
    front of every check of the trailer), no error"""
    d, text, m = dc.device_member(150000, refuse)
    assert (m.refused_at[0] == 0) == (refuse == "first") and (refuse == "first" or m.refused_at[0] > 8 * 4096)
    with pytest.raises(zlib.error):
        zlib.decompress(d, -15)
    rc, got, why = device_gunzip(lib, dw.gzip_member(d, text), dict(MEMBER_ENV, SHK_GUNZIP_DEVICE_CHUNK=4096))
    assert (rc, why) == (1, "a chunk does not end where the next begins")


def test_member_that_reaches_in_front_of_its_first_byte_from_a_later_chunk(lib):
    """Chunk 0 is shorter than a window, and in a later chunk (marker mode) a match reaches one byte in front of the stream's
    first: every chunk ends where the next begins and ISIZE agrees with the symbols counted, so the windows are made, the
    marker finds an entry no window round could resolve, and k_gz_resolve refuses the member for it — not the CRC."""
    d, text, m = dc.device_member(150000, "front")
    at, so_far = m.refused_at
    assert at >= 10240 and so_far < 32768 and min(t for a, t in m.landings if a >= 4096) < 32768
    with pytest.raises(zlib.error):
        zlib.decompress(d, -15)
    rc, got, why = device_gunzip(lib, dw.gzip_member(d, text), dict(MEMBER_ENV, SHK_GUNZIP_DEVICE_CHUNK=4096))
    assert (rc, why) == (1, "a back-reference in front of the stream")


def test_shaped_streams_through_preprocess():
    """One FASTQ text written as a BGZF file and as a gzip member of landing, fixed, 15-bit dynamic and stored blocks, through
    shk_preprocess: both take their device route, and reads and counts equal those of the plain text."""
    g = synth.random_genome(20000, 15)
    codes, quals = synth.sample_reads(g, 1500, 150, 16, err=0.01)
    fq = bytes(synth.to_fastq_fixed(codes, quals))
    bgzf, member = dc.shaped_streams(fq)
    assert zlib.decompress(member, 31) == fq

    def product(data):
        h = AssemblyHelper.new(31, True, 3, 20, 0, False, False, False, False)
        h.preprocess(data, None)
        h.assemble()
        return h

    def run():
        a, b, c = product(fq), product(bgzf), product(member)
        tb, tc = b.timings(), c.timings()
        assert tb.get("gunzip_device_bgzf_blocks_x1", 0) == (len(fq) + 4999) // 5000 and "gunzip_host_clock" not in tb, tb
        assert tc.get("gunzip_device_members_x1", 0) == 1 and "gunzip_device_bgzf_blocks_x1" not in tc and "gunzip_host_clock" not in tc, tc
        want = (a.get_assembly(), a.get_preprocessing_info())
        assert (b.get_assembly(), b.get_preprocessing_info()) == want
        assert (c.get_assembly(), c.get_preprocessing_info()) == want
    with_env(dict(MEMBER_ENV, SHK_GUNZIP_DEVICE_CHUNK=4096), run)
