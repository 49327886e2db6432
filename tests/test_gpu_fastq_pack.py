"""The device FASTQ parser (csrc/fastq_gpu.hip) against the reference packer of tests/fastq_cases.py: the batch that
shk_device_pack_fastq_slice(rank 0, world 1) brings back — n_seg, n_bases, n_reads, n_input_bases, seg_off and every one of the
(n_bases >> 4) + 2 words — on every text of the catalogue, and the route it took: a text that silently went to the host parser
would compare that parser with itself."""
import ctypes as C
import time

import numpy as np
import pytest

import fastq_cases as fc
from sparrowhawk_amd import _lib
from test_fastq_cases import assert_same_batch, host_pack, joined

pytestmark = pytest.mark.gpu

CASES = fc.cases()
SHK_E_PARSE = -3


@pytest.fixture(autouse=True)
def device_parser(monkeypatch):
    monkeypatch.delenv("SHK_HOST_PARSER", raising=False)


def device_pack(lib, f1, f2, k, min_qual, rank=0, world=1):
    """(rc, (words, seg_off, n_reads, n_input_bases) or None, route or message)"""
    out = _lib.ShkPacked()
    up, route = C.c_uint64(0), C.c_char_p()
    rc = lib.shk_device_pack_fastq_slice(f1, len(f1), f2, len(f2) if f2 is not None else 0, k, min_qual, rank, world,
                                         C.byref(out), C.byref(up), C.byref(route))
    what = (route.value or b"").decode()
    if rc != 0:
        return rc, None, what
    try:
        words = np.ctypeslib.as_array(out.bases, shape=((out.n_bases >> 4) + 2,)).copy()
        seg = np.ctypeslib.as_array(out.seg_off, shape=(out.n_seg + 1,)).copy()
        assert int(seg[0]) == 0 and int(seg[-1]) == out.n_bases, (seg[0], seg[-1], out.n_bases)
        return 0, (words, seg, int(out.n_reads), int(out.n_input_bases)), what
    finally:
        lib.shk_packed_free(C.byref(out))


@pytest.mark.parametrize("name", list(CASES))
def test_device_parser_equals_the_reference_word_for_word(lib, name):
    c = CASES[name]
    want = fc.reference(name)
    rc, got, route = device_pack(lib, c.f1, c.f2, c.k, c.min_qual)
    if want is None:
        assert rc == SHK_E_PARSE, (name, rc, route)
        return
    assert rc == 0, (name, rc, route)
    assert route == c.route, (name, "route", route, "expected", c.route)
    if c.route == "host":
        want = host_pack(lib, joined(c), c.k, c.min_qual)          # (the split rule of long runs is the host packer's)
    assert_same_batch(got, want, name)


@pytest.mark.parametrize("name", ["piece_boundaries_k15", "short_and_long_records_share_words_k15", "several_runs_split_by_N_k15"])
def test_the_ranks_of_a_world_of_three_hold_the_segments_in_rank_order(lib, name):
    c = CASES[name]
    whole = fc.reference(name)
    segs, n_reads, n_in = [], 0, 0
    for rank in range(3):
        rc, got, route = device_pack(lib, c.f1, c.f2, c.k, c.min_qual, rank, 3)
        assert rc == 0 and route == "text_slice", (rank, rc, route)
        assert got[2] > 0, rank                                     # (every rank has a share)
        segs += fc.unpack_segments(got[0], got[1])
        n_reads += got[2]; n_in += got[3]
    assert (n_reads, n_in) == (whole[2], whole[3])
    assert segs == fc.unpack_segments(whole[0], whole[1])           # concatenated in rank order, not sorted


def test_the_third_level_of_the_scan_4096x4096_plus_3_records(lib):
    """134 MB of minimal records around six real ones: the record counts are scanned in three levels (more than 4096 * 4096
    items).  The reference is that of the six real records; the minimal ones keep nothing.
    Measured on an MI355X: 0.11 s for the test, 0.02 s of it the call (profiles/fastq_pack/README.txt)."""
    text, six, n_reads, n_in = fc.big_case()
    want = fc.ref_pack(six, 15, 20)
    assert len(want[1]) == 7
    t0 = time.perf_counter()
    rc, got, route = device_pack(lib, text, None, 15, 20)
    print("device parser on %d bytes, %d records: %.2f s" % (len(text), n_reads, time.perf_counter() - t0))
    assert rc == 0 and route == "text_slice", (rc, route)
    assert_same_batch(got, (want[0], want[1], n_reads, n_in), fc.BIG)


def test_an_empty_last_record_is_taken_on_the_slice_route_as_by_the_host_packer_and_the_oracle(lib):
    """read_fastq_share cut every slice where its trailing blank lines begin; the line end that closes an empty quality line
    went with them, and the host parser — which gets such a text, no longer 4 lines per record — called the record truncated."""
    for text in (b"@a\n\n+\n\n", b"@a\n\n+\n\n\n", b"@a\r\n\r\n+\r\n\r\n", CASES["empty_last_record_with_final_newline_k15"].f1):
        want = host_pack(lib, text, 15, 20)
        assert want is not None, text
        assert_same_batch(want, fc.ref_pack(text, 15, 20), text)
        for world in (1, 2):
            n_reads = 0
            for rank in range(world):
                rc, got, route = device_pack(lib, text, None, 15, 20, rank, world)
                assert rc == 0, (text, world, rank, rc, route)
                n_reads += got[2]
                if world == 1:
                    assert_same_batch(got, want, text)
            assert n_reads == want[2], (text, world)
    rc, got, route = device_pack(lib, b"@a\n\n+\n", None, 15, 20)
    assert rc == SHK_E_PARSE and "truncated" in route, (rc, route)
