"""The device FASTA packer (csrc/fasta_gpu.hip) against the reference packer of tests/fasta_cases.py: the batch that
shk_device_pack_fasta brings back — n_seg, n_bases, n_reads, n_input_bases, seg_off and every one of the (n_bases >> 4) + 2
words — on every text of the catalogue, and the route it took: a regular text that silently went to the host packer would
compare that packer with itself, so it fails the test."""
import ctypes as C
import time

import numpy as np
import pytest

import fasta_cases as fa
from sparrowhawk_amd import _lib
from test_fastq_cases import assert_same_batch

CASES = fa.cases()
REGULAR = [n for n, c in CASES.items() if c.ok]
SHK_E_PARSE = -3


def test_the_catalogue_holds_at_least_230_regular_cases():
    """(no GPU) the cap that keeps the device tests honest: none of these may take the host route"""
    assert len(REGULAR) >= 230


def device_pack(lib, f1, f2, k):
    """(rc, (words, seg_off, n_reads, n_input_bases) or None, route or message)"""
    out, route = _lib.ShkPacked(), C.c_char_p()
    rc = lib.shk_device_pack_fasta(f1, len(f1), f2, len(f2) if f2 is not None else 0, k, C.byref(out), C.byref(route))
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


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_device_packer_equals_the_reference_word_for_word(lib, name):
    c = CASES[name]
    want = fa.reference(name)
    rc, got, route = device_pack(lib, c.f1, c.f2, c.k)
    if not c.ok:
        assert want is None
        # the device packer declined, the host packer took the text over and words the refusal
        assert rc == SHK_E_PARSE and route.startswith("host: ") and "FASTA" in route, (name, rc, route)
        return
    assert rc == 0, (name, rc, route)
    assert route == "device", (name, "a regular text went to", route)
    assert_same_batch(got, want, name)


@pytest.mark.gpu
def test_the_second_level_of_the_scan_over_the_chunks(lib):
    """17 MiB of text (fasta_cases.BIG_BYTES): more than 4096 chunks of 4096 bytes, more than 4096 runs — the chunk counts, the run
    bits and the runs' segment counts all take the second level of exclusive_scan, and a header lies across the first chunk of
    that level."""
    text, k = fa.big_case()
    want = fa.ref_pack_fasta(text, k)
    assert len(want[1]) - 1 > fa.SCAN_ITEMS
    t0 = time.perf_counter()
    rc, got, route = device_pack(lib, text, None, k)
    print("device packer on %d bytes: %.2f s" % (len(text), time.perf_counter() - t0))
    assert rc == 0 and route == "device", (rc, route)
    assert_same_batch(got, want, "the 17 MiB text")
