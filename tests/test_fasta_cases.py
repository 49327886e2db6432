"""The host FASTA packer (shk_pack_fasta) against the reference packer of tests/fasta_cases.py and against the pin of SPEC S1a —
shk_pack_fastq on the FASTQ twin — on every text of the catalogue: the counts, seg_off and every word.  No GPU."""
import ctypes as C
import gzip
import os
import re

import numpy as np
import pytest

import fasta_cases as fa
import fastq_cases as fc
from sparrowhawk_amd import _lib
from test_fastq_cases import assert_same_batch, host_pack, windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = fa.cases()
REGULAR = [n for n, c in CASES.items() if c.ok]
REFUSED = [n for n, c in CASES.items() if not c.ok]
LONG_RUNS = [n for n in CASES if n.startswith("piece_rule_")]
SHK_E_PARSE = -3


def host_pack_fasta(lib, text, k):
    """(rc, (words, seg_off, n_reads, n_input_bases) or None, message)"""
    out, err = _lib.ShkPacked(), C.c_char_p()
    rc = lib.shk_pack_fasta(text, len(text), k, C.byref(out), C.byref(err))
    if rc != 0:
        return rc, None, (err.value or b"").decode()
    try:
        words = np.ctypeslib.as_array(out.bases, shape=((out.n_bases >> 4) + 2,)).copy()
        seg = np.ctypeslib.as_array(out.seg_off, shape=(out.n_seg + 1,)).copy()
        assert int(seg[-1]) == out.n_bases
        return 0, (words, seg, int(out.n_reads), int(out.n_input_bases)), ""
    finally:
        lib.shk_packed_free(C.byref(out))


def pooled(c):
    """a pair as one text: file 1, then file 2, a newline supplied where file 1 lacks its last one"""
    if c.f2 is None:
        return c.f1
    return c.f1 + (b"\n" if c.f1 and not c.f1.endswith(b"\n") else b"") + c.f2


@pytest.mark.parametrize("name", REGULAR)
def test_host_packer_equals_the_reference_and_the_fastq_twin(lib, name):
    c = CASES[name]
    want = fa.reference(name)
    assert want is not None, name
    rc, got, msg = host_pack_fasta(lib, pooled(c), c.k)
    assert rc == 0, (name, rc, msg)
    assert_same_batch(got, want, name)
    assert_same_batch(got, host_pack(lib, fa.twin_of(c), c.k, 0), name + ": the FASTQ twin")


@pytest.mark.parametrize("name", REFUSED)
def test_refusals_are_parse_errors_that_say_fasta(lib, name):
    c = CASES[name]
    assert fa.reference(name) is None
    if c.f2 is None:
        rc, got, msg = host_pack_fasta(lib, c.f1, c.k)
    else:                                                       # (two files are two calls of the packer: the damage is in file 2)
        assert host_pack_fasta(lib, c.f1, c.k)[0] == 0
        rc, got, msg = host_pack_fasta(lib, c.f2, c.k)
    assert rc == SHK_E_PARSE and "FASTA" in msg, (name, rc, msg)


@pytest.mark.parametrize("name", LONG_RUNS)
def test_the_pieces_of_the_reference_hold_every_kmer_of_the_unsplit_runs_once(name):
    c = CASES[name]
    split, whole = fa.reference(name), fa.ref_pack_fasta(c.f1, c.k, c.f2, split=False)
    n = int(re.search(r"run_of_(\d+)_", name).group(1))
    assert int(np.diff(whole[1].astype(np.int64)).max()) == n
    lengths = np.diff(split[1].astype(np.int64))
    assert int(lengths.max()) <= fa.RUN_MAX + c.k - 1 and int(lengths.min()) >= c.k
    n_pieces = 1 if n <= fa.RUN_MAX + c.k - 1 else -(-(n - c.k + 1) // fa.RUN_MAX)
    assert len(lengths) == len(whole[1]) - 1 + n_pieces - 1
    assert windows(split[0], split[1], c.k) == windows(whole[0], whole[1], c.k)


def test_the_piece_rule_at_its_edges():
    k = 31
    assert fa.pieces_of(fa.RUN_MAX + k - 1, k) == [(0, fa.RUN_MAX + k - 1)]
    assert fa.pieces_of(fa.RUN_MAX + k, k) == [(0, fa.RUN_MAX + k - 1), (fa.RUN_MAX, fa.RUN_MAX + k)]      # a last piece of exactly k bases
    assert [b - a for a, b in fa.pieces_of(2 * fa.RUN_MAX + k - 1, k)] == [fa.RUN_MAX + k - 1] * 2
    assert [b - a for a, b in fa.pieces_of(2 * fa.RUN_MAX + k, k)] == [fa.RUN_MAX + k - 1] * 2 + [k]


def test_gzip_and_two_member_gzip_give_the_plain_texts_batch(lib):
    for name in ("line_width_60_k15", "header_of_40000_bytes_k15", "piece_rule_run_of_100000_k31"):
        c = CASES[name]
        want = fa.reference(name)
        cut = c.f1.index(b"\n>", len(c.f1) // 2) + 1
        for blob in (gzip.compress(c.f1, 6), gzip.compress(c.f1[:cut], 6) + gzip.compress(c.f1[cut:], 1)):
            rc, got, msg = host_pack_fasta(lib, blob, c.k)
            assert rc == 0, (name, rc, msg)
            assert_same_batch(got, want, name)


def test_the_catalogue_has_the_shapes_it_names():
    assert len(REGULAR) >= 230 and len(REFUSED) == 5 and sum(n.startswith("fuzz_") for n in CASES) == 200
    # the constants the chunk-edge cases and the large text are built from are the packer's
    src = open(os.path.join(ROOT, "sparrowhawk_amd", "csrc", "fasta_gpu.h")).read()
    assert int(re.search(r"FASTA_GPU_CHUNK = (\d+);", src).group(1)) == fa.CHUNK
    src = open(os.path.join(ROOT, "sparrowhawk_amd", "csrc", "scan_gpu.h")).read()
    assert int(re.search(r"SCAN_ITEMS = (\d+);", src).group(1)) == fa.SCAN_ITEMS
    assert fa.BIG_BYTES > fa.SCAN_ITEMS * fa.CHUNK and fa.BIG_BYTES < 100000000
    t = CASES["chunk_edge_newline_then_header_k15"].f1
    assert t[fa.CHUNK - 1:fa.CHUNK + 1] == b"\n>"
    assert CASES["chunk_edge_crlf_across_k15"].f1[fa.CHUNK - 1:fa.CHUNK + 1] == b"\r\n"
    t = CASES["chunk_edge_header_covers_a_whole_chunk_k15"].f1
    assert b"\n" not in t[fa.CHUNK - 90:3 * fa.CHUNK]
    assert max(len(ln) for ln in CASES["header_of_40000_bytes_k15"].f1.split(b"\n") if ln.startswith(b">")) == 40001      # ('>' and 40 000 bytes)
    w, seg, n_reads, n_in = fa.reference("run_across_three_chunks_k15")
    assert int(np.diff(seg.astype(np.int64)).max()) == 2 * fa.CHUNK + 600
    # word phases: 15, 16 and 17 bases at every phase
    w, seg, _, _ = fa.reference("word_phases_k15")
    seg = seg.astype(np.int64)
    assert {(int(a) % 16, int(n)) for a, n in zip(seg[:-1], np.diff(seg)) if n in (15, 16, 17)} == {(p, n) for p in range(16) for n in (15, 16, 17)}
    # runs of k - 1 on either side of a header: nothing of them is kept
    for k in (15, 31):
        w, seg, n_reads, n_in = fa.reference("run_of_k_minus_1_on_either_side_of_a_header_k%d" % k)
        assert n_reads == 2 and np.diff(seg.astype(np.int64)).tolist() == [100, 100]
    # every kind of invalid byte ends a run; lower case does not
    w, seg, n_reads, n_in = fa.reference("every_kind_of_invalid_byte_k15")
    assert np.diff(seg.astype(np.int64))[:len(fa.INVALID) + 1].tolist() == [20] * len(fa.INVALID) + [40]
    # empty records count, and keep nothing
    assert fa.reference("empty_records_k15")[2] == 7 and fa.reference("gt_alone_k15")[2] == 3
    # no records at all: no error, an empty batch
    for name in ("empty_text_k15", "only_newlines_k15"):
        w, seg, n_reads, n_in = fa.reference(name)
        assert (len(seg), n_reads, n_in) == (1, 0, 0) and not w.any()
    # the fuzz texts reach what they mix
    fz = [CASES[n].f1 for n in CASES if n.startswith("fuzz_")]
    assert sum(b"\r\n" in t for t in fz) > 50 and sum(t[-1:] not in (b"\n", b"") for t in fz) > 20 and sum(b"\n\n" in t for t in fz) > 50
    assert all(len(pooled(c)) <= 260000 for c in CASES.values())


def test_the_large_text_is_built_as_described():
    text, k = fa.big_case()
    assert fa.BIG_BYTES <= len(text) < fa.BIG_BYTES + 70000     # (the last record's line ends and header come on top)
    edge = fa.SCAN_ITEMS * fa.CHUNK
    assert text[edge - 100:edge + 100] == b"h" * 200            # the long header lies across the first chunk of the second level
    assert text.count(b">") == text.count(b"\n>") + 1
