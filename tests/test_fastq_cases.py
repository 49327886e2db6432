"""The host packer (shk_pack_fastq) and the oracle's reader against the reference packer of tests/fastq_cases.py, on every
text of its catalogue: the counts, seg_off and every word of the packed stream.  No GPU."""
import collections
import ctypes as C

import numpy as np
import pytest

import fastq_cases as fc
from sparrowhawk_amd import _lib
from util import run_oracle

CASES = fc.cases()
# the three cases whose expected result is the oracle's verdict (written next to each in fastq_cases.py)
PINNED = {
    "quality_bytes_below_0x21_min_qual_0_k15": "taken; a base under a quality byte below 0x21 is not valid, also at min_qual 0",
    "empty_last_record_with_final_newline_k15": "taken: one more read, of no bases",
    "empty_last_record_without_final_newline_k15": "refused: truncated FASTQ record",
}


def joined(c):
    """a pair as the product packs it: file 1, then file 2, a newline supplied where file 1 lacks its last one"""
    if c.f2 is None:
        return c.f1
    return c.f1 + (b"\n" if c.f1 and not c.f1.endswith(b"\n") else b"") + c.f2


def host_pack(lib, text, k, min_qual):
    """(words, seg_off, n_reads, n_input_bases) of shk_pack_fastq, or None for SHK_E_PARSE"""
    out, err = _lib.ShkPacked(), C.c_char_p()
    rc = lib.shk_pack_fastq(text, len(text), k, min_qual, C.byref(out), C.byref(err))
    if rc == -3:
        return None
    assert rc == 0, (rc, err.value)
    try:
        words = np.ctypeslib.as_array(out.bases, shape=((out.n_bases >> 4) + 2,)).copy()
        seg = np.ctypeslib.as_array(out.seg_off, shape=(out.n_seg + 1,)).copy()
        assert int(seg[-1]) == out.n_bases
        return words, seg, int(out.n_reads), int(out.n_input_bases)
    finally:
        lib.shk_packed_free(C.byref(out))


def first_difference(got, want):
    """the first segment in which two packed batches differ, decoded"""
    a, b = fc.unpack_segments(got[0], got[1]), fc.unpack_segments(want[0], want[1])
    for j, (x, y) in enumerate(zip(a, b)):
        if x != y or got[1][j] != want[1][j]:
            return "segment %d: got %r at %d, want %r at %d" % (j, x, got[1][j], y, want[1][j])
    return "%d segments, want %d" % (len(a), len(b))


def assert_same_batch(got, want, what):
    assert got is not None and want is not None, what
    assert (got[2], got[3]) == (want[2], want[3]), (what, "n_reads, n_input_bases", got[2:], want[2:])
    assert len(got[1]) == len(want[1]) and np.array_equal(got[1], want[1]), (what, first_difference(got, want))
    assert len(got[0]) == len(want[0]) == (int(want[1][-1]) >> 4) + 2, what
    assert np.array_equal(got[0], want[0]), (what, first_difference(got, want))


def windows(words, seg_off, k):
    """the k-mer windows of a packed batch, counted (as byte strings of codes)"""
    cnt = collections.Counter()
    for s in fc.unpack_segments(words, seg_off):
        if len(s) >= k:
            w = np.lib.stride_tricks.sliding_window_view(np.frombuffer(s, dtype=np.uint8), k)
            cnt.update(np.ascontiguousarray(w).view("V%d" % k).reshape(-1).tolist())
    return cnt


def canonical_counts(words, seg_off, k):
    """{canonical k-mer as key words: count} of a packed batch, by rolling both strands"""
    W, mask, top = (2 * k + 63) // 64, (1 << (2 * k)) - 1, 2 * (k - 1)
    cnt = {}
    for s in fc.unpack_segments(words, seg_off):
        fw = rv = 0
        for i, ch in enumerate(s):
            c = b"ACGT".index(ch)
            fw = ((fw << 2) | c) & mask
            rv = (rv >> 2) | ((3 - c) << top)
            if i >= k - 1:
                v = min(fw, rv)
                key = tuple((v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(W))
                cnt[key] = cnt.get(key, 0) + 1
    return cnt


@pytest.mark.parametrize("name", list(CASES))
def test_host_packer_equals_the_reference_word_for_word(lib, name):
    c = CASES[name]
    want = fc.reference(name)
    got = host_pack(lib, joined(c), c.k, c.min_qual)
    if want is None:
        assert got is None and c.route is None, name
        return
    if want is fc.RunTooLong:
        # a run beyond the limit: the split rule is the host packer's own.  Every k-mer window of the unsplit runs lies in
        # exactly one of its segments, and none of them is longer than the limit.
        assert c.route == "host"
        whole = fc.ref_pack(c.f1, c.k, c.min_qual, c.f2, run_max=1 << 30)
        assert got is not None and (got[2], got[3]) == (whole[2], whole[3])
        assert int(np.diff(got[1].astype(np.int64)).max()) <= fc.RUN_MAX + c.k - 1
        assert windows(got[0], got[1], c.k) == windows(whole[0], whole[1], c.k)
        return
    assert c.route in ("text_slice", "host")
    assert_same_batch(got, want, name)


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if len(joined(c)) < 20000])
def test_reference_equals_the_oracle_in_canonical_kmer_counts(name):
    """keeps the reference independent of the product's parser: the oracle reads the same text"""
    c = CASES[name]
    want = fc.reference(name)
    try:
        o = run_oracle([c.f1] + ([c.f2] if c.f2 is not None else []), k=c.k, min_count=0, min_qual=c.min_qual)
    except ValueError as e:
        assert want is None, (name, "the oracle refuses, the reference takes", str(e))
        return
    assert want is not None and want is not fc.RunTooLong, (name, "the oracle takes, the reference refuses")
    assert want[2] == o.n_reads and want[3] == o.n_bases
    assert canonical_counts(want[0], want[1], c.k) == {tuple(int(x) for x in key): int(n) for key, n in zip(*o.distinct())}


def test_the_pinned_cases_are_below_the_oracle_limit_and_have_its_verdict():
    for name, verdict in PINNED.items():
        c = CASES[name]
        assert len(joined(c)) < 20000                          # (so the test above holds the oracle against each)
        assert (fc.reference(name) is None) == verdict.startswith("refused"), name
    w, seg, n_reads, n_in = fc.reference("empty_last_record_with_final_newline_k15")
    assert n_reads == 3 and len(seg) == 3
    # below 0x21: every record loses its two marked bases, so no run is the whole sequence
    w, seg, n_reads, n_in = fc.reference("quality_bytes_below_0x21_min_qual_0_k15")
    assert n_in - int(seg[-1]) >= n_reads and len(seg) - 1 > n_reads


def test_the_catalogue_has_the_shapes_it_names():
    # every word phase with every length of 15, 16, 17; a segment inside one word
    w, seg, _, _ = fc.reference("word_phases_k15")
    seg = seg.astype(np.int64)
    length = np.diff(seg)
    assert set(length.tolist()) == set(fc.PHASE_LENGTHS) and 300 <= len(length) <= 400
    seen = {(int(a) % 16, int(n)) for a, n in zip(seg[:-1], length) if n in (15, 16, 17)}
    assert seen == {(p, n) for p in range(16) for n in (15, 16, 17)}
    assert any(a >> 4 == (b - 1) >> 4 for a, b in zip(seg[:-1], seg[1:]))
    # several runs per record: more segments than records, and dropped runs of 14 between kept ones
    for name in ("several_runs_split_by_N_k15", "several_runs_split_by_low_quality_k15"):
        w, seg, n_reads, n_in = fc.reference(name)
        assert len(seg) - 1 > 2 * n_reads and n_in - int(seg[-1]) > n_reads + 14 * 20
    # piece boundaries: stream offsets off the multiples of 16, raw lengths on both sides of the switch
    for k in (15, 31):
        w, seg, _, _ = fc.reference("piece_boundaries_k%d" % k)
        assert len({int(a) % 16 for a in seg}) == 16
    crlf = CASES["piece_boundaries_crlf_k15"].f1.split(b"\n")
    assert {len(ln) for ln in crlf[1::4]} >= {256, 257, 258} and all(ln.endswith(b"\r") for ln in crlf[:-1])
    # short and long records meet inside words
    for name in ("short_and_long_records_share_words_k15", "short_and_long_records_share_words_min_qual_20_k15"):
        lens = [len(ln) for ln in CASES[name].f1.split(b"\n")[1::4]]
        assert min(lens) < 41 and max(lens) == 5000 and sum(300 <= n <= 5000 for n in lens) == 18
    # nothing kept
    w, seg, n_reads, n_in = fc.reference("nothing_kept_k31")
    assert len(seg) == 1 and not w.any() and n_reads == 100 and n_in > 1000
    # run limit: on either side of it
    for n, ref_takes in ((16384, True), (16385, True), (16384 + 30, True), (16384 + 31, False), (40000, False)):
        for shape in ("one_record", "inside_50000"):
            r = fc.reference("run_limit_%d_%s_k31" % (n, shape))
            assert (r is not fc.RunTooLong) == ref_takes
            if ref_takes:
                assert int(np.diff(r[1].astype(np.int64)).max()) == n
    # scan levels: the two scans differ
    for n in (4097, 8193):
        w, seg, n_reads, n_in = fc.reference("scan_levels_2_%d_records_k15" % n)
        assert n_reads == n and len(seg) - 1 == (n // 4) * 6 + sum(range(n % 4))
    # every text but the scan-level ones is small; routes
    for name, c in CASES.items():
        if not name.startswith("scan_levels"):
            assert len(joined(c)) <= 110000, name
        if c.route == "host":
            assert name.startswith("run_limit_") or name.startswith("empty_last_record_"), name
        if name.startswith("fuzz_"):
            assert c.route == "text_slice" and fc.reference(name) not in (None, fc.RunTooLong)
    assert sum(n.startswith("fuzz_") for n in CASES) == 200


def test_the_large_case_is_built_as_described():
    text, six, n_reads, n_in = fc.big_case()
    assert n_reads == 4096 * 4096 + 3 and text.count(b"\n") == 4 * n_reads and len(text) > 134000000
    recs = six.split(b"\n")
    for i, at in enumerate((0, 4095, 4096, 4096 * 4096 - 1, 4096 * 4096, n_reads - 1)):
        start = 8 * (at - i) + sum(len(r) + 1 for r in recs[:4 * i])
        assert text[start:].startswith(b"\n".join(recs[4 * i:4 * i + 4]) + b"\n"), at
    assert text.startswith(six[:40]) and text.endswith(six[-40:])
