"""FASTQ texts at the edges of the device parser (csrc/fastq_gpu.hip) and a plain reference packer for them.

ref_pack() restates SPEC S1 / S2 and DESIGN "Data layout" in Python/numpy, independent of csrc/fastq.cpp; cases() is a
catalogue of seeded texts, each built to reach one branch of k_read_wave / k_merge_edges / exclusive_scan / gpu_join_spans
with a known shape.  tests/test_fastq_cases.py holds the host packer and the oracle against it, tests/test_gpu_fastq_pack.py
the device parser, word for word."""
import collections

import numpy as np

RUN_MAX = 16384          # a valid run of more than RUN_MAX + k - 1 bases is split by the host packer (csrc/fastq.cpp)
BIG = "scan_levels_3_4096x4096_plus_3_records_k15"

Case = collections.namedtuple("Case", "f1 f2 k min_qual route")


class RunTooLong(Exception):
    """a valid run of more than RUN_MAX + k - 1 bases: the split rule is the host packer's, not the reference's"""


_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i
    _CODE[_c + 32] = _i                                         # lower case


def _records(text):
    """SPEC S1: the (sequence, quality) lines of a text, or None for a parse error"""
    lines = text.split(b"\n")
    if lines[-1] == b"":
        lines.pop()                                             # the text ends with its newline
        terminated = len(lines)
    else:
        terminated = len(lines) - 1                             # the last line has none
    out, i = [], 0
    while i < len(lines):
        if i < terminated and lines[i] in (b"", b"\r"):         # a blank line in front of a record
            i += 1
            continue
        if i + 4 > len(lines):
            return None                                         # truncated record
        four = [ln[:-1] if ln.endswith(b"\r") else ln for ln in lines[i:i + 4]]
        if not four[0].startswith(b"@") or not four[2].startswith(b"+") or len(four[1]) != len(four[3]):
            return None
        out.append((four[1], four[3]))
        i += 4
    return out


def pack_codes(codes):
    """base i in bits 2 * (i % 16) of word i / 16; (n >> 4) + 2 words, zero behind the last base"""
    n = len(codes)
    nw = (n >> 4) + 2
    c = np.zeros(nw * 16, dtype=np.uint32)
    c[:n] = codes
    return (c.reshape(nw, 16) << (2 * np.arange(16, dtype=np.uint32))).sum(axis=1, dtype=np.uint64).astype(np.uint32)


def ref_pack(text, k, min_qual, text2=None, run_max=RUN_MAX):
    """(words u32[(n_bases >> 4) + 2], seg_off u32[n_seg + 1], n_reads, n_input_bases) of one text — or of two, file 1 and then
    file 2 into one stream — or None where SPEC S1 calls for a parse error.  RunTooLong for a run beyond the limit."""
    recs = []
    for t in (text,) if text2 is None else (text, text2):
        r = _records(bytes(t))
        if r is None:
            return None
        recs += r
    kept, seg_off, n_input = [], [0], 0
    for seq, qual in recs:
        n_input += len(seq)
        if len(seq) < k:
            continue
        s = np.frombuffer(seq, dtype=np.uint8)
        q = np.frombuffer(qual, dtype=np.uint8).astype(np.int64)
        code = _CODE[s]
        valid = (code < 4) & (q - 33 >= min_qual)               # SPEC S2 (Q1)
        edge = np.flatnonzero(np.diff(np.concatenate(([0], valid.view(np.int8), [0]))))
        for a, b in zip(edge[0::2], edge[1::2]):                # the maximal runs of valid bases
            if b - a > run_max + k - 1:
                raise RunTooLong(int(b - a))
            if b - a >= k:
                kept.append(code[a:b])
                seg_off.append(seg_off[-1] + int(b - a))
    codes = np.concatenate(kept) if kept else np.zeros(0, dtype=np.uint8)
    return pack_codes(codes), np.asarray(seg_off, dtype=np.uint32), len(recs), n_input


def unpack_segments(words, seg_off):
    """the segment strings of a packed batch, in order"""
    codes = ((np.asarray(words, dtype=np.uint32)[:, None] >> (2 * np.arange(16, dtype=np.uint32))) & 3).astype(np.uint8).reshape(-1)
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[codes].tobytes()
    return [text[int(a):int(b)] for a, b in zip(seg_off, seg_off[1:])]


# ---- the texts ---------------------------------------------------------------------------------------------------------------
def seq_of(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()


def rec(seq, qual=None, name=b"r", nl=b"\n"):
    return b"@" + name + nl + seq + nl + b"+" + nl + (b"I" * len(seq) if qual is None else qual) + nl


def with_bytes(seq, at, byte):
    b = bytearray(seq)
    for i in at:
        b[i] = byte
    return bytes(b)


PIECE_LENGTHS = (63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 258, 320)
PIECE_INVALID = (0, 63, 64, 65, 127, 128, 192)
PHASE_LENGTHS = (15, 16, 17, 31, 32, 33, 47, 48, 49)


def piece_records(rng, k, nl=b"\n"):
    """every length of PIECE_LENGTHS all valid and with one invalid base at each place of PIECE_INVALID and at L - 1; short
    records of k + 1 .. k + 5 bases in between move the stream offset off the multiples of 16"""
    out, i = [], 0
    for L in PIECE_LENGTHS:
        for at in (None,) + tuple(p for p in PIECE_INVALID if p < L - 1) + (L - 1,):
            s = seq_of(rng, L)
            out.append(rec(s if at is None else with_bytes(s, [at], ord("N")), nl=nl))
            if i % 3 == 0:
                out.append(rec(seq_of(rng, k + 1 + (i // 3) % 5), nl=nl))
            i += 1
    return out


def runs_record(rng, lengths, sep_seq, sep_qual):
    """valid runs of these lengths, one separator base between two of them"""
    seq, qual = b"", b""
    for j, n in enumerate(lengths):
        if j:
            seq += sep_seq if sep_seq else seq_of(rng, 1)
            qual += sep_qual
        seq += seq_of(rng, n)
        qual += b"I" * n
    return rec(seq, qual)


def long_run_cases(out):
    k = 31
    for n, route in ((RUN_MAX, "text_slice"), (RUN_MAX + 1, "host"), (RUN_MAX + k - 1, "host"), (RUN_MAX + k, "host"), (40000, "host")):
        rng = np.random.default_rng(9000 + n)
        short = [rec(seq_of(rng, 40 + j)) for j in range(3)]
        out["run_limit_%d_one_record_k31" % n] = Case(short[0] + rec(seq_of(rng, n)) + short[1], None, k, 20, route)
        # the same run inside a record of 50 000 bases: an 'N' on either side, and one every 3000 bases in the rest
        s = bytearray(seq_of(rng, 50000))
        a = 2999
        for p in list(range(0, a, 1500)) + [a] + list(range(a + 1 + n, 50000, 3000)):
            s[p] = ord("N")
        assert bytes(s[a + 1:a + 1 + n]).count(b"N") == 0 and s[a + 1 + n] == ord("N")
        out["run_limit_%d_inside_50000_k31" % n] = Case(short[0] + rec(bytes(s)) + short[2], None, k, 20, route)


def big_case():
    """4096 * 4096 + 3 records: the third level of exclusive_scan.  Minimal records, and six real ones of 40 bases at the
    indices 0, 4095, 4096, 4096^2 - 1, 4096^2 and the last.  Returns (text, the six records as one text, n_reads, n_input_bases)."""
    rng = np.random.default_rng(4096)
    n = 4096 * 4096 + 3
    real = [rec(seq_of(rng, 40)) for _ in range(6)]
    at = [0, 4095, 4096, 4096 * 4096 - 1, 4096 * 4096, n - 1]
    m = b"@\nA\n+\nI\n"
    parts, prev = [], -1
    for i, r in zip(at, real):
        parts.append(m * (i - prev - 1))
        parts.append(r)
        prev = i
    return b"".join(parts), b"".join(real), n, (n - 6) + 6 * 40


def fuzz_case(seed):
    rng = np.random.default_rng(seed)
    k = int(rng.choice([15, 21, 31, 63]))
    min_qual = int(rng.choice([0, 20, 33, 93]))
    nl_kind = int(rng.integers(0, 3))                           # \n, \r\n, mixed
    bad_base, bad_qual = float(rng.choice([0.0, 0.005, 0.03])), float(rng.choice([0.0, 0.005, 0.03]))
    lengths = [0, 1, 14, 15, 16, 17, 31, 33, 47, 63, 64, 65, 100, 127, 128, 150, 192, 255, 256, 257, 258, 320, 700, 1500]
    n_rec = int(rng.integers(1, 61))
    lines = []
    for i in range(n_rec):
        L = int(rng.choice(lengths))
        if i == n_rec - 1 and L == 0:
            L = 1                                               # (an empty last record is a case of its own)
        s = bytearray(seq_of(rng, L))
        q = bytearray([33 + min_qual] * L) if rng.random() < 0.5 else bytearray(rng.integers(33 + min_qual, 127, L).astype(np.uint8).tobytes())
        for p in np.flatnonzero(rng.random(L) < bad_base):
            s[p] = int(rng.choice(list(b"NnRY.-*")))
        if min_qual:
            for p in np.flatnonzero(rng.random(L) < bad_qual):
                q[p] = 33 + min_qual - 1
        if rng.random() < 0.2:
            s = bytearray(bytes(s).lower())
        lines += [b"@f%d" % i, bytes(s), b"+" if rng.random() < 0.7 else b"+f%d" % i, bytes(q)]
    ends = [b"\r\n" if nl_kind == 1 or (nl_kind == 2 and rng.random() < 0.5) else b"\n" for _ in lines]
    tail = int(rng.integers(0, 4))
    if tail == 1:
        ends[-1] = b""                                          # the last line without its newline
    elif tail == 2:
        ends[-1] += b"\n"                                       # a blank line behind the text
    return Case(b"".join(a + b for a, b in zip(lines, ends)), None, k, min_qual, "text_slice")


_CASES = None


def cases():
    """{name: Case(f1, f2, k, min_qual, route)}; route is "text_slice" (the device parser) or "host" (the fallback).  The
    134 MB text is not in here: big_case() builds it."""
    global _CASES
    if _CASES is not None:
        return _CASES
    out = {}
    # ---- word phases: with 17 behind every round of PHASE_LENGTHS (288 = 18 words) the rounds begin at every phase in turn
    rng = np.random.default_rng(1)
    out["word_phases_k15"] = Case(b"".join(rec(seq_of(rng, n)) for _ in range(32) for n in PHASE_LENGTHS + (17,)), None, 15, 20, "text_slice")
    # ---- several runs per record
    for name, sep_seq, sep_qual in (("N", b"N", b"I"), ("low_quality", b"", bytes([33 + 20 - 1]))):
        rng = np.random.default_rng(2)
        recs = []
        for i in range(150):
            lengths = [int(x) for x in rng.integers(15, 21, int(rng.integers(2, 7)))]
            for j in range(1, len(lengths) - 1):
                if rng.random() < 0.3:
                    lengths[j] = 14                             # dropped, between kept ones
            recs.append(runs_record(rng, lengths, sep_seq, sep_qual))
        out["several_runs_split_by_%s_k15" % name] = Case(b"".join(recs), None, 15, 20, "text_slice")
    # ---- the 64-base pieces and the small/long switch at a raw length of 256
    for k in (15, 31):
        out["piece_boundaries_k%d" % k] = Case(b"".join(piece_records(np.random.default_rng(3), k)), None, k, 20, "text_slice")
        out["piece_boundaries_crlf_k%d" % k] = Case(b"".join(piece_records(np.random.default_rng(3), k, b"\r\n")), None, k, 20, "text_slice")
    # ---- line ends
    rng = np.random.default_rng(4)
    recs = piece_records(rng, 15)[:60]
    plain = b"".join(recs)
    some = b"".join(ln + (b"\r\n" if rng.random() < 0.5 else b"\n") for ln in plain.split(b"\n")[:-1])
    out["crlf_on_some_lines_k15"] = Case(some, None, 15, 20, "text_slice")
    out["last_line_without_newline_k15"] = Case(plain[:-1], None, 15, 20, "text_slice")
    out["last_line_ends_in_cr_without_newline_k15"] = Case(plain.replace(b"\n", b"\r\n")[:-1], None, 15, 20, "text_slice")
    out["trailing_blank_lines_k15"] = Case(plain + b"\n\r\n\n", None, 15, 20, "text_slice")
    # ---- short records (edge[]) and long ones (atomicOr) in the same words
    for name, min_qual, low in (("", 0, 0.0), ("_min_qual_20", 20, 0.03)):
        rng = np.random.default_rng(5)
        recs = []
        for L in (300, 5000, 4097, 1023, 2500, 301, 3333, 800, 4999, 1600, 640, 2222, 3100, 901, 4500, 1234, 2750, 3999):
            s = bytearray(seq_of(rng, L))
            for p in rng.integers(0, L, max(1, L // 200)):
                s[p] = ord("N")
            q = bytearray(b"I" * L)
            for p in np.flatnonzero(rng.random(L) < low):
                q[p] = 33 + 19
            recs += [rec(bytes(s), bytes(q)), rec(seq_of(rng, int(rng.integers(15, 41))))]
        out["short_and_long_records_share_words%s_k15" % name] = Case(b"".join(recs), None, 15, min_qual, "text_slice")
    # ---- validity
    for mq in (0, 20, 33, 93):
        rng = np.random.default_rng(60 + mq)
        quals = [33 + mq, 33 + mq, 33 + mq, 0x7E, 0x7F, 0x80, 0xFF] + ([33 + mq - 1] if mq else [])
        recs = []
        for i in range(120):
            L = int(rng.integers(40, 90))
            s = bytearray(seq_of(rng, L))
            if i % 4 == 1:
                s = bytearray(bytes(s).lower())
            for p in np.flatnonzero(rng.random(L) < 0.04):
                s[p] = int(rng.choice(list(b"NnRYKMSWBDHVryu.-*")))
            q = bytes(int(rng.choice(quals)) if rng.random() < 0.12 else 33 + mq for _ in range(L))
            recs.append(rec(bytes(s), q))
        out["validity_min_qual_%d_k15" % mq] = Case(b"".join(recs), None, 15, mq, "text_slice")
    # quality bytes below '!' (0x21).  SPEC S2 (Q1) gives quality - 33 >= min_qual, so at min_qual = 0 such a base is not valid
    # (-1 >= 0 is false) although the same paragraph says that 0 "accepts every quality byte".  The oracle's verdict: NOT
    # VALID — oracle/shk_oracle.c compares (int)byte - 33 < (int)min_qual as signed numbers.  The runs end at these bases.
    rng = np.random.default_rng(7)
    recs = []
    for i in range(60):
        L = int(rng.integers(40, 90))
        q = bytearray(b"I" * L)
        for p in rng.integers(0, L, 2):
            q[p] = int(rng.choice([0x20, 0x09, 0x01, 0x1F, 0x00, 0x0B]))
        recs.append(rec(seq_of(rng, L), bytes(q)))
    out["quality_bytes_below_0x21_min_qual_0_k15"] = Case(b"".join(recs), None, 15, 0, "text_slice")
    # ---- nothing kept
    rng = np.random.default_rng(8)
    recs = [runs_record(rng, [int(x) for x in rng.integers(1, 31, int(rng.integers(1, 5)))], b"N", b"I") for _ in range(100)]
    out["nothing_kept_k31"] = Case(b"".join(recs), None, 31, 20, "text_slice")
    # ---- empty records
    rng = np.random.default_rng(9)
    some = [rec(seq_of(rng, int(rng.integers(15, 70)))) for _ in range(12)]
    empty = rec(b"")
    out["empty_records_in_the_middle_k15"] = Case(some[0] + empty + some[1] + some[2] + empty + empty + some[3], None, 15, 20, "text_slice")
    # An empty record as the LAST one.  The oracle's verdicts (oracle/shk_oracle.c: lines 0..2 of a record need their newline,
    # line 3 needs to begin inside the text):
    #   with its final '\n' ("...@r\n\n+\n\n"):  TAKEN, one read of no bases.  Without its trailing blank lines the text no longer
    #       has 4 lines per record, so the device parser hands it over: the host parser on the whole slice is the route.
    #   without it ("...@r\n\n+\n"):  REFUSED, "truncated FASTQ record" — the quality line does not begin inside the text.
    out["empty_last_record_with_final_newline_k15"] = Case(some[4] + some[5] + empty, None, 15, 20, "host")
    out["empty_last_record_alone_with_final_newline_k15"] = Case(b"@a\n\n+\n\n", None, 15, 20, "host")
    out["empty_last_record_without_final_newline_k15"] = Case(some[4] + some[5] + empty[:-1], None, 15, 20, None)
    # ---- the run limit
    long_run_cases(out)
    # ---- scan levels: more than 4096 records, 0 .. 3 segments each
    for n in (4097, 8193):
        rng = np.random.default_rng(n)
        recs = [runs_record(rng, [int(x) for x in rng.integers(15, 18, i % 4)] if i % 4 else [10], b"N", b"I") for i in range(n)]
        out["scan_levels_2_%d_records_k15" % n] = Case(b"".join(recs), None, 15, 20, "text_slice")
    # ---- two files
    rng = np.random.default_rng(11)
    a = b"".join(rec(seq_of(rng, int(rng.integers(50, 200)))) for _ in range(40))
    b = b"".join(rec(seq_of(rng, int(rng.integers(50, 200)))) for _ in range(30))
    nothing = b"".join(rec(seq_of(rng, 20)) for _ in range(10))
    out["two_files_first_without_last_newline_k31"] = Case(a[:-1], b, 31, 20, "text_slice")
    out["two_files_first_crlf_k31"] = Case(a.replace(b"\n", b"\r\n"), b, 31, 20, "text_slice")
    out["two_files_first_crlf_without_last_newline_k31"] = Case(a.replace(b"\n", b"\r\n")[:-2], b, 31, 20, "text_slice")
    out["two_files_second_empty_k31"] = Case(a, b"", 31, 20, "text_slice")
    out["two_files_first_keeps_nothing_k31"] = Case(nothing, b, 31, 20, "text_slice")
    out["two_files_k51"] = Case(a, b[:-1], 51, 20, "text_slice")
    # ---- fuzz
    for i in range(200):
        out["fuzz_%03d" % i] = fuzz_case(31000 + i)
    _CASES = out
    return out


_REF = {}


def reference(name):
    """ref_pack of a catalogue case, computed once"""
    if name not in _REF:
        c = cases()[name]
        try:
            _REF[name] = ref_pack(c.f1, c.k, c.min_qual, c.f2)
        except RunTooLong:
            _REF[name] = RunTooLong
    return _REF[name]
