"""FASTA texts at the edges of the two FASTA packers (csrc/fastq.cpp: pack_fasta, csrc/fasta_gpu.hip: gpu_pack_fasta) and a
plain reference packer for them.

ref_pack_fasta() restates SPEC S1a in Python/numpy, independent of both packers; fastq_twin() builds the FASTQ text that the
same paragraph pins a FASTA text to; cases() is a catalogue of seeded, named texts.  tests/test_fasta_cases.py holds the host
packer against both, tests/test_gpu_fasta_pack.py the device packer, word for word."""
import collections

import numpy as np

from fastq_cases import pack_codes, seq_of

RUN_MAX = 16384          # SPEC S1a: a valid run of more than RUN_MAX + k - 1 bases goes in as pieces of RUN_MAX k-mers
CHUNK = 4096             # csrc/fasta_gpu.h: FASTA_GPU_CHUNK, the text bytes of one workgroup (tests/test_fasta_cases.py reads it there)
SCAN_ITEMS = 4096        # csrc/scan_gpu.h: items per workgroup and level of exclusive_scan
BIG_BYTES = 17 * 1024 * 1024 + 12345      # more than SCAN_ITEMS chunks: the second level of the scan over the chunks' counts

Case = collections.namedtuple("Case", "f1 f2 k ok")      # ok False: SPEC S1a calls for a parse error

_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i
    _CODE[_c + 32] = _i                                         # lower case is valid


def records(text):
    """SPEC S1a: the joined sequences of the records of one text, or None for a parse error"""
    recs = None
    for ln in bytes(text).split(b"\n"):
        if ln.endswith(b"\r"):                                  # a '\r' in front of '\n', or as the last byte of the text
            ln = ln[:-1]
        if not ln:
            continue                                            # blank lines are ignored wherever they stand
        if ln.startswith(b">"):
            recs = [] if recs is None else recs
            recs.append([])                                     # the header itself is ignored
        elif recs is None:
            return None                                         # a non-blank line in front of the first header
        else:
            recs[-1].append(ln)
    return [b"".join(r) for r in (recs or [])]


def pieces_of(n, k, run_max=RUN_MAX):
    """the piece rule, stated here on its own: [a, b) inside a run of n >= k bases.  Up to run_max + k - 1 bases the run is one
    piece; beyond, piece i begins at i * run_max and holds run_max k-mers (run_max + k - 1 bases), the last one what is left
    (at least one k-mer: k bases), so that neighbours overlap by k - 1 bases and every k-mer lies in exactly one piece"""
    if n <= run_max + k - 1:
        return [(0, n)]
    return [(a, min(n, a + run_max + k - 1)) for a in range(0, n - k + 1, run_max)]


def ref_pack_fasta(text, k, text2=None, split=True):
    """(words u32[(n_bases >> 4) + 2], seg_off u32[n_seg + 1], n_reads, n_input_bases) of one text, or of two pooled, file 1
    first — or None where SPEC S1a calls for a parse error.  split=False: long runs stay whole (to pin the piece rule)."""
    recs = []
    for t in (text,) if text2 is None else (text, text2):
        r = records(t)
        if r is None:
            return None
        recs += r
    kept, seg_off, n_input = [], [0], 0
    for seq in recs:
        n_input += len(seq)
        if len(seq) < k:
            continue
        code = _CODE[np.frombuffer(seq, dtype=np.uint8)]
        valid = code < 4
        edge = np.flatnonzero(np.diff(np.concatenate(([0], valid.view(np.int8), [0]))))
        for a, b in zip(edge[0::2], edge[1::2]):                # the maximal runs of valid bases
            if b - a < k:
                continue
            for pa, pb in (pieces_of(int(b - a), k) if split else [(0, int(b - a))]):
                kept.append(code[a + pa:a + pb])
                seg_off.append(seg_off[-1] + pb - pa)
    codes = np.concatenate(kept) if kept else np.zeros(0, dtype=np.uint8)
    return pack_codes(codes), np.asarray(seg_off, dtype=np.uint32), len(recs), n_input


def fastq_twin(text):
    """the FASTQ text of the pin: every record with its joined sequence and a quality that passes"""
    return b"".join(b"@x\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for s in records(text))


# ---- the texts ---------------------------------------------------------------------------------------------------------------
def wrap(seq, width, nl=b"\n"):
    return b"".join(seq[i:i + width] + nl for i in range(0, len(seq), width))


def fa(name, seq, width=60, nl=b"\n"):
    return b">" + name + nl + wrap(seq, width, nl)


def with_invalid(rng, seq, rate, alphabet=b"N"):
    b = bytearray(seq)
    for p in np.flatnonzero(rng.random(len(b)) < rate):
        b[p] = int(rng.choice(list(alphabet)))
    return bytes(b)


def runs(rng, lengths, sep=b"N"):
    return sep.join(seq_of(rng, n) for n in lengths)


def padded_to(text, at):
    """text + a record of no bases whose header ends (with its newline) exactly at byte `at`"""
    room = at - len(text)
    assert room >= 2, room
    return text + b">" + b"p" * (room - 2) + b"\n"


INVALID = [b"N", b"n", b"R", b"y", b"K", b"*", b"-", b" ", b"\t", b"\r", b"\x80", b"\xff", b">", b"@", b"+"]
PIECE_RUNS = lambda k: (RUN_MAX + k - 2, RUN_MAX + k - 1, RUN_MAX + k, 2 * RUN_MAX + k - 1, 2 * RUN_MAX + k, 100000)      # noqa: E731


def fuzz_case(seed):
    rng = np.random.default_rng(seed)
    k = int(rng.choice([15, 21, 31, 63]))
    nl_kind = int(rng.integers(0, 3))                           # \n, \r\n, mixed
    rate = float(rng.choice([0.0, 0.003, 0.03]))
    lengths = [0, 1, 14, 15, 16, 17, 31, 33, 47, 63, 64, 65, 100, 127, 128, 150, 300, 700, 1500, 5000]
    lines = []
    for _ in range(int(rng.integers(0, 4))):
        lines.append(b"")                                       # blank lines in front of the first header
    for i in range(int(rng.integers(0, 13))):
        lines.append(b">" + rng.choice(np.frombuffer(b"abc >@+\t", dtype=np.uint8), int(rng.choice([0, 1, 5, 30]))).tobytes())
        s = with_invalid(rng, seq_of(rng, int(rng.choice(lengths))), rate, b"NnRY.-* \t@+>\x80\xfe")
        if rng.random() < 0.2:
            s = s.lower()
        width = int(rng.choice([1, 7, 15, 16, 17, 60, 70, 80, 1000000]))
        for j in range(0, len(s), width):
            ln = s[j:j + width]
            lines.append(b"N" + ln[1:] if ln.startswith(b">") else ln)      # (a '>' that begins a line would be a header)
            if rng.random() < 0.04:
                lines.append(b"")                               # a blank line inside the record
        if rng.random() < 0.2:
            lines.append(b"")
    ends = [b"\r\n" if nl_kind == 1 or (nl_kind == 2 and rng.random() < 0.5) else b"\n" for _ in lines]
    if lines and rng.random() < 0.3:
        ends[-1] = b""                                          # the last line without its newline
    return Case(b"".join(a + b for a, b in zip(lines, ends)), None, k, True)


def big_case():
    """BIG_BYTES of text (17 MiB: more than SCAN_ITEMS chunks of CHUNK bytes, so the chunk counts take the second level of
    exclusive_scan): five records on 60-character lines, an 'N' about every 3000 bases (more than SCAN_ITEMS runs), and a
    header of 5000 bytes across the chunk that begins the second level.  k = 31."""
    rng = np.random.default_rng(1717)
    parts, size = [], 0
    first = SCAN_ITEMS * CHUNK - 2000                           # a header from here reaches over chunk SCAN_ITEMS
    while size < BIG_BYTES:
        if not parts:
            n = (first // 61) * 60
        else:
            n = min(4000000, BIG_BYTES - size)
        s = bytearray(seq_of(rng, n))
        s[::3001] = b"N" * len(s[::3001])
        name = b"h" * 5000 if len(parts) == 1 else b"g%d" % len(parts)
        parts.append(fa(name, bytes(s)))
        size += len(parts[-1])
    return b"".join(parts), 31


_CASES = None


def cases():
    """{name: Case(f1, f2, k, ok)}.  The 17 MiB text is not in here: big_case() builds it."""
    global _CASES
    if _CASES is not None:
        return _CASES
    out = {}
    # ---- line widths: records of many lengths, a short last line in most
    for w in (1, 15, 16, 17, 60, 64, 70, 80):
        rng = np.random.default_rng(100 + w)
        recs = [fa(b"r%d" % i, with_invalid(rng, seq_of(rng, int(n)), 0.01), w) for i, n in enumerate(rng.integers(0, 400 if w > 1 else 90, 20))]
        recs.append(fa(b"full", seq_of(rng, 4 * w), w))         # (no short last line)
        out["line_width_%d_k15" % w] = Case(b"".join(recs), None, 15, True)
    # ---- line ends
    rng = np.random.default_rng(2)
    recs = [fa(b"r%d x" % i, with_invalid(rng, seq_of(rng, int(n)), 0.01), 60) for i, n in enumerate(rng.integers(20, 300, 12))]
    plain = b"".join(recs)
    out["no_final_newline_k15"] = Case(plain[:-1], None, 15, True)
    out["crlf_on_all_lines_k15"] = Case(plain.replace(b"\n", b"\r\n"), None, 15, True)
    out["crlf_without_final_newline_k15"] = Case(plain.replace(b"\n", b"\r\n")[:-1], None, 15, True)      # (ends in '\r')
    out["crlf_on_some_lines_k15"] = Case(b"".join(ln + (b"\r\n" if rng.random() < 0.5 else b"\n") for ln in plain.split(b"\n")[:-1]), None, 15, True)
    blank = []
    for r in recs:
        ls = r.split(b"\n")[:-1]
        blank.append(ls[0] + b"\n" + b"".join(ln + (b"\n\n" if j % 2 else b"\n\r\n\n") for j, ln in enumerate(ls[1:])))
    out["blank_lines_inside_records_k15"] = Case(b"".join(blank), None, 15, True)
    out["blank_lines_between_records_k15"] = Case(b"\n\r\n" + b"\n\n".join(recs) + b"\n\r\n\n", None, 15, True)
    # ---- run lengths around k; every 2-bit word phase
    for k in (15, 31):
        rng = np.random.default_rng(30 + k)
        lengths = [int(x) for x in rng.choice([k - 1, k, k + 1], 90)]
        out["runs_of_k_minus_1_k_k_plus_1_k%d" % k] = Case(b"".join(fa(b"r", runs(rng, lengths[i:i + 9]), 17) for i in range(0, 90, 9)), None, k, True)
    rng = np.random.default_rng(4)
    out["word_phases_k15"] = Case(b"".join(fa(b"p", seq_of(rng, n), 7) for _ in range(32) for n in (15, 16, 17, 31, 32, 33, 47, 48, 49, 17)), None, 15, True)
    # ---- invalid bytes at the ends of lines; a run that ends exactly at a line end
    rng = np.random.default_rng(5)
    lines = []
    for i in range(40):
        ln = bytearray(seq_of(rng, 60))
        if i % 4 == 0: ln[0] = ord("N")
        if i % 4 == 1: ln[-1] = ord("N")
        if i % 4 == 2: ln[0] = ln[-1] = ord("N")
        lines.append(bytes(ln))
    out["invalid_first_and_last_byte_of_lines_k15"] = Case(b">e\n" + b"\n".join(lines) + b"\n", None, 15, True)
    out["run_ends_at_a_line_end_k15"] = Case(b">e\n" + seq_of(rng, 60) + b"\nN" + seq_of(rng, 59) + b"\n" + seq_of(rng, 60) + b"\n>f\n" + seq_of(rng, 60) + b"\n", None, 15, True)
    # ---- every kind of invalid byte, each between two runs of 20 (and lower case, which is valid)
    rng = np.random.default_rng(6)
    seq = b"".join(seq_of(rng, 20) + x for x in INVALID) + seq_of(rng, 20).lower() + seq_of(rng, 20)
    out["every_kind_of_invalid_byte_k15"] = Case(fa(b"kinds", seq, 1000) + fa(b"wrapped", seq, 23).replace(b"\n>", b"\nN"), None, 15, True)
    # ---- headers
    for k in (15, 31):
        rng = np.random.default_rng(70 + k)
        out["run_of_k_minus_1_on_either_side_of_a_header_k%d" % k] = Case(
            fa(b"A", seq_of(rng, 100) + b"N" + seq_of(rng, k - 1), 60) + fa(b"B", seq_of(rng, k - 1) + b"N" + seq_of(rng, 100), 60), None, k, True)
    rng = np.random.default_rng(8)
    a, b = fa(b"a", seq_of(rng, 100)), fa(b"b", seq_of(rng, 130))
    out["empty_records_k15"] = Case(a + b">empty\n" + b + b">e2\n>e3\n\n>e4\r\n" + a, None, 15, True)
    out["header_as_last_line_k15"] = Case(a + b">last\n", None, 15, True)
    out["header_as_last_line_without_newline_k15"] = Case(a + b">last", None, 15, True)
    out["gt_alone_k15"] = Case(b">\n" + wrap(seq_of(rng, 100), 60) + b">\n>", None, 15, True)
    out["header_of_40000_bytes_k15"] = Case(a + b">" + b"h>@+ACGT\t\r" * 4000 + b"\n" + wrap(seq_of(rng, 200), 60) + b, None, 15, True)
    # ---- the piece rule
    for k in (15, 31):
        for n in PIECE_RUNS(k):
            rng = np.random.default_rng(9000 + n)
            out["piece_rule_run_of_%d_k%d" % (n, k)] = Case(fa(b"s", seq_of(rng, 40 + n % 7)) + fa(b"long", seq_of(rng, 30) + b"N" + seq_of(rng, n) + b"N" + seq_of(rng, 50)) + fa(b"t", seq_of(rng, 44)), None, k, True)
    # ---- the edges of the device packer's chunks (CHUNK bytes each)
    rng = np.random.default_rng(10)
    head = fa(b"first", seq_of(rng, 500))
    t = padded_to(head, CHUNK - 61) + seq_of(rng, 60) + b"\n"
    assert len(t) == CHUNK
    out["chunk_edge_newline_then_header_k15"] = Case(t + fa(b"next", seq_of(rng, 300)), None, 15, True)
    t = padded_to(head, CHUNK - 60) + seq_of(rng, 59) + b"\r\n"
    assert t[CHUNK - 1:CHUNK + 1] == b"\r\n"
    out["chunk_edge_crlf_across_k15"] = Case(t + wrap(seq_of(rng, 200), 60) + fa(b"next", seq_of(rng, 300)), None, 15, True)
    t = padded_to(head, CHUNK - 130) + wrap(seq_of(rng, 120), 60)[:-1] + b"\n>" + b"ACGTACGTAC" * 3 + b"\n" + wrap(seq_of(rng, 200), 60)
    assert t.index(b"\n>ACGT") + 1 < CHUNK < t.index(b"\n>ACGT") + 30
    out["chunk_edge_header_across_k15"] = Case(t, None, 15, True)
    t = padded_to(head, CHUNK - 200) + wrap(seq_of(rng, 100), 60) + b">" + b"ACGT" * (2 * CHUNK // 4 + 100) + b"\n" + wrap(seq_of(rng, 200), 60)
    assert t.index(b">ACGTACGT") < CHUNK and t.index(b">ACGTACGT") + 2 * CHUNK + 400 > 3 * CHUNK
    out["chunk_edge_header_covers_a_whole_chunk_k15"] = Case(t + fa(b"z", seq_of(rng, 100)), None, 15, True)
    out["run_across_three_chunks_k15"] = Case(padded_to(head, CHUNK - 300) + wrap(seq_of(rng, 2 * CHUNK + 600), 60) + fa(b"z", seq_of(rng, 100)), None, 15, True)
    # ---- two files
    rng = np.random.default_rng(11)
    a = b"".join(fa(b"a%d" % i, with_invalid(rng, seq_of(rng, int(n)), 0.01), 70) for i, n in enumerate(rng.integers(20, 400, 15)))
    b = b"".join(fa(b"b%d" % i, with_invalid(rng, seq_of(rng, int(n)), 0.01), 60) for i, n in enumerate(rng.integers(20, 400, 10)))
    out["two_files_first_without_last_newline_k31"] = Case(a[:-1], b, 31, True)
    out["two_files_k15"] = Case(a, b"\n\n" + b, 15, True)
    out["two_files_second_empty_k31"] = Case(a, b"", 31, True)
    # ---- nothing at all: as an empty FASTQ text, no records and no error
    out["empty_text_k15"] = Case(b"", None, 15, True)
    out["only_newlines_k15"] = Case(b"\n\r\n\n", None, 15, True)
    # ---- refusals
    fastq = b"@r\n" + seq_of(rng, 50) + b"\n+\n" + b"I" * 50 + b"\n"
    out["refused_sequence_in_front_of_the_first_header"] = Case(b"ACGT\n>r\nACGT\n", None, 15, False)
    out["refused_a_fastq_text"] = Case(fastq, None, 15, False)
    out["refused_blank_lines_then_sequence"] = Case(b"\n\r\nACGT\n>r\nACGT\n", None, 15, False)
    out["refused_sequence_in_front_of_the_first_header_of_file_2"] = Case(a, b"ACGT\n>r\nACGT\n", 15, False)
    out["refused_a_fastq_text_as_file_2"] = Case(a[:-1], fastq, 15, False)
    # ---- fuzz
    for i in range(200):
        out["fuzz_%03d" % i] = fuzz_case(41000 + i)
    _CASES = out
    return out


_REF = {}


def reference(name):
    """ref_pack_fasta of a catalogue case, computed once"""
    if name not in _REF:
        c = cases()[name]
        _REF[name] = ref_pack_fasta(c.f1, c.k, c.f2)
    return _REF[name]


def twin_of(c):
    """the FASTQ twin of a regular case (both files, file 1 first)"""
    return fastq_twin(c.f1) + (fastq_twin(c.f2) if c.f2 is not None else b"")
