"""CPU tests of the slice rule of the sharded FASTA entry point (shk_shard_preprocess_fasta): the two host functions that state
where a FASTA record starts (shk_host_first_fasta_record_start, shk_host_last_fasta_record_start) against a restatement of the
rule in three lines of Python, the slices of every world against the host packer (the slices' records, in rank order, are the
records of the whole text), and the rule functions with fasta_slice_bounds as a stand-alone program under AddressSanitizer and
UBSan (tests/cpp/fasta_slices_main.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import fasta_cases as fa
from sparrowhawk_amd import ShkError
from sparrowhawk_amd.helper import pack_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sparrowhawk_amd", "csrc")
NONE = (1 << 64) - 1


def model_starts(t):
    """The rule: a record starts at p when t[p] == '>' and p begins a line (p == 0 or t[p - 1] == '\\n')."""
    return [p for p in range(len(t)) if t[p] == 62 and (p == 0 or t[p - 1] == 10)]


def host_first(lib, t, frm):
    return int(lib.shk_host_first_fasta_record_start(t, len(t), frm))


def host_last(lib, t):
    return int(lib.shk_host_last_fasta_record_start(t, len(t)))


def test_the_host_rule_equals_its_restatement(lib):
    rng = np.random.default_rng(99)
    texts = [c.f1 for c in fa.cases().values()] + [c.f2 for c in fa.cases().values() if c.f2 is not None]
    assert len(texts) > 250
    for t in texts:
        starts = np.asarray(model_starts(t), dtype=np.int64)
        assert host_last(lib, t) == (int(starts[-1]) if len(starts) else NONE)
        froms = [0, 1, len(t) // 2, max(len(t) - 1, 0), len(t), len(t) + 5] + [int(x) for x in rng.integers(0, len(t) + 1, 12)]
        froms += [int(s) + d for s in starts[:4] for d in (-1, 0, 1) if s + d >= 0]
        for frm in froms:
            i = int(np.searchsorted(starts, frm))
            assert host_first(lib, t, frm) == (int(starts[i]) if i < len(starts) else NONE), (t[:40], frm)
    # every `from` and every prefix of a small text
    t = b"\n>a b>c\r\nAC>GT\n\r\n>\nA\r>x\n>last"
    for n in range(len(t) + 1):
        cut = t[:n]
        starts = model_starts(cut)
        assert host_last(lib, cut) == (starts[-1] if starts else NONE), n
        for frm in range(n + 2):
            assert host_first(lib, cut, frm) == min((s for s in starts if s >= frm), default=NONE), (n, frm)
    assert model_starts(t) == [1, 17, 24]                       # ('>' inside a header and a sequence line, and behind a lone '\r': no starts)
    assert host_first(lib, b"", 0) == NONE and host_last(lib, b"") == NONE
    assert int(lib.shk_host_first_fasta_record_start(None, 0, 0)) == NONE and int(lib.shk_host_last_fasta_record_start(None, 0)) == NONE


def slices_of(lib, t, world):
    """[s_0 ... s_world] of a plain text by the rule: s_0 = 0, s_world = the end, s_r = the first start at or after floor(r * n / world)"""
    n = len(t)
    s = [0]
    for r in range(1, world):
        p = host_first(lib, t, r * n // world)
        s.append(n if p == NONE else p)
    return s + [n]


def packed(t, k):
    """(segments as arrays of codes, n_reads) by the host packer, or the error code"""
    try:
        bases, seg, nb, nr = pack_fasta(t, k)
    except ShkError as e:
        return e.code
    codes = ((np.asarray(bases, dtype=np.uint32)[:, None] >> (2 * np.arange(16, dtype=np.uint32))) & 3).astype(np.uint8).reshape(-1)
    return [codes[int(a):int(b)].tobytes() for a, b in zip(seg, seg[1:])], nr


def slice_texts():
    rng = np.random.default_rng(5150)
    # ('>' inside header lines and inside sequence lines; one that happens to begin a line begins a record, by the rule)
    recs = [fa.fa(b"r%d >x" % i, fa.with_invalid(rng, fa.seq_of(rng, int(n)), 0.02, b"N>"), 60) for i, n in enumerate(rng.integers(0, 500, 14))]
    plain = b"".join(recs)
    blank = b"\n\r\n" + b"\n\n".join(r.replace(b"\n", b"\n\n", 2) for r in recs) + b"\n\r\n\n"
    return {"newline": plain, "crlf": plain.replace(b"\n", b"\r\n"), "blank lines": blank, "no last newline": plain[:-1],
            "crlf, no last newline": plain.replace(b"\n", b"\r\n")[:-1], "one record": recs[5], "empty": b"", "headers only": b">a\n>b\n>c",
            "no header at all": fa.wrap(fa.seq_of(rng, 700), 60)}


@pytest.mark.parametrize("world", [1, 2, 3, 5, 64])
def test_the_slices_of_a_world_hold_the_records_of_the_text(lib, world):
    k = 15
    for name, t in slice_texts().items():
        starts = set(model_starts(t))
        s = slices_of(lib, t, world)
        assert s == sorted(s) and s[0] == 0 and s[-1] == len(t), (name, s)
        parts = [t[a:b] for a, b in zip(s, s[1:])]
        assert b"".join(parts) == t
        for r, (a, part) in enumerate(zip(s, parts)):
            if r > 0 and part:
                assert a in starts and part.startswith(b">"), (name, world, r)
        if world == 64:
            assert sum(1 for p in parts if p) <= max(len(starts), 1) < world      # (more ranks than records: empty slices)
        whole = packed(t, k)
        got = [packed(p, k) for p in parts]
        if name == "no header at all":                              # the lines in front of the first header lie in slice 0: refused there
            assert whole == -3 and got[0] == -3 and all(g == ([], 0) for g in got[1:]), (name, world)
            continue
        assert [seg for g in got for seg in g[0]] == whole[0], (name, world)
        assert sum(g[1] for g in got) == whole[1] == len(starts), (name, world)


def test_the_rule_stand_alone_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "fasta_slices_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "fasta_slices_main.cpp"), os.path.join(CSRC, "fastq.cpp"), os.path.join(CSRC, "inflate_mt.cpp"),
                           "-o", exe, "-pthread", "-lz"])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "" and p.stdout == "ok\n", p.stdout[-2000:] + p.stderr[-4000:]
