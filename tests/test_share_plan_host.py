"""The host planning of the share readers (csrc/share_plan.h: plan_share, estimate_share, share_in_batches) without a GPU:
tests/cpp/share_plan_main.cpp plans one rank's share of small files written here and prints the plan, as a stand-alone program
built with AddressSanitizer and UBSan (their runtimes linked into the program: nothing preloaded, no Python in the process),
and the plans are compared with a computation made here from the restatements of the slice rules in test_fastq_slices.py and
test_fasta_slices.py.  What it checks: which kind of file each one is, where the rank's nominal cuts lie, how much text the
share has, and whether the share goes in batches — all decided before a byte is uploaded."""
import gzip
import os
import struct
import subprocess
import zlib

import pytest

from test_fasta_slices import model_starts
from test_fastq_slices import model_first_record_start, plan, records
from test_gpu_shard_fastq import bgzf_block

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sparrowhawk_amd", "csrc")
NONE = (1 << 64) - 1
SHK_OK, SHK_E_PARAM = 0, -1


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("share_plan") / "share_plan_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "share_plan_main.cpp"), os.path.join(CSRC, "fastq.cpp"),
                           os.path.join(CSRC, "inflate_mt.cpp"), "-o", out, "-lz", "-pthread"])
    return out


def run(exe, tmp_path, cases):
    """cases: (fmt, rank, world, min, batch, file1, file2) — a file is bytes (written here), None (no file) or "null:N".
    Returns, per case, (the head line's fields, [the fields of each file])."""
    lines = []
    for c, (fmt, rank, world, mn, batch, f1, f2) in enumerate(cases):
        args = []
        for i, f in enumerate((f1, f2)):
            if isinstance(f, bytes):
                path = str(tmp_path / ("c%d_%d" % (c, i)))
                with open(path, "wb") as fh:
                    fh.write(f)
                args.append(path)
            else:
                args.append("-" if f is None else f)
        lines.append("%s %d %d %s %s %s %s" % (fmt, rank, world, "-" if mn is None else mn, "-" if batch is None else batch, args[0], args[1]))
    listing = str(tmp_path / "cases.txt")
    with open(listing, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    p = subprocess.run([exe, listing], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", p.stdout + p.stderr
    out = p.stdout.splitlines()
    assert out[-1] == "ok: %d cases" % len(cases)
    plans = [None] * len(cases)
    for ln in out[:-1]:
        kind, c, rest = ln.split(" ", 2)
        if kind == "case":
            head, err = rest.split(" err=", 1)
            d = {k: int(v) for k, v in (kv.split("=") for kv in head.split())}
            d["err"] = err
            plans[int(c)] = (d, [])
        else:
            i, fields = rest.split(" ", 1)
            plans[int(c)][1].append({k: int(v) for k, v in (kv.split("=") for kv in fields.split())})
    return plans


def fasta_records(n):
    return b"".join(b">s%d some words\n" % i + b"ACGTTGCA" * (i + 1) + b"\n" + b"GG" * (i % 3 + 1) + b"\n" for i in range(n))


def bounds(fmt, t, e, world):
    """[s_0 ... s_world] of the text t[:e] by the slice rule: nominal cuts floor(r * e / world)"""
    s = [0]
    for r in range(1, world):
        cut = r * e // world
        if fmt == "fastq":
            p = model_first_record_start(t[:e], cut)
        else:
            p = min((x for x in model_starts(t[:e]) if x >= cut), default=NONE)
        s.append(e if p == NONE else p)
    return s + [e]


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_plain_text_is_cut_among_the_ranks_and_its_blank_tail_left_out(exe, tmp_path, fmt):
    body = records(7, 11) if fmt == "fastq" else fasta_records(7)
    crlf = records(7, 12, b"\r\n") if fmt == "fastq" else fasta_records(7).replace(b"\n", b"\r\n")
    texts = [(body, len(body)), (body + b"\n\n\n", len(body)), (crlf + b"\r\n\r\n", len(crlf))]
    cases = [(fmt, r, w, 0, None, t, None) for t, _ in texts for w in (1, 2, 3, 8) for r in range(w)]
    plans = iter(run(exe, tmp_path, cases))
    for t, e in texts:
        for world in (1, 2, 3, 8):
            want = bounds(fmt, t, e, world)
            assert want == sorted(want)
            got = [next(plans) for _ in range(world)]
            total = 0
            for r, (head, files) in enumerate(got):
                assert head["plan_rc"] == SHK_OK and head["est_rc"] == SHK_OK and head["nf"] == 1 and head["in_batches"] == 0
                (f,) = files
                assert f["gz"] == 0 and f["walked"] == 0 and f["host"] == 1
                assert f["l"] == len(t) and f["e"] == e                          # the trailing blank lines are not text
                assert (f["c0"], f["c1"]) == (r * e // world, (r + 1) * e // world)
                assert (f["s0"], f["s1"]) == (want[r], want[r + 1]), (world, r)  # the slices tile [0, e)
                assert f["est"] == f["s1"] - f["s0"] == head["total"]
                assert f["end"] == (len(t) if f["s1"] == e else f["s1"])         # the slice that reaches the end takes the blank lines along
                total += f["est"]
            assert total == e
            if world == 8:
                assert any(f[0]["est"] == 0 for _, f in got)                     # more ranks than records


def chain_file():
    """five blocks of unequal text, an empty one in the middle, the end-of-file marker"""
    t = records(7, 21)
    n = len(t)
    cuts = [0, n * 3 // 10, n * 4 // 10, n * 4 // 10, n * 8 // 10, n]
    chunks = [t[a:b] for a, b in zip(cuts, cuts[1:])]
    assert [len(c) == 0 for c in chunks] == [False, False, True, False, False] and len({len(c) for c in chunks}) == 5
    return t, chunks, b"".join(bgzf_block(c) for c in chunks) + bgzf_block(b"")


def isize_word(z):
    return struct.unpack("<I", z[-4:])[0]


def test_a_walked_chain_is_cut_at_block_starts(exe, tmp_path, lib):
    t, chunks, z = chain_file()
    isize = [len(c) for c in chunks] + [0]
    off = [sum(isize[:b]) for b in range(len(isize) + 1)]
    worlds = (1, 2, 3, 7)
    plans = iter(run(exe, tmp_path, [("fastq", r, w, 0, None, z, None) for w in worlds for r in range(w)]))
    for world in worlds:
        first = plan(lib, isize, world)
        ests = []
        for r in range(world):
            head, (f,) = next(plans)
            assert head["plan_rc"] == SHK_OK and head["est_rc"] == SHK_OK
            assert f["gz"] == 1 and f["walked"] == 1 and f["blocks"] == 6 and f["text"] == len(t)
            assert (f["c0"], f["c1"]) == (off[first[r]], off[first[r + 1]]), (world, r)
            assert f["est"] == f["c1"] - f["c0"] == head["total"] and f["host"] == 0      # (nothing was inflated for it)
            assert (f["est"] == 0) == (sum(isize[first[r]:first[r + 1]]) == 0)
            ests.append(f["est"])
        assert sum(ests) == len(t)
        if world == 7:
            assert ests.count(0) >= 3                                            # four blocks with text: ranks with empty runs


def test_what_is_gzip_and_no_chain_is_guessed_from_its_last_word(exe, tmp_path):
    t, chunks, z = chain_file()
    truncated = z[:-9]                                                         # (the end-of-file marker lacks its trailer and a byte)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    d = c.compress(chunks[1]) + c.flush()
    named = struct.pack("<4BI2BH2BHH", 31, 139, 8, 4 | 8, 0, 0, 255, 6, 66, 67, 2, 18 + 2 + len(d) + 8 - 1) + b"n\0" + d + struct.pack("<II", zlib.crc32(chunks[1]), len(chunks[1]))
    with_fname = bgzf_block(chunks[0]) + named + b"".join(bgzf_block(x) for x in chunks[2:]) + bgzf_block(b"")
    member = gzip.compress(t)
    files = [(truncated, 0), (with_fname, 0), (z, None), (member, 0)]           # (z with SHK_GUNZIP_DEVICE_MIN unset: a small file)
    worlds = (1, 2, 3)
    plans = iter(run(exe, tmp_path, [("fastq", w - 1, w, mn, None, f, None) for f, mn in files for w in worlds]))
    for f, mn in files:
        for world in worlds:
            head, (g,) = next(plans)
            assert head["plan_rc"] == SHK_OK and head["est_rc"] == SHK_OK
            assert g["gz"] == 1 and g["walked"] == 0 and g["host"] == 0
            assert g["est"] == isize_word(f) // world == head["total"]
    assert isize_word(member) == len(t) and isize_word(truncated) != 0


def test_the_edges_of_what_a_file_is_and_the_argument_errors(exe, tmp_path):
    short = b"\x1f\x8b" + b"A" * 15
    t = records(3, 5)
    cases = [("fastq", 0, 1, 0, None, short, None), ("fastq", 0, 1, 0, None, None, None), ("fasta", 2, 3, 0, None, None, None)]
    errors = []
    for fmt in ("fastq", "fasta"):
        entry = "shard_preprocess_" + fmt
        for f1, f2, rank, world, msg in [("null:5", None, 0, 1, "a null file with a size, or a second file without a first"),
                                         (None, t, 0, 1, "a null file with a size, or a second file without a first"),
                                         (t, "null:3", 0, 1, "a null file with a size, or a second file without a first"),
                                         (t, None, 2, 2, "rank beyond world"), (t, None, 5, 2, "rank beyond world"), (t, None, 0, 0, "rank beyond world")]:
            cases.append((fmt, rank, world, 0, None, f1, f2))
            errors.append(entry + ": " + msg)
    plans = run(exe, tmp_path, cases)
    head, (f,) = plans[0]
    assert head["plan_rc"] == SHK_OK and f["gz"] == 0 and f["walked"] == 0      # 17 bytes that begin 1F 8B: too short for a member, plain text
    for head, files in plans[1:3]:
        assert head["plan_rc"] == SHK_OK and head["est_rc"] == SHK_OK and head["nf"] == 0 and files == [] and head["total"] == 0 and head["err"] == ""
    for (head, files), msg in zip(plans[3:], errors):
        assert head["plan_rc"] == SHK_E_PARAM and head["err"] == msg and files == []


def fasta_of(n):
    return b">r\n" + b"A" * (n - 4) + b"\n"


def fastq_of(n):
    ln = (n - 8) // 2
    return b"@rr\n" + b"C" * ln + b"\n+\n" + b"I" * ln + b"\n"


def test_the_share_goes_in_batches_from_one_base_beyond_a_batch(exe, tmp_path):
    """SHK_BATCH_BASES=1024, the knob's floor: a byte of FASTA text is a base, two bytes of FASTQ text hold at most one"""
    cases = [("fasta", fasta_of(1024), None, 0), ("fasta", fasta_of(1025), None, 1), ("fastq", fastq_of(2048), None, 0), ("fastq", fastq_of(2050), None, 1),
             ("fasta", fasta_of(600), fasta_of(424), 0), ("fasta", fasta_of(600), fasta_of(425), 1),
             ("fastq", fastq_of(1024), fastq_of(1024), 0), ("fastq", fastq_of(1024), fastq_of(1026), 1)]
    for fmt, f1, f2, _ in cases:
        assert all(len(f) == len(f.rstrip(b"\n")) + 1 for f in (f1, f2) if f)   # (no blank tail: the slice is the file)
    plans = run(exe, tmp_path, [(fmt, 0, 1, 0, 1024, f1, f2) for fmt, f1, f2, _ in cases])
    for (fmt, f1, f2, want), (head, files) in zip(cases, plans):
        assert head["plan_rc"] == SHK_OK and head["est_rc"] == SHK_OK and head["batch_bases"] == 1024
        assert head["total"] == len(f1) + (len(f2) if f2 else 0) == sum(f["s1"] - f["s0"] for f in files)
        if f2:
            assert all(f["est"] <= (1024 if fmt == "fasta" else 2048) for f in files)      # neither file of a pair crosses the edge alone
        assert head["in_batches"] == want, (fmt, head)
    # without the knob nothing this small goes in batches
    (head, _), = run(exe, tmp_path, [("fasta", 0, 1, 0, None, fasta_of(1025), None)])
    assert head["in_batches"] == 0 and head["batch_bases"] == 1 << 31
