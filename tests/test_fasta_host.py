"""The host FASTA packer (csrc/fastq.cpp: pack_fasta) without a GPU and without Python in the process: tests/cpp/fasta_main.cpp
runs it as a stand-alone program built with AddressSanitizer and UBSan (their runtimes linked into the program, nothing
preloaded) on texts written to a temporary directory — the refusals, every prefix of one 300-byte catalogue text, the header
of 40 000 bytes and the run of 100 000 bases.  It must end clean, and its counts and checksums are those of the reference
packer (tests/fasta_cases.py)."""
import os
import subprocess

import fasta_cases as fa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sparrowhawk_amd", "csrc")
M64 = (1 << 64) - 1


def checksum(ref):
    h = 0
    for v in list(ref[1]) + list(ref[0]):
        h ^= (int(v) + 0x9E3779B97F4A7C15 + (h << 6) + (h >> 2)) & M64
    return h


def test_pack_fasta_stand_alone_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "fasta_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "fasta_main.cpp"), os.path.join(CSRC, "fastq.cpp"), os.path.join(CSRC, "inflate_mt.cpp"),
                           "-o", exe, "-pthread", "-lz"])
    cases = fa.cases()
    k = 15
    base = next(c.f1 for n, c in cases.items() if n.startswith("fuzz_") and len(c.f1) >= 300 and b"\r\n" in c.f1[:300] and b"N" in c.f1[:300]
                and c.f1[:300].count(b">") >= 3)[:300]
    texts = [c.f1 for n, c in cases.items() if not c.ok and c.f2 is None] + [cases["refused_a_fastq_text_as_file_2"].f2]
    texts += [base[:i] for i in range(len(base) + 1)]
    texts += [cases["header_of_40000_bytes_k15"].f1, cases["piece_rule_run_of_100000_k15"].f1]
    paths = []
    for i, t in enumerate(texts):
        paths.append(str(tmp_path / ("t%03d.fa" % i)))
        with open(paths[-1], "wb") as f:
            f.write(t)
    p = subprocess.run([exe, str(k)] + paths, capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", p.stdout[-2000:] + p.stderr[-4000:]
    lines = p.stdout.splitlines()
    assert lines[-1] == "ok: %d texts" % len(texts) and len(lines) == len(texts) + 1
    refused = 0
    for t, line in zip(texts, lines):
        got = [int(x) for x in line.split()]
        ref = fa.ref_pack_fasta(t, k)
        if ref is None:
            assert got[0] == -3, (t[:60], line)
            refused += 1
            continue
        assert got == [0, len(ref[1]) - 1, int(ref[1][-1]), ref[2], ref[3], checksum(ref)], (t[:60], line)
    assert refused >= 4
