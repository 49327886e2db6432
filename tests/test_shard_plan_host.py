"""The host planning of the sharded assembly (csrc/shard_plan.h) without a GPU: tests/cpp/shard_plan_main.cpp runs it on cases
made by hand, as a stand-alone program built with AddressSanitizer and UBSan (their runtimes linked into the program: nothing
preloaded, no Python in the process).  What it checks: the order table over the first chains and its error, the end requests
of two ranks, the records for one and three key words, the ring min-key merge over three ranks with its ties, the layout in
both forms with its error, the contig lists of the two writers with the two reasons to decline, and the threaded loop at the
size where it starts to use threads."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shard_plan_host_cases(tmp_path):
    exe = str(tmp_path / "shard_plan_main")
    # (-Wno-unknown-pragmas as in csrc/Makefile: kmer.h and unitig_graph.h carry `#pragma unroll` for the device compiler)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "sparrowhawk_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "shard_plan_main.cpp"), "-o", exe, "-pthread"])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.startswith("ok: ") and p.stderr == "", p.stdout + p.stderr
