"""The BGZF block encoder that the kernels and the host share (csrc/deflate_write.h; SPEC S11a) without a GPU and without
Python in the process: tests/cpp/deflate_write_main.cpp runs it as a stand-alone program built with AddressSanitizer and
UBSan (their runtimes linked into the program: nothing preloaded).  What it checks: the code lengths of 300 seeded
histograms (complete, at most 15 bits, the same ranks whoever sorts), the checksum arithmetic against zlib, the order of the
code-length code, and the catalogue of tests/bgzf_write_cases.py, generated inside the program, compressed by the shared
encoder and inflated again member by member with zlib."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_deflate_write_host_cases(tmp_path):
    exe = str(tmp_path / "deflate_write_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "sparrowhawk_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "deflate_write_main.cpp"), "-o", exe, "-pthread", "-lz"])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.startswith("ok: ") and p.stderr == "", p.stdout + p.stderr
