"""The device block pool's bookkeeping (csrc/block_cache.h) and its two owners (csrc/device_mem.h: PoolBlock, PoolScope) without
a GPU: tests/cpp/pool_main.cpp runs them on a malloc backend, as a stand-alone program built with AddressSanitizer and UBSan
(their runtimes linked into the program: nothing preloaded, no Python in the process).  What it checks: size rounding, the
reuse bound, blocks and devices, who is charged and released, the one retry after a refusal, the disabled pool, trim, the
owners' release rules, and the fill-on-hand-out test mode: with it on every byte of a block equals the word — a fresh block,
a reused one of the same size, a reused larger one with its tail, a block above the 256 MiB rounding, the retry after trim —
the counter is the sum of the block sizes handed out, and with it off the backend's fill is never called."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_device_pool_bookkeeping_and_owners(tmp_path):
    exe = str(tmp_path / "pool_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "sparrowhawk_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "pool_main.cpp"), "-o", exe, "-pthread"])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.startswith("ok: ") and p.stderr == "", p.stdout + p.stderr
