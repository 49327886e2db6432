"""CPU tests of how one rank's run of BGZF blocks is cut into windows where its share exceeds one batch
(shk_plan_share_windows; csrc/share_windows.h): hand-made ISIZE lists and seeded random ones.  Every rank's windows are
consecutive, each holds at most the budget and none is without text unless the run is; over all ranks the windows cover every
block once; the result is shk_plan_fastq_slices followed by shk_plan_bgzf_windows on the rank's run; a block beyond the budget
is SHK_E_PARAM.  The header is also run alone, as a stand-alone program under AddressSanitizer and UBSan (their runtimes
linked into the program: nothing preloaded, no Python in the process)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHK_E_PARAM = -1


def slices(lib, a, world):
    first = np.zeros(world + 1, dtype=np.uint64)
    assert lib.shk_plan_fastq_slices(a.ctypes.data if len(a) else None, len(a), world, first.ctypes.data) == world
    return [int(x) for x in first]


def bgzf_windows(lib, a, budget):
    first = np.zeros(len(a) + 1, dtype=np.uint64)
    n = lib.shk_plan_bgzf_windows(a.ctypes.data if len(a) else None, len(a), budget, first.ctypes.data, len(first))
    return n if n < 0 else [int(x) for x in first[:n]]


def share_windows(lib, a, world, rank, budget):
    first = np.zeros(len(a) + 1, dtype=np.uint64)
    n = lib.shk_plan_share_windows(a.ctypes.data if len(a) else None, len(a), world, rank, budget, first.ctypes.data, len(first))
    return n if n < 0 else [int(x) for x in first[:n]]


def check(lib, isize, world, budget):
    a = np.ascontiguousarray(isize, dtype=np.uint32)
    run = slices(lib, a, world)
    covered = np.zeros(len(a), dtype=np.int64)
    for r in range(world):
        b0, b1 = run[r], run[r + 1]
        got = share_windows(lib, a, world, r, budget)
        want = bgzf_windows(lib, a[b0:b1].copy(), budget)
        if isinstance(want, int):
            assert got == SHK_E_PARAM == want, (isize, world, r)
            covered[b0:b1] += 1
            continue
        assert got == [w + b0 for w in want], (isize, world, r)                 # the composition of the two planners
        assert (got == []) == (b0 == b1)
        run_text = int(a[b0:b1].sum())
        for w, wb0 in enumerate(got):
            wb1 = got[w + 1] if w + 1 < len(got) else b1
            assert b0 <= wb0 < wb1 <= b1 and (w > 0 or wb0 == b0)               # consecutive, from the run's first block on
            text = int(a[wb0:wb1].sum())
            assert text <= budget and (text > 0 or run_text == 0), (isize, world, r, w)
            covered[wb0:wb1] += 1
    assert (covered == 1).all(), (isize, world)                                 # every block once, over all ranks


def test_hand_made_lists(lib):
    for isize, world, budget in [([], 1, 65536), ([], 3, 65536), ([4096], 1, 65536), ([4096], 4, 4096), ([0, 0, 0], 2, 65536),
                                 ([0, 100, 0, 0, 200, 0, 300, 0], 3, 300), ([65536] * 4 + [0], 2, 65536), ([10, 20, 30], 7, 30),
                                 ([100, 100, 5000, 100], 3, 4999)]:
        check(lib, isize, world, budget)


def test_a_block_beyond_the_budget_and_bad_ranks_are_parameter_errors(lib):
    a = np.array([100, 100, 5000, 100], dtype=np.uint32)
    first = np.zeros(8, dtype=np.uint64)
    assert share_windows(lib, a, 1, 0, 4999) == SHK_E_PARAM
    assert share_windows(lib, a, 1, 0, 5000) == [0, 2, 3]
    assert share_windows(lib, a, 2, 2, 5000) == SHK_E_PARAM                     # rank beyond world
    assert lib.shk_plan_share_windows(a.ctypes.data, 4, 0, 0, 5000, first.ctypes.data, 8) == SHK_E_PARAM
    assert lib.shk_plan_share_windows(None, 4, 1, 0, 5000, first.ctypes.data, 8) == SHK_E_PARAM
    big = np.array([65537], dtype=np.uint32)
    assert lib.shk_plan_share_windows(big.ctypes.data, 1, 1, 0, 1 << 20, first.ctypes.data, 8) == SHK_E_PARAM
    # cap: the count comes back whole, only `cap` entries are written
    first[:] = 77
    assert lib.shk_plan_share_windows(a.ctypes.data, 4, 1, 0, 5000, first.ctypes.data, 2) == 3
    assert [int(x) for x in first[:3]] == [0, 2, 77]


def test_200_seeded_random_lists(lib):
    rng = np.random.default_rng(20261)
    for _ in range(200):
        n = int(rng.integers(0, 120))
        isize = np.where(rng.random(n) < 0.2, 0, rng.integers(0, 65537, n)).astype(np.uint32)
        check(lib, isize, int(rng.integers(1, 10)), int(rng.integers(65536, 465536)))


def test_share_windows_header_alone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "share_windows_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "sparrowhawk_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "share_windows_main.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.startswith("ok: ") and p.stderr == "", p.stdout + p.stderr
