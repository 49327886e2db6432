"""The host planning of the sharded preprocess (csrc/exchange_plan.h) without a GPU: tests/cpp/exchange_plan_main.cpp reads
cases from a file and prints what the header gives, as a stand-alone program built with AddressSanitizer and UBSan (their
runtimes linked into the program: nothing preloaded, no Python in the process).  The results are compared with
sparrowhawk_amd/dist.py (plan_exchange, choose_partitions) and with short restatements of the rules written here: the size
row, the dedupe verdict at its boundary, the 2^32 limit on the raw records of an owned partition, the byte layout of the two
all-to-alls, the layout of the gathered solid set and the check of the words behind the histogram."""
import os
import subprocess

import numpy as np
import pytest

from sparrowhawk_amd.dist import choose_partitions, plan_exchange

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW, AUTO, ALWAYS = 0, 1, 2
LINES = {"choose": 1, "plan": 7, "verdict": 5, "bytes": 5, "gather": 5, "histo": 1}


class Runner:
    """Collects cases, runs the program once over all of them, hands each case its lines as {name: [numbers]}."""

    def __init__(self, tmp):
        self.tmp, self.cases, self.out = tmp, [], None
        self.exe = os.path.join(tmp, "exchange_plan_main")
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                               "-I", os.path.join(ROOT, "sparrowhawk_amd", "csrc"),
                               os.path.join(ROOT, "tests", "cpp", "exchange_plan_main.cpp"), "-o", self.exe])

    def run(self, cases):
        path = os.path.join(self.tmp, "cases_%d.txt" % len(os.listdir(self.tmp)))
        with open(path, "w") as f:
            for kind, numbers in cases:
                f.write(kind + " " + " ".join(str(int(x)) for x in numbers) + "\n")
        p = subprocess.run([self.exe, path], capture_output=True, text=True)
        assert p.returncode == 0 and p.stderr == "", p.stdout + p.stderr
        lines, out = iter(p.stdout.split("\n")), []
        for kind, _ in cases:
            got = {}
            for i in range(LINES[kind]):
                name, _, rest = next(lines).partition(" ")
                got[name] = rest if kind == "histo" else [int(x) for x in rest.split()]
                if kind == "plan" and name == "plan" and got["plan"] != [0]:
                    break                                  # (a refused plan prints its code alone)
            out.append(got)
        assert [x for x in lines if x] == []
        return out


@pytest.fixture(scope="module")
def runner(tmp_path_factory):
    return Runner(str(tmp_path_factory.mktemp("exchange_plan")))


def counts_for(world, P, seed):
    """[world, P] records: one rank with none, partitions nobody has records of, sizes from 0 to beyond 2^16."""
    rng = np.random.default_rng(seed)
    pr = rng.integers(0, 70000, size=(world, P)).astype(np.uint64)
    pr[rng.integers(0, 70000, size=(world, P)) < 20000] = 0
    pr[:, rng.integers(0, P)] = 0
    if world > 1:
        pr[world - 1, :] = 0
    return pr


def test_choose_partitions(runner):
    cases = [(tot, world, per) for per in (100_000, 40_000) for world in (1, 3, 8, 128, 20000)
             for tot in (0, 1, 64 * per, 64 * per + 1, 128 * per, 16384 * per, 16384 * per + 1, 1 << 40, (1 << 64) - 1)]
    out = runner.run([("choose", c) for c in cases])
    for (tot, world, per), got in zip(cases, out):
        assert got["choose"] == [choose_partitions(tot, world, per_part=per)], (tot, world, per)


def test_plan_exchange_equals_the_python_plan(runner):
    cases = []
    for world in (1, 2, 3, 4):
        for P in (world, 64):
            pr = counts_for(world, P, 7 * world + P)
            cases += [(pr, rank) for rank in range(world)]
    edge = np.zeros((2, 4), dtype=np.uint64)
    edge[0, 1] = edge[1, 3] = 0xFFFFFFFF                   # as many as a run count holds, in partitions rank 1 owns
    cases.append((edge, 1))
    out = runner.run([("plan", [pr.shape[0], pr.shape[1], rank] + list(pr.ravel())) for pr, rank in cases])
    for (pr, rank), got in zip(cases, out):
        want = plan_exchange(pr, rank)
        assert got["plan"] == [0]
        for name, key in (("owned", "owned"), ("base", "base"), ("send", "send_counts"), ("recv", "recv_counts"), ("run_off", "run_off"),
                          ("run_cnt", "run_cnt")):
            assert got[name] == [int(x) for x in np.asarray(want[key]).ravel()], (pr.shape, rank, name)
    assert out[-1]["run_cnt"] == [0xFFFFFFFF, 0, 0, 0xFFFFFFFF]


def test_plan_exchange_refuses(runner):
    over = np.zeros((2, 4), dtype=np.uint64)
    over[0, 1] = 0x100000000                               # one more than a run count holds
    out = runner.run([("plan", [2, 4, 1] + list(over.ravel())),          # rank 1 owns partition 1
                      ("plan", [2, 4, 0] + list(over.ravel())),          # rank 0 does not: its plan stands
                      ("plan", [3, 2, 0] + [1] * 6),                     # P < world
                      ("plan", [2, 4, 2] + [1] * 8),                     # rank >= world
                      ("plan", [2, 4, 7] + [1] * 8)])
    assert [x["plan"] for x in out] == [[-1], [0], [-1], [-1], [-1]]
    assert out[1]["send"] == [0, 0x100000000]


def verdict_by_the_rules(rows):
    """rows: per rank (send, raw, failed, mode).  -> peer_failed, weighted, counts [world][P], raw_counts [world][P]"""
    modes = [m for _, _, _, m in rows]
    dd, raw = sum(sum(s) for s, _, _, _ in rows), sum(sum(r) for _, r, _, _ in rows)
    weighted = False if RAW in modes else (True if ALWAYS in modes else dd * 2 <= raw)
    return (any(f for _, _, f, _ in rows), weighted, [x for s, r, _, _ in rows for x in (s if weighted else r)],
            [x for _, r, _, _ in rows for x in r])


def fits_by_the_rules(rows, weighted, rank):
    world, P = len(rows), len(rows[0][0])
    return not weighted or all(sum(rows[r][1][p] for r in range(world)) <= 0xFFFFFFF0 for p in range(rank, P, world))


def run_verdicts(runner, cases):
    """cases: (rows, rank) -> the program's lines, each checked against the restated rules."""
    out = runner.run([("verdict", [len(rows), len(rows[0][0]), rank] + [x for s, r, f, m in rows for x in s + r + [f, m]]) for rows, rank in cases])
    for (rows, rank), got in zip(cases, out):
        peer, weighted, counts, raw_counts = verdict_by_the_rules(rows)
        assert got["rows"] == [x for s, r, f, m in rows for x in s + r + [f, m]]      # filled, then read back by its names
        assert got["verdict"] == [int(peer), int(weighted)], rows
        assert got["counts"] == counts and got["raw_counts"] == raw_counts, rows
        assert got["fit"] == [int(fits_by_the_rules(rows, weighted, rank))], (rows, rank)
    return out


def test_dedupe_verdict_at_its_boundary(runner):
    at = [([1, 2, 0], [2, 4, 0], 0, AUTO), ([3, 0, 1], [6, 0, 2], 0, AUTO)]              # 7 distinct, 14 raw: exactly half
    above = [([2, 2, 0], [2, 4, 0], 0, AUTO), at[1]]                                     # one more distinct record
    forced = [([2, 2], [2, 2], 0, AUTO), ([3, 1], [3, 1], 0, ALWAYS), ([1, 1], [1, 2], 0, AUTO)]      # nothing deduplicates
    one_raw = [([1, 0], [9, 9], 0, ALWAYS), ([1, 0], [9, 9], 0, RAW), ([0, 1], [9, 9], 0, AUTO)]
    out = run_verdicts(runner, [(at, 0), (above, 1), (forced, 2), (one_raw, 0), ([(s, r, f, AUTO) for s, r, f, _ in one_raw], 0)])
    assert [x["verdict"] for x in out] == [[0, 1], [0, 0], [0, 1], [0, 0], [0, 1]]


def test_a_failed_flag_on_each_rank_in_turn_is_reported(runner):
    rows = [([1, 2], [4, 4], 0, AUTO), ([0, 0], [0, 0], 0, AUTO), ([2, 1], [4, 4], 0, AUTO)]
    cases = [([(s, r, int(i == bad), m) for i, (s, r, _, m) in enumerate(rows)], 0) for bad in (0, 1, 2, None)]
    out = run_verdicts(runner, cases)
    assert [x["verdict"][0] for x in out] == [1, 1, 1, 0]


def test_raw_record_limit_of_an_owned_partition(runner):
    a = 0x55555550                                          # 3 * a == 0xFFFFFFF0
    def rows(extra, mode):
        # 3 ranks, 6 partitions: partition 3 belongs to rank 0; every rank holds a distinct record of it and a (+ extra) raw ones
        return [([0, 0, 0, 1, 0, 0], [0, 0, 0, a + (extra if r == 2 else 0), 0, 0], 0, mode) for r in range(3)]
    out = run_verdicts(runner, [(rows(0, ALWAYS), 0), (rows(1, ALWAYS), 0), (rows(1, ALWAYS), 1), (rows(1, ALWAYS), 2), (rows(1, RAW), 0)])
    assert [x["fit"] for x in out] == [[1], [0], [1], [1], [1]]
    assert sum(out[1]["raw_counts"]) == 0xFFFFFFF1 and out[1]["verdict"] == [0, 1] and out[4]["verdict"] == [0, 0]


def test_exchange_layout_in_bytes(runner):
    cases = [(counts_for(world, P, 100 + world), rank, elem) for world, P in ((1, 3), (3, 7), (4, 64)) for rank in range(world)
             for elem in (16, 24, 4)]
    out = runner.run([("bytes", [pr.shape[0], pr.shape[1], rank, elem] + list(pr.ravel())) for pr, rank, elem in cases])
    by_key = {}
    for (pr, rank, elem), got in zip(cases, out):
        want = plan_exchange(pr, rank)
        send, recv = [int(x) for x in want["send_counts"]], [int(x) for x in want["recv_counts"]]
        assert got["send_bytes"] == [x * elem for x in send] and got["recv_bytes"] == [x * elem for x in recv]
        assert got["send_off"] == [sum(got["send_bytes"][:r]) for r in range(len(send))]        # prefix sums of bytes
        assert got["recv_off"] == [sum(got["recv_bytes"][:r]) for r in range(len(recv))]
        assert got["n"] == [sum(send), sum(recv)]
        by_key[(pr.shape, rank, elem)] = got
    for (shape, rank, elem), got in by_key.items():          # the weights: the records' element offsets, 4 bytes each
        if elem != 4:
            w = by_key[(shape, rank, 4)]
            assert w["send_off"] == [x // elem * 4 for x in got["send_off"]] and w["recv_off"] == [x // elem * 4 for x in got["recv_off"]]
            assert all(x % elem == 0 for x in got["send_off"] + got["recv_off"])


def test_gather_layout(runner):
    cases = [[5, 0, 7], [0], [0, 0], [3], [1, 2, 3, 0], [1 << 33, 1]]
    out = runner.run([("gather", [len(c)] + c) for c in cases])
    for rows, got in zip(cases, out):
        before = [sum(rows[:r]) for r in range(len(rows))]
        assert got["off8"] == [8 * x for x in before] and got["len8"] == [8 * x for x in rows]
        assert got["off4"] == [4 * x for x in before] and got["len4"] == [4 * x for x in rows]
        assert got["total"] == [sum(rows)]


def test_histogram_words(runner):
    out = runner.run([("histo", [7, 0, 7]), ("histo", [0, 0, 0]), ("histo", [7, 0, 9]), ("histo", [(1 << 64) - 1, 3, 0])])
    assert out[0]["histo"] == "" and out[1]["histo"] == ""
    assert out[2]["histo"] == ("shard_preprocess: the ranks counted 7 k-mer instances, their reads hold 9: the record exchange lost or "
                               "duplicated data")
    assert out[3]["histo"] == ("shard_preprocess: the ranks counted 18446744073709551615 k-mer instances, their reads hold 0: the record "
                               "exchange lost or duplicated data")
