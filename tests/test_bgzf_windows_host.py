"""CPU tests of the two host-side rules of the windowed BGZF route (csrc/preprocess.cpp, route 2): the planner that cuts a
chain of blocks into windows of bounded text (shk_plan_bgzf_windows) and the rule by which a window's text is cut at its
last record start (shk_host_last_record_start), the latter against a model of a few lines."""
import numpy as np

NONE = (1 << 64) - 1


def plan(lib, isize, budget):
    a = np.asarray(isize, dtype=np.uint32)
    first = np.zeros(len(a) + 1, dtype=np.uint64)
    n = lib.shk_plan_bgzf_windows(a.ctypes.data if len(a) else None, len(a), budget, first.ctypes.data, len(first))
    return n, [int(x) for x in first[:max(n, 0)]]


def test_planner_on_random_block_lists(lib):
    """Windows are consecutive, cover every block once, hold at most the budget and — unless the file has no text — some;
    a budget below one block's ISIZE is refused."""
    rng = np.random.default_rng(20262)
    for case in range(300):
        nb = int(rng.integers(0, 400))
        kind = case % 4
        if kind == 0:
            isize = rng.integers(0, 65537, nb)
        elif kind == 1:
            isize = np.where(rng.random(nb) < 0.4, 0, rng.integers(1, 65537, nb))      # empty blocks anywhere
        elif kind == 2:
            isize = np.where(rng.random(nb) < 0.1, 0, 65280)                            # bgzip's own figure
        else:
            isize = np.where(rng.random(nb) < 0.5, 0, 65536)
        isize = np.asarray(isize, dtype=np.uint32)
        budget = int(rng.choice([65536, 65537, 100000, 131072, 1 << 20, 5 << 20, 1 << 30]))
        n, first = plan(lib, isize, budget)
        assert n >= 0, (case, n)
        if nb == 0:
            assert n == 0
            continue
        assert n >= 1 and first[0] == 0, (case, first[:3])
        assert all(a < b for a, b in zip(first, first[1:])) and first[-1] < nb, case      # consecutive, none without blocks
        bounds = first + [nb]
        sums = [int(isize[a:b].astype(np.uint64).sum()) for a, b in zip(bounds, bounds[1:])]
        assert sum(sums) == int(isize.astype(np.uint64).sum())
        assert max(sums) <= budget, (case, max(sums), budget)
        if sum(sums):
            assert min(sums) > 0, (case, sums)
        else:
            assert n == 1
        # no window could have taken the first non-empty block of the next one: the cut is not earlier than it must be
        for w in range(n - 1):
            assert sums[w] + int(isize[bounds[w + 1]]) > budget, (case, w)
    # refused: a block alone beyond the budget
    assert plan(lib, [100, 65536, 5], 65535)[0] == -1
    assert plan(lib, [70000], 65536)[0] == -1
    assert plan(lib, [1, 2, 3], 2)[0] == -1
    assert plan(lib, [1, 2, 3], 3) == (2, [0, 2]) and plan(lib, [3, 2, 2], 3) == (3, [0, 1, 2]) and plan(lib, [1, 2, 3], 6) == (1, [0])
    assert plan(lib, [0, 0, 0], 65536) == (1, [0])
    # the caller's room is respected: the count comes back, `cap` entries are written
    a = np.full(10, 65536, dtype=np.uint32)
    first = np.full(3, 77, dtype=np.uint64)
    assert lib.shk_plan_bgzf_windows(a.ctypes.data, 10, 65536, first.ctypes.data, 2) == 10
    assert list(first) == [0, 1, 77]


def model(t):
    """the last line that starts with '@' and whose line after next — begun inside t — starts with '+'"""
    starts = ([0] if t else []) + [i + 1 for i in range(len(t)) if t[i] == 10 and i + 1 < len(t)]
    best = None
    for j in range(len(starts) - 2):
        if t[starts[j]] == 64 and t[starts[j + 2]] == 43:
            best = starts[j]
    return best


def host(lib, t):
    got = lib.shk_host_last_record_start(t, len(t))
    return None if got == NONE else got


def records(rng, n, crlf=False, at_quals=False, plus_text=False):
    nl = b"\r\n" if crlf else b"\n"
    out = []
    for i in range(n):
        ln = int(rng.integers(1, 40))
        seq = bytes(rng.choice(list(b"ACGTN"), ln).tolist())
        qual = bytearray(rng.integers(33, 74, ln).astype(np.uint8).tobytes())
        if at_quals and i % 2 == 0:
            qual[0] = 64                                      # '@'
        if at_quals and i % 3 == 0:
            qual[0] = 43                                      # '+'
        name = b"r%d" % i
        out.append(b"@" + name + nl + seq + nl + b"+" + (name if plus_text else b"") + nl + bytes(qual) + nl)
    return out


def test_last_record_start_against_the_model(lib):
    """Random and adversarial tails: quality lines that start with '@' (and '+'), a '+' line with text, CRLF, a tail that
    ends inside each of the four lines, and text without any boundary."""
    rng = np.random.default_rng(20263)
    assert host(lib, b"") is None
    n_found = n_none = 0
    for case in range(400):
        recs = records(rng, int(rng.integers(1, 8)), crlf=case % 3 == 1, at_quals=case % 2 == 0, plus_text=case % 5 == 0)
        text = b"".join(recs)
        if case % 7 == 3:
            text = text[int(rng.integers(0, len(recs[0]))):]      # (starts in mid-record: byte 0 still begins a line)
        # every end inside the last two records: inside each of the four lines, at each line's end, behind each newline
        lo = len(text) - len(recs[-1]) - (len(recs[-2]) if len(recs) > 1 else 0)
        for end in range(max(lo, 0), len(text) + 1):
            t = text[:end]
            want = model(t)
            assert host(lib, t) == want, (case, end, t[-80:])
            n_found += want is not None
            n_none += want is None
    assert n_found > 1000 and n_none > 100, (n_found, n_none)
    # a known answer each: the quality line '@...' is passed over, its line after next is a sequence
    r = b"@a\nACGT\n+\n@III\n@b\nGGCC\n+\n+III\n"
    assert host(lib, r) == 15
    assert host(lib, r[:23]) == 0 and host(lib, r[:24]) == 15      # r[23], the '+' line of the second record, decides '@b'
    assert host(lib, r + b"@c\nAC\n+") == 30
    # no boundary at all
    for t in (b"ACGTACGT" * 50, b"\n" * 30, b"@@@@\n@@@@\n@@@@\n@@@@\n", b"+\n+\n+\n+\n", b"@only a header", b"@h\nACGT\n", b"\x00" * 100):
        assert model(t) is None and host(lib, t) is None, t[:20]
    # random bytes of a small alphabet: many coincidental candidates
    for case in range(300):
        t = bytes(rng.choice(list(b"@+\nA\r"), int(rng.integers(0, 200)), p=[0.2, 0.2, 0.3, 0.2, 0.1]).tolist())
        assert host(lib, t) == model(t), t
