"""CPU tests of the slice rule of the sharded FASTQ entry point (shk_shard_preprocess_fastq): where rank r's share of a file
begins (shk_host_first_record_start, against a restatement of the rule in a few lines of Python), that the slices of every
world partition the text at record starts, and the planner that gives every rank its run of BGZF blocks
(shk_plan_fastq_slices)."""
import numpy as np

NONE = (1 << 64) - 1


def model_first_record_start(t, frm):
    """The rule: the smallest p >= frm that begins a line, holds '@' and whose line after next begins with '+'; a line whose
    line after next has not begun inside t is undecided — the search stops there (NONE), it never passes the line over."""
    n, p = len(t), frm
    if p >= n:
        return NONE
    if p > 0 and t[p - 1] != 10:                # inside a line: the next line is the first candidate
        p = t.find(b"\n", p) + 1
        if p == 0:
            return NONE
    while p < n:
        b = t.find(b"\n", p) + 1                # the next line
        c = t.find(b"\n", b) + 1 if 0 < b < n else 0      # the line after next
        if b == 0 or c == 0 or c >= n:
            return NONE
        if t[p] == 64 and t[c] == 43:
            return p
        p = b
    return NONE


def host_first(lib, t, frm):
    return int(lib.shk_host_first_record_start(t, len(t), frm))


def records(n, seed=1, eol=b"\n"):
    """n records whose quality lines begin with '@' and with '+' now and then, and whose names and sequences vary in length"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        ln = int(rng.integers(1, 40))
        seq = bytes(rng.choice(list(b"ACGT"), ln).tolist())
        qual = bytearray(rng.integers(33, 74, ln, dtype=np.uint8).tobytes())
        qual[0] = [64, 43, 73][i % 3]            # '@', '+', 'I'
        out.append(b"@r%d" % i + eol + seq + eol + b"+" + eol + bytes(qual) + eol)
    return b"".join(out)


def test_first_record_start_equals_the_model_at_every_offset(lib):
    for eol in (b"\n", b"\r\n"):
        t = records(6, 3, eol)
        starts = [i for i in range(len(t)) if t.startswith(b"@r", i) and (i == 0 or t[i - 1] == 10)]
        assert len(starts) == 6
        for frm in range(len(t) + 2):
            want = model_first_record_start(t, frm)
            assert host_first(lib, t, frm) == want, (eol, frm)
            # the model itself, against the records as they were written: the next start whose '+' line has begun and is not
            # the text's last byte ... the last two records' tails are undecided
            if want != NONE:
                assert want == min(s for s in starts if s >= frm)
        # a quality line that begins with '@' is never taken for a start
        assert all(host_first(lib, t, s + 1) in starts + [NONE] for s in range(len(t)))


def test_a_cut_text_is_undecided_never_a_later_start(lib):
    """Every prefix of the text: what is found is what the model finds, and a start that the whole text has at or behind
    `from` is either found as it is or not decided yet — never replaced by a later one."""
    t = records(6, 4)
    for n in range(len(t) + 1):
        cut = t[:n]
        for frm in (0, 1, n // 3, n // 2, max(n - 5, 0)):
            got = host_first(lib, cut, frm)
            assert got == model_first_record_start(cut, frm), (n, frm)
            whole = model_first_record_start(t, frm)
            assert got in (whole, NONE), (n, frm, got, whole)
    assert host_first(lib, b"", 0) == NONE
    assert int(lib.shk_host_first_record_start(None, 0, 0)) == NONE
    assert host_first(lib, b"@a\nA\n+\nI\n", 100) == NONE


def slices_of(lib, t, world):
    """[s_0 ... s_world] of a plain text: nominal cuts floor(r * n / world)"""
    n = len(t)
    s = [0]
    for r in range(1, world):
        p = host_first(lib, t, r * n // world)
        s.append(n if p == NONE else p)
    return s + [n]


def test_the_slices_partition_the_text_at_record_starts(lib):
    for nrec in range(21):
        t = records(nrec, 100 + nrec)
        starts = {i for i in range(len(t)) if t.startswith(b"@r", i) and (i == 0 or t[i - 1] == 10)}
        for world in range(1, 8):
            s = slices_of(lib, t, world)
            assert s == sorted(s) and s[0] == 0 and s[-1] == len(t), (nrec, world, s)
            parts = [t[a:b] for a, b in zip(s, s[1:])]
            assert b"".join(parts) == t
            for a, part in zip(s, parts):
                if part:
                    assert a in starts, (nrec, world, a)
                    assert part.count(b"\n") % 4 == 0


def plan(lib, isize, world):
    a = np.asarray(isize, dtype=np.uint32)
    first = np.full(world + 1, 77, dtype=np.uint64)
    rc = lib.shk_plan_fastq_slices(a.ctypes.data if len(a) else None, len(a), world, first.ctypes.data)
    assert rc == world, rc
    return [int(x) for x in first]


def test_slice_planner(lib):
    rng = np.random.default_rng(515)
    cases = [[], [0], [0, 0, 0], [5], [0, 0, 7, 9, 0, 0, 3, 0, 0], [65536] * 10, [100, 100], [0, 100, 0, 100, 0]]
    for _ in range(200):
        nb = int(rng.integers(0, 60))
        cases.append(np.where(rng.random(nb) < 0.3, 0, rng.integers(1, 65537, nb)).tolist())
    for isize in cases:
        nb, text = len(isize), int(sum(isize))
        off = [int(sum(isize[:b])) for b in range(nb + 1)]
        for world in (1, 2, 3, 5, 7, nb + 3):
            first = plan(lib, isize, world)
            assert first[0] == 0 and first[world] == nb, (isize, world, first)
            assert first == sorted(first)
            for r in range(1, world):
                want = r * text // world
                b = first[r]
                assert b == nb or off[b] >= want, (isize, world, r)              # the run starts at or behind its cut ...
                assert b == 0 or off[b - 1] < want, (isize, world, r)            # ... at the FIRST such block
    assert plan(lib, [4, 4, 4, 4], 1) == [0, 4]
    assert plan(lib, [4, 4, 4, 4], 2) == [0, 2, 4]
    assert plan(lib, [100, 100], 5) == [0, 1, 1, 2, 2, 2]               # more ranks than blocks: empty runs
    assert plan(lib, [0, 0, 10, 0, 10, 0, 0], 2) == [0, 3, 7]           # empty blocks at the front, in the middle, at the end
    a = np.array([70000], dtype=np.uint32)
    first = np.zeros(2, dtype=np.uint64)
    assert lib.shk_plan_fastq_slices(a.ctypes.data, 1, 1, first.ctypes.data) == -1
    assert lib.shk_plan_fastq_slices(a.ctypes.data, 1, 0, first.ctypes.data) == -1
