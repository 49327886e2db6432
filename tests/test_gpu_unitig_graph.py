"""GPU tests of csrc/unitig_graph_gpu.hip — SPEC S9 on UNITIG records as kernels, the device twin of the host stage of the
sharded assembly (csrc/unitig_graph.cpp).  Everything goes through shk_device_unitig_assemble; the yardstick is the host
entry point's text on the same records, byte for byte, and — for the random graphs — the oracle's contigs.

The hand-built cases spell their records as (first k-mer, last k-mer, nodes, summed count) of one strand; the mirror
strand is added as a record of its own, as the sharded assembly hands them over.  Links follow from the k-mers alone: a
record ending in a + X is followed by every record starting with X + b (X: k-1 bases)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pygraph import PyGraph, rc
from sparrowhawk_amd import _lib
from test_oracle import _random_graph_case
from test_unitig_graph import kmer_words, library_contigs
from util import parse_fastq, revcomp, run_oracle

pytestmark = pytest.mark.gpu


def _text(fn, L, args):
    ptr = fn(*args)
    assert ptr, "the entry point returned NULL"
    text = C.string_at(ptr).decode()
    L.shk_host_free(ptr)
    return text


class BothPaths:
    """Stands in for the library in test_unitig_graph.library_contigs: every call of the host entry point also runs the
    device entry point on the same arguments and compares the two texts."""

    def __init__(self, L):
        self._L = L
        self.calls = 0

    def shk_host_unitig_assemble(self, *args):
        dev = _text(self._L.shk_device_unitig_assemble, self._L, args)
        ptr = self._L.shk_host_unitig_assemble(*args)
        assert ptr
        assert dev == C.string_at(ptr).decode(), "device and host text differ"
        self.calls += 1
        return ptr

    def shk_host_free(self, ptr):
        self._L.shk_host_free(ptr)


# ---- 1. the oracle family ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", range(8))
def test_device_unitig_correction_equals_host_text_and_oracle(block):
    """The eight blocks of 40 random small graphs of test_unitig_level_correction_equals_the_oracle, on other seeds: the
    device text equals the host text (BothPaths), and the contigs spelled from it, their summed counts and the removal
    counts are the oracle's.  (A block takes 2 - 4 s on the GPU box, nearly all of it the Python graph and the oracle.)"""
    L = BothPaths(_lib.load())
    rng = np.random.default_rng(7100 + block)
    tips = bubbles = 0
    for case in range(block * 40, block * 40 + 40):
        fq, k, min_count, flags = _random_graph_case(rng, case)
        counts = {}
        for rd, _q in parse_fastq(fq):
            for i in range(len(rd) - k + 1):
                s = rd[i:i + k]
                r = revcomp(s)
                x = s if s < r else r
                counts[x] = counts.get(x, 0) + 1
        pg = PyGraph(counts, k, min_count)
        o = run_oracle([fq], k=k, min_count=min_count, min_qual=0, **flags)
        o.assemble()
        got, removed = library_contigs(L, pg, k, not flags["no_dead_end_removal"], not flags["no_bubble_collapse"],
                                       drop_mirror_of_short_rings=bool(case % 2))
        want = list(zip(o.contigs(), [int(x) for x in o.contig_kc()]))
        assert got == want, f"case {case}: contigs differ (k={k}, {len(got)} vs {len(want)})"
        assert removed == (o.tips_removed, o.bubbles_removed), f"case {case}"
        tips += removed[0]
        bubbles += removed[1]
    assert L.calls == 40
    assert tips > 0 and bubbles > 0, "a block of these seeds removes both tips and bubbles"


# ---- 2. / 3. hand-built records ---------------------------------------------------------------------------------------
class Records:
    """Unitigs spelled by hand.  mode: where the k-mers differ — "any": everywhere, "hi": only in their first 20 bases (the
    highest word of a wide key), "lo": only in their last 20 bases (the lowest word); the one base a link's two sides differ
    by, and the mirror strands (whose ends are the other ends), fall where they must."""
    VAR = 20

    def __init__(self, k, mode="any", seed=1):
        self.k, self.mode, self.W = k, mode, (2 * k + 63) // 64
        self.rng = np.random.default_rng(seed * 1000 + k)
        self.filler = self._rnd(k)
        self.rows = []                                       # (first, last, nodes, kc, circ)

    def _rnd(self, n):
        return "".join(self.rng.choice(list("ACGT"), n))

    def seq(self, n):
        """n bases that differ from every other call's where the mode says"""
        if self.mode == "any" or n <= self.VAR:
            return self._rnd(n)
        v = self._rnd(self.VAR)
        return v + self.filler[:n - self.VAR] if self.mode == "hi" else self.filler[:n - self.VAR] + v

    def kmer(self):
        return self.seq(self.k)

    def core(self):
        return self.seq(self.k - 1)

    def unit(self, first, last, nodes, kc):
        assert len(first) == self.k and len(last) == self.k
        self.rows.append((first, last, nodes, kc, 0))
        if first != rc(last):                                # (a record that is its own mirror strand comes once)
            self.rows.append((rc(last), rc(first), nodes, kc, 0))
        return len(self.rows) - 1

    def ring(self, first, last, nodes, kc):
        self.rows.append((first, last, nodes, kc, 1))

    def arrays(self):
        n, W = len(self.rows), self.W
        first = np.zeros((n, W), dtype=np.uint64); last = np.zeros((n, W), dtype=np.uint64)
        ln = np.zeros(n, dtype=np.uint64); kc = np.zeros(n, dtype=np.uint64); circ = np.zeros(n, dtype=np.uint8)
        mk = np.zeros((n, W), dtype=np.uint64); mo = np.zeros(n, dtype=np.uint8); mp = np.zeros(n, dtype=np.uint64)
        for r, (f, l, nn, c, ci) in enumerate(self.rows):
            first[r] = kmer_words(f, W); last[r] = kmer_words(l, W)
            ln[r], kc[r], circ[r] = nn, c, ci
            # the smallest node of a record, wanted for rings only: any key will do as long as both paths get the same
            mk[r] = kmer_words(min(f, rc(f)), W); mo[r] = 0 if ci else int(f > rc(f)); mp[r] = r % max(1, nn)
        return first, last, ln, kc, circ, mk, mo, mp


def run_both(k, arrays, tips=1, bubbles=1):
    """host text == device text; returns (text, (tips removed, bubbles removed)) or (error line, None)"""
    L = _lib.load()
    first, last, ln, kc, circ, mk, mo, mp = arrays
    args = (k, len(ln), first.ctypes.data, last.ctypes.data, ln.ctypes.data, kc.ctypes.data, circ.ctypes.data,
            mk.ctypes.data, mo.ctypes.data, mp.ctypes.data, int(tips), int(bubbles))
    host = _text(L.shk_host_unitig_assemble, L, args)
    dev = _text(L.shk_device_unitig_assemble, L, args)
    assert dev == host, f"device:\n{dev[:600]}\nhost:\n{host[:600]}"
    if host.startswith("error:"):
        return host, None
    return host, tuple(int(x) for x in host.split("\n")[0].split()[1:])


def contig_nodes(text):
    return sorted(int(line.split()[2]) for line in text.strip().split("\n")[1:])


J_NODES, P_NODES = 1300, 1400                                # chains too long for a tip or a bubble branch at every k (2k <= 510)


def junction(R, n_tips, tip_nodes, tip_kc):
    """J with four in-edges: n_tips short dead ends, the rest long chains"""
    x = R.core()
    R.unit(x + "A", R.kmer(), J_NODES, 10 * J_NODES)
    for i, b in enumerate("ACGT"):
        if i < n_tips:
            R.unit(R.kmer(), b + x, tip_nodes[i], tip_kc[i])
        else:
            R.unit(R.kmer(), b + x, P_NODES, 10 * P_NODES)


def case_four_tips(k, mode):
    R = Records(k, mode, 11)
    junction(R, 4, (3, 9, 9, 5), (30, 80, 90, 500))           # t == d: the best — 9 nodes, count 90 — stays
    _t, removed = run_both(k, R.arrays())
    assert removed == (3 + 9 + 5, 0)


def case_three_tips(k, mode):
    R = Records(k, mode, 12)
    junction(R, 3, (3, 9, 5), (30, 80, 500))                  # t < d: all go
    text, removed = run_both(k, R.arrays())
    assert removed == (17, 0)
    assert contig_nodes(text) == [J_NODES + P_NODES]          # what is left is one simple link


def case_tips_tied(k, mode):
    R = Records(k, mode, 13)
    x = R.core()
    R.unit(x + "C", R.kmer(), J_NODES, 10 * J_NODES)
    a, b = R.kmer(), R.kmer()
    R.unit(a, "G" + x, 7, 70)
    R.unit(b, "T" + x, 7, 70)                                 # equal in (len, sum): the smaller canonical first k-mer stays
    text, removed = run_both(k, R.arrays())
    assert removed == (7, 0)
    stays = 0 if min(a, rc(a)) < min(b, rc(b)) else 1
    kept = [line for line in text.strip().split("\n")[1:] if int(line.split()[2]) == J_NODES + 7]
    assert len(kept) == 1 and {int(r) // 2 for r in kept[0].split(":")[1].split()} == {0, 1 + stays}


def case_tips_fully_equal(k, mode):
    # equal in (len, sum) AND in their canonical first k-mer (one starts with a, the other with revcomp(a)): the host keeps the
    # first of its ascending candidates, so the device's last tie-break is the lower start record
    R = Records(k, mode, 16)
    x = R.core()
    R.unit(x + "C", R.kmer(), J_NODES, 10 * J_NODES)
    a = R.kmer()
    R.unit(a, "G" + x, 7, 70)                                 # records 2, 3
    R.unit(rc(a), "T" + x, 7, 70)                             # records 4, 5
    text, removed = run_both(k, R.arrays())
    assert removed == (7, 0)
    kept = [line for line in text.strip().split("\n")[1:] if int(line.split()[2]) == J_NODES + 7]
    assert len(kept) == 1 and {int(r) // 2 for r in kept[0].split(":")[1].split()} == {0, 1}


def case_bubble_counts_beyond_64_bit_products(k, mode):
    # weak: 12 nodes, kc 3 * 2^60; strong: 10 nodes, kc 2^62.  strong.kc * 12 = 3 * 2^64 against weak.kc * 10 = 30 * 2^60: the
    # low 64 bits alone (0 against 14 * 2^60) order the two the wrong way round
    R = Records(k, mode, 17)
    x, y = R.core(), R.core()
    R.unit(R.kmer(), "A" + x, J_NODES, 10 * J_NODES)
    R.unit(y + "G", R.kmer(), P_NODES, 10 * P_NODES)
    R.unit(x + "A", "A" + y, 12, 3 << 60)
    R.unit(x + "C", "C" + y, 10, 1 << 62)
    text, removed = run_both(k, R.arrays())
    assert removed == (0, 12)
    assert contig_nodes(text) == [J_NODES + 10 + P_NODES]


def tip_path(k, mode, total):
    """a dead end of three records, `total` nodes in all, beside a long chain into J"""
    R = Records(k, mode, 14)
    x, y, z = R.core(), R.core(), R.core()
    R.unit(x + "A", R.kmer(), J_NODES, 10 * J_NODES)
    R.unit(R.kmer(), "C" + x, P_NODES, 10 * P_NODES)
    R.unit(R.kmer(), "A" + y, 5, 50)
    R.unit(y + "C", "G" + z, total - 10, 10 * (total - 10))
    R.unit(z + "T", "T" + x, 5, 50)
    return run_both(k, R.arrays())


def case_tip_path_at_the_limit(k, mode):
    text, removed = tip_path(k, mode, 2 * k)
    assert removed == (2 * k, 0)
    assert contig_nodes(text) == [J_NODES + P_NODES]          # round 2 finds no fork left: the long chain runs into J
    text, removed = tip_path(k, mode, 2 * k + 1)
    assert removed == (0, 0)
    assert contig_nodes(text) == [2 * k + 1, J_NODES, P_NODES]


def bubble(k, mode, weak_nodes, third=None, weak_kc_per_node=2, strong=(10, 200), tips=1, bubbles=1):
    R = Records(k, mode, 15)
    x, y = R.core(), R.core()
    R.unit(R.kmer(), "A" + x, J_NODES, 10 * J_NODES)          # S
    R.unit(y + "G", R.kmer(), P_NODES, 10 * P_NODES)          # E
    R.unit(x + "A", "A" + y, weak_nodes, weak_kc_per_node * weak_nodes)
    R.unit(x + "C", "C" + y, strong[0], strong[1])
    if third == "dead end":
        R.unit(x + "G", R.kmer(), 6, 600)
    elif third == "elsewhere":
        z = R.core()
        R.unit(x + "G", "A" + z, 6, 600)
        R.unit(z + "C", R.kmer(), J_NODES, 10 * J_NODES)
        R.unit(R.kmer(), "C" + z, J_NODES, 10 * J_NODES)
    return run_both(k, R.arrays(), tips, bubbles), R


def case_bubble_at_the_limit(k, mode):
    (text, removed), _R = bubble(k, mode, 2 * k)
    assert removed == (0, 2 * k)
    assert contig_nodes(text) == [J_NODES + 10 + P_NODES]
    (text, removed), _R = bubble(k, mode, 2 * k + 1)
    assert removed == (0, 0)


def case_bubble_from_both_sides(k, mode):
    # equal means, different lengths: the shorter branch is the better one — S and rc(E) both see the bubble, one side decides
    (text, removed), _R = bubble(k, mode, 20, weak_kc_per_node=20, strong=(10, 200))
    assert removed == (0, 20)


def case_three_branches(k, mode):
    # two of three branches end at E; the third is a dead end — seen from its mirror strand it is a tip on rc(S), which has
    # three in-edges: it goes in the tip round, the weak branch in the bubble round behind it — or it ends at another junction
    (text, removed), _R = bubble(k, mode, 12, third="dead end")
    assert removed == (6, 12)
    (text, removed), _R = bubble(k, mode, 12, third="elsewhere")
    assert removed == (0, 12)


WIDE = [(63, "hi"), (63, "lo"), (127, "hi"), (127, "lo"), (255, "hi"), (255, "lo")]
TIP_AND_BUBBLE_CASES = [case_four_tips, case_three_tips, case_tips_tied, case_tips_fully_equal, case_tip_path_at_the_limit,
                        case_bubble_at_the_limit, case_bubble_from_both_sides, case_bubble_counts_beyond_64_bit_products,
                        case_three_branches]


@pytest.mark.parametrize("case", TIP_AND_BUBBLE_CASES, ids=lambda f: f.__name__)
def test_hand_built_tips_and_bubbles(case):
    case(31, "any")


@pytest.mark.parametrize("k,mode", WIDE)
@pytest.mark.parametrize("case", TIP_AND_BUBBLE_CASES, ids=lambda f: f.__name__)
def test_wide_keys(case, k, mode):
    """k = 63, 127, 255 (2, 4, 8 words), the k-mers differing in their highest words only, and in their lowest words only:
    a comparison or a hash that drops a word merges records or orders them wrongly."""
    case(k, mode)


def test_no_records():
    R = Records(31)
    text, removed = run_both(31, R.arrays())
    assert text == "removed 0 0\n"


def test_one_ring_record():
    R = Records(31)
    R.ring(R.kmer(), R.kmer(), 500, 5000)
    text, removed = run_both(31, R.arrays())
    assert text == "removed 0 0\n1 0 500 5000 : 0\n"


def test_one_unitig_on_both_strands():
    R = Records(31)
    R.unit(R.kmer(), R.kmer(), 50, 500)
    text, removed = run_both(31, R.arrays())
    assert removed == (0, 0) and contig_nodes(text) == [50]


def test_a_record_that_is_its_own_mirror():
    R = Records(31)
    f = R.kmer()
    R.unit(f, rc(f), 40, 400)                                 # first == revcomp(last)
    assert len(R.rows) == 1
    R2 = Records(31, seed=2)                                  # ... and one with a dead end and a long chain running into it
    x = R2.core()
    g = x + "A"
    R2.unit(g, rc(g), J_NODES, 10 * J_NODES)
    R2.unit(R2.kmer(), "C" + x, 4, 40)
    R2.unit(R2.kmer(), "G" + x, P_NODES, 10 * P_NODES)
    assert len(R2.rows) == 5
    text, removed = run_both(31, R.arrays())
    assert removed == (0, 0) and contig_nodes(text) == [40]
    text, removed = run_both(31, R2.arrays())
    assert removed == (4, 0)


def test_a_ring_of_several_records_that_forms_after_a_removal():
    k = 31
    R = Records(k)
    x, y = R.core(), R.core()
    R.unit(y + "A", "C" + x, 200, 2000)                       # R1 -> R2 -> R1, and a dead end into R1's first node
    R.unit(x + "G", "T" + y, 150, 1500)
    R.unit(R.kmer(), "G" + y, 6, 60)
    text, removed = run_both(k, R.arrays())
    assert removed == (6, 0)
    lines = text.strip().split("\n")[1:]
    assert len(lines) == 1 and lines[0].startswith("1 ") and int(lines[0].split()[2]) == 350


@pytest.mark.parametrize("tips,bubbles", [(0, 1), (1, 0), (0, 0)])
def test_rounds_switched_off(tips, bubbles):
    k = 31
    R = Records(k, "any", 21)
    junction(R, 3, (3, 9, 5), (30, 80, 500))
    _t, removed = run_both(k, R.arrays(), tips, bubbles)
    assert removed == ((17, 0) if tips else (0, 0))
    (_t, removed), _R = bubble(k, "any", 12, tips=tips, bubbles=bubbles)
    assert removed == ((0, 12) if bubbles else (0, 0))


# ---- 4. more records than one launch's threads ------------------------------------------------------------------------
def _revcomp31(x):
    mask = np.uint64((1 << 62) - 1)
    x = (~x) & mask
    out = np.zeros_like(x)
    for i in range(31):
        out |= ((x >> np.uint64(2 * i)) & np.uint64(3)) << np.uint64(2 * (30 - i))
    return out


def test_large_graph_on_the_device():
    """The graph of test_large_unitig_graph_takes_the_threaded_passes — 72 000 unitigs on both strands: 46 000 isolated ones,
    10 000 pairs joined by a simple link, 2 000 forks with a 5-node dead end — built with numpy; the same expectations.
    144 000 records are more than the 65 536 from which the host code itself goes parallel, and more than the 131 072
    threads of the largest launch: the grids stride."""
    k = 31
    rng = np.random.default_rng(5)
    mask = (1 << 62) - 1

    def rnd(n):
        return rng.integers(0, mask, n, dtype=np.uint64)
    top = np.uint64(3 << 60)
    n_iso, n_pair, n_fork = 46000, 10000, 2000
    f = [rnd(n_iso)]; l = [rnd(n_iso)]; nodes = [np.full(n_iso, 40)]
    expect = {frozenset([i]): 40 for i in range(n_iso)}
    base = n_iso
    bf = rnd(n_pair)                                          # A -> B: A's last k-mer overlaps B's first by k-1
    f += [rnd(n_pair), bf]; l += [(rnd(n_pair) & top) | (bf >> np.uint64(2)), rnd(n_pair)]
    nodes += [np.full(n_pair, 30), np.full(n_pair, 50)]
    for i in range(n_pair):
        expect[frozenset([base + i, base + n_pair + i])] = 80
    base += 2 * n_pair
    jf = rnd(n_fork)                                          # J, a long chain into it (first base A) and a dead end (first base C)
    pre = jf >> np.uint64(2)
    f += [jf, rnd(n_fork), rnd(n_fork)]; l += [rnd(n_fork), pre, pre | np.uint64(1 << 60)]
    nodes += [np.full(n_fork, 100), np.full(n_fork, 200), np.full(n_fork, 5)]
    for i in range(n_fork):
        expect[frozenset([base + i, base + n_fork + i])] = 300
    f = np.concatenate(f); l = np.concatenate(l); nodes = np.concatenate(nodes).astype(np.uint64)
    n = 2 * len(f)
    assert n == 144000
    first = np.zeros(n, dtype=np.uint64); last = np.zeros(n, dtype=np.uint64)
    first[0::2] = f; last[0::2] = l; first[1::2] = _revcomp31(l); last[1::2] = _revcomp31(f)
    ln = np.repeat(nodes, 2); kc = ln * np.uint64(10); circ = np.zeros(n, dtype=np.uint8)
    L = _lib.load()
    args = (k, n, first.ctypes.data, last.ctypes.data, ln.ctypes.data, kc.ctypes.data, circ.ctypes.data, None, None, None, 1, 1)
    text = _text(L.shk_device_unitig_assemble, L, args)
    assert not text.startswith("error:"), text[:200]
    lines = text.strip().split("\n")
    assert lines[0] == "removed %d 0" % (n_fork * 5)
    got = {}
    for line in lines[1:]:
        head, ids = line.split(":")
        ring, _rot, nn, _kc = (int(x) for x in head.split())
        assert ring == 0
        got[frozenset(int(r) // 2 for r in ids.split())] = nn
    assert got == expect
    assert text == _text(L.shk_host_unitig_assemble, L, args)


# ---- 5. inconsistent input --------------------------------------------------------------------------------------------
def _drop(arrays, r):
    return tuple(np.ascontiguousarray(np.delete(a, r, axis=0)) for a in arrays)


def test_inconsistent_records_are_reported_as_the_host_reports_them():
    k = 31
    R = Records(k, "any", 31)
    junction(R, 3, (3, 9, 5), (30, 80, 500))
    good = R.arrays()
    text, none = run_both(k, _drop(good, 1))                  # a linear record without its mirror
    assert none is None and text == "error: unitig graph: a chain without its mirror strand"
    dup = tuple(np.ascontiguousarray(np.concatenate([a, a[:1]], axis=0)) for a in good)
    text, none = run_both(k, dup)                             # two records with the same first k-mer
    assert none is None and text == "error: unitig graph: two chains start at the same oriented node"
    # mirrors that do not pair up: A's mirror is A', and so is B's (B ends as A does, and starts elsewhere)
    R2 = Records(k, "any", 32)
    a_first, a_last = R2.kmer(), R2.kmer()
    R2.unit(a_first, a_last, 40, 400)
    R2.rows.append((R2.kmer(), a_last, 40, 400, 0))
    text, none = run_both(k, R2.arrays())
    assert none is None and text == "error: unitig graph: mirror strands do not pair up"
    _t, removed = run_both(k, good)                           # the device is as usable as before
    assert removed == (17, 0)
