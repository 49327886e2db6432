"""shk_host_unitig_chains — the S10 walk alone, from settled arrays (unitig_chains in csrc/unitig_graph.cpp) — pinned
against a walk written here with plain Python dicts and lists, which shares nothing with the library; and the inputs
both entry points of the walk refuse, one test per rule of unitig_chains_check.  The device twin is compared with this
entry point's text in test_gpu_unitig_chains.py."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sparrowhawk_amd import _lib
from unitig_chains_cases import NIL, N_RANDOM, Builder, chains_text, random_case, refused_cases


def python_walk(c):
    """the text of the entry points for case c: heads in ascending record number, the strand with the smaller first k-mer
    (or the chain that is its own mirror strand), text offsets as the running sum of nodes + k - 1; then what closes on
    itself, by its lowest record; then the rings from the start"""
    n, k = c.n, c.k
    key = {r: sum(int(c.first[r][w]) << (64 * w) for w in range(c.W)) for r in range(n)}
    succ = {r: int(c.succ[r]) for r in range(n) if int(c.succ[r]) != NIL}
    mirror = {r: int(c.mirror[r]) for r in range(n)}
    linear = [r for r in range(n) if c.alive[r] and not c.circ[r]]
    has_pred = set(succ.values())
    lines, seen, need, text_off = [], set(), [], 0
    for r in linear:
        if r in has_pred:
            continue
        chain = [r]
        while chain[-1] in succ:
            chain.append(succ[chain[-1]])
        seen.update(chain)
        other = mirror[chain[-1]]
        if other != r and not key[r] < key[other]:
            continue
        nodes, kc, spelled = 0, 0, []
        for x in chain:
            spelled.append("%d@%d" % (x, nodes))
            nodes += int(c.len[x]); kc += int(c.kc[x])
        lines.append("0 %d %d %d : %s" % (nodes, kc, text_off, " ".join(spelled)))
        text_off += nodes + k - 1
    for r in linear:
        if r in seen:
            continue
        ring = [r]
        while succ.get(ring[-1], r) != r:
            ring.append(succ[ring[-1]])
        seen.update(ring)
        for x in ring:
            seen.add(mirror[x]); need += [x, mirror[x]]
        lines.append("1 %d %d - : %s" % (sum(int(c.len[x]) for x in ring), sum(int(c.kc[x]) for x in ring), " ".join(map(str, ring))))
    for r in range(n):
        if c.alive[r] and c.circ[r]:
            need.append(r)
            lines.append("1 %d %d - : %d" % (int(c.len[r]), int(c.kc[r]), r))
    lines.append("need_min :" + "".join(" %d" % r for r in need))
    return "\n".join(lines) + "\n"


@pytest.mark.parametrize("block", range(6))
def test_host_walk_equals_the_python_walk(block):
    L = _lib.load()
    kinds = set()
    for i in range(block * 50, block * 50 + 50):
        c = random_case(i)
        text = chains_text(L, "shk_host_unitig_chains", c)
        assert text == python_walk(c), f"case {i} (k={c.k}, {c.n} records)"
        kinds |= {line[0] for line in text.split("\n") if line[:2] in ("0 ", "1 ")}
    assert kinds == {"0", "1"}, "a block of these seeds holds linear contigs and rings"
    assert block * 50 + 50 <= N_RANDOM


def test_host_walk_hand_checked():
    # a chain of two on both strands, its records 0 -> 1 and 2 -> 3 with mirror[0] = 3; a ring of two that is its own mirror
    # strand (4 <-> 5); a ring from the start (6) and a dead one (7)
    B = Builder(31, 1)
    B.chain_pair(2); B.self_ring(2); B.circ_record(1); B.circ_record(0)
    c = B.build(shuffle=False, ln=10, kc=7)
    c.first[:, 0] = [5, 9, 4, 8, 1, 2, 3, 0]                  # head 2 starts with the smaller k-mer than head 0
    text = chains_text(_lib.load(), "shk_host_unitig_chains", c)
    assert text == "0 20 14 0 : 2@0 3@10\n1 20 14 - : 4 5\n1 10 7 - : 6\nneed_min : 4 5 5 4 6\n"
    assert text == python_walk(c)


def test_no_records():
    c = Builder(31, 1).build()
    assert chains_text(_lib.load(), "shk_host_unitig_chains", c) == "need_min :\n"


def test_arrays_missing_is_a_parameter_error():
    L = _lib.load()
    c = Builder(31, 1)
    c.chain_pair(2)
    c = c.build()
    args = list(c.args())
    for i in range(2, len(args)):
        bad = list(args); bad[i] = None
        assert not L.shk_host_unitig_chains(*bad)
    assert not L.shk_host_unitig_chains(32, *args[1:])         # k even


@pytest.mark.parametrize("name", [name for name, _c, _m in refused_cases()])
def test_refused_input(name):
    (case, message), = [(c, m) for nm, c, m in refused_cases() if nm == name]
    assert chains_text(_lib.load(), "shk_host_unitig_chains", case) == message
