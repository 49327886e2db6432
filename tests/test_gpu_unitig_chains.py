"""GPU tests of the S10 walk on the device (csrc/unitig_graph_gpu.hip: predecessors, ranks by pointer jumping, the strand
choice at the tails, the scans over the heads, the placement): shk_device_unitig_chains against shk_host_unitig_chains on
the same settled arrays, text for text — contigs, their order, nodes, counts, text offsets, every record's node offset,
the rings and need_min.  The host entry point is pinned against a walk in Python by test_unitig_chains_host.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sparrowhawk_amd import _lib
from unitig_chains_cases import N_RANDOM, Builder, chains_text, random_case, refused_cases

pytestmark = pytest.mark.gpu


def both(case):
    """device text == host text; returns it"""
    L = _lib.load()
    host = chains_text(L, "shk_host_unitig_chains", case)
    dev = chains_text(L, "shk_device_unitig_chains", case)
    assert host is not None and dev is not None
    if dev != host:
        h, d = host.split("\n"), dev.split("\n")
        at = next((i for i in range(min(len(h), len(d))) if h[i] != d[i]), min(len(h), len(d)))
        raise AssertionError("line %d of %d / %d differs\ndevice: %.300s\nhost:   %.300s" % (at, len(d), len(h), "\n".join(d[at:at + 2]), "\n".join(h[at:at + 2])))
    assert not host.startswith("error:"), host
    return host


def lines_of(text):
    body = text.split("\n")[:-2]
    return [x for x in body if x.startswith("0 ")], [x for x in body if x.startswith("1 ")]


@pytest.mark.parametrize("block", range(6))
def test_random_cases(block):
    assert block * 50 + 50 <= N_RANDOM
    for i in range(block * 50, block * 50 + 50):
        both(random_case(i))


def test_no_records():
    assert both(Builder(31, 1).build()) == "need_min :\n"


def test_one_record_that_is_its_own_mirror():
    B = Builder(31, 2)
    B.self_chain(1)
    assert both(B.build(ln=40, kc=400)) == "0 40 400 0 : 0@0\nneed_min :\n"


def test_one_unitig_on_both_strands():
    B = Builder(31, 3)
    B.chain_pair(1)
    lin, rings = lines_of(both(B.build(ln=50, kc=500)))
    assert len(lin) == 1 and not rings and lin[0].startswith("0 50 500 0 : ")


@pytest.mark.parametrize("L", [1, 2, 3, 63, 64, 65, 255, 256, 257])
def test_chain_lengths(L):
    """a chain on both strands and one that is its own mirror strand, around the widths of a wave and of a workgroup and
    around the powers of two at which the jumping needs one round more"""
    B = Builder(63, 10 + L)
    B.chain_pair(L); B.self_chain(L); B.chain_pair(1)
    lin, rings = lines_of(both(B.build()))
    assert sorted(len(x.split(":")[1].split()) for x in lin) == sorted([L, L, 1]) and not rings


def test_a_chain_of_100000_records_with_its_mirror():
    """200 000 records: more than the 131 072 threads of the largest launch, 17 jumping rounds"""
    B = Builder(31, 4)
    B.chain_pair(100000)
    lin, rings = lines_of(both(B.build()))
    assert len(lin) == 1 and not rings and len(lin[0].split(":")[1].split()) == 100000


@pytest.mark.parametrize("L", [2, 3, 64, 1000])
def test_rings(L):
    """a ring with its mirror ring and a ring that is its own mirror, beside chains (a ring of 2, 64 records: after 1, 6
    rounds every record of it is its own ancestor)"""
    B = Builder(127, 20 + L)
    B.chain_pair(5); B.ring_pair(L); B.self_ring(L); B.circ_record(); B.chain_pair(70); B.circ_record(0)
    lin, rings = lines_of(both(B.build()))
    assert len(lin) == 2 and sorted(len(x.split(":")[1].split()) for x in rings) == sorted([1, L, L])


def test_rings_only():
    B = Builder(31, 5)
    for L in (1, 2, 4, 7, 300):
        B.ring_pair(L); B.self_ring(L)
    B.circ_record(); B.circ_record()
    lin, rings = lines_of(both(B.build()))
    assert not lin and len(rings) == 12


def test_50000_single_record_contigs():
    B = Builder(31, 6)
    for _ in range(50000):
        B.chain_pair(1)
    lin, rings = lines_of(both(B.build()))
    assert len(lin) == 50000 and not rings


@pytest.mark.parametrize("k", [63, 127, 255])
@pytest.mark.parametrize("word", ["highest", "lowest"])
def test_first_kmers_that_differ_in_one_word(k, word):
    """W = 2, 4, 8: the strand choice compares all words, most significant first"""
    W = (2 * k + 63) // 64
    B = Builder(k, 30 + k)
    for L in (1, 2, 5, 1, 3, 1, 1, 4):
        B.chain_pair(L)
    c = B.build(vary=W - 1 if word == "highest" else 0)
    assert len({tuple(r) for r in np.delete(c.first, W - 1 if word == "highest" else 0, axis=1)}) == 1
    lin, rings = lines_of(both(c))
    assert len(lin) == 8 and not rings


def test_offsets_beyond_32_bits():
    """2^31 nodes per record: node offsets from the third record of a chain on, and text offsets from the third contig on, pass 2^32"""
    B = Builder(31, 7)
    for L in (4, 1, 6, 2):
        B.chain_pair(L)
    lin, _rings = lines_of(both(B.build(ln=1 << 31)))
    assert max(int(x.split()[3]) for x in lin) > 1 << 32
    assert max(int(rec.split("@")[1]) for x in lin for rec in x.split(":")[1].split()) > 1 << 32


def test_counts_beyond_62_bits():
    B = Builder(31, 8)
    B.chain_pair(2)
    lin, _rings = lines_of(both(B.build(kc=1 << 62)))
    assert len(lin) == 1 and int(lin[0].split()[2]) == 1 << 63


def test_refused_input_is_refused_in_the_host_entry_points_words():
    L = _lib.load()
    for name, case, message in refused_cases():
        assert chains_text(L, "shk_device_unitig_chains", case) == message, name
        assert chains_text(L, "shk_host_unitig_chains", case) == message, name
    B = Builder(31, 9)
    B.chain_pair(3)
    both(B.build())                                            # the device is as usable as before


def test_hand_built_graphs_with_the_chains_walked_on_the_host(monkeypatch):
    """SHK_UNITIG_CHAINS_DEVICE=0: the device twin of the whole stage hands alive / mirror / succ home and the host walks,
    as it did before the walk had kernels of its own — three of the hand-built graphs of test_gpu_unitig_graph.py"""
    import test_gpu_unitig_graph as T
    monkeypatch.setenv("SHK_UNITIG_CHAINS_DEVICE", "0")
    T.case_three_tips(31, "any")
    T.case_bubble_at_the_limit(63, "hi")
    T.test_a_ring_of_several_records_that_forms_after_a_removal()
