"""The BGZF block encoder on the host (SPEC S11a; csrc/deflate_write.h through shk_host_deflate_lengths and
shk_host_bgzf_compress): the code lengths against a Huffman tree built here, and the files against gzip, zlib and the
library's own reader.  No GPU.  tests/test_gpu_bgzf_write.py holds the device twin to these files byte for byte."""
import ctypes as C
import gzip
import heapq

import numpy as np
import pytest

from bgzf_write_cases import BLOCK, EOF_MARKER, STORED_CASES, catalogue, check_file, fibonacci_counts, histogram, lucas_counts


def lengths(lib, counts):
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    assert counts.shape == (257,)
    out = np.zeros(257, dtype=np.uint8)
    rc = lib.shk_host_deflate_lengths(counts.ctypes.data, out.ctypes.data)
    assert rc == 0, rc
    return out


def huffman(counts):
    """(cost in bits, depth) of Huffman's tree over the used symbols, built here: a heap of (weight, leaf before inner node,
    order of making)"""
    used = [int(c) for c in counts if c]
    if len(used) == 1:
        return used[0], 1
    heap = [(c, 0, i, 0) for i, c in enumerate(used)]         # (weight, inner, serial, depth of the subtree)
    heapq.heapify(heap)
    cost, serial = 0, len(used)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        cost += a[0] + b[0]
        heapq.heappush(heap, (a[0] + b[0], 1, serial, max(a[3], b[3]) + 1))
        serial += 1
    return cost, heap[0][3]


def kraft(lens):
    return sum(1 << (15 - int(l)) for l in lens if l)


def check_lengths(lib, counts, what):
    lens = lengths(lib, counts)
    used = counts > 0
    assert lens.max() <= 15 and (lens[~used] == 0).all() and (lens[used] > 0).all(), what
    assert kraft(lens) == 1 << 15, (what, "the code is not complete")
    cost = int((counts.astype(np.int64) * lens).sum())
    best, depth = huffman(counts)
    if depth <= 15:
        assert cost == best, (what, cost, best)
    else:
        assert cost > best, (what, cost, best)
    return cost, best, depth


def random_histograms(n, seed=2024):
    rng = np.random.default_rng(seed)
    for i in range(n):
        used = 1 if i % 20 == 0 else (2 if i % 20 == 1 else int(rng.integers(1, 257)))      # literals in use; end-of-block comes on top
        c = np.zeros(257, dtype=np.uint32)
        which = rng.permutation(256)[:used]
        kind = i % 4
        if kind == 0:
            c[which] = rng.integers(1, 300, used)
        elif kind == 1:
            c[which] = np.minimum(rng.geometric(0.002, used), 60000)
        elif kind == 2:
            c[which] = np.maximum(1, (65280 * rng.dirichlet(np.full(used, 0.05))).astype(np.int64))      # a few values hold nearly all
        else:
            c[which] = 7                                                                  # ties everywhere
        c[256] = 1
        yield i, c


def test_code_lengths_are_complete_and_cost_what_huffman_costs(lib):
    """Every length at most 15, unused symbols 0, Kraft sum exactly 1; where Huffman's own tree is at most 15 deep the cost is
    its cost, and where it is deeper the cost is above it.
    The Fibonacci histogram (22 counts 1, 1, 2 ... F22 and end-of-block): measured, printed below.  With the tie rule of SPEC
    S11a (a leaf before an inner node of the same weight) Huffman's tree over these 23 counts is 12 deep, not 22 — end-of-block
    is a third count of 1, every later step finds a leaf and an inner node of one weight, and taking the leaf first grows two
    combs side by side.  So the limiter is not needed there: Huffman 121 390 bits, the library 121 390 bits, margin 0; nothing
    is asserted of it beyond "complete and at most 15".
    The Lucas histogram (lucas_counts: every count above the sum the tree has joined so far) is 22 deep under ANY tie rule and
    does need the limiter: measured Huffman 167 735 bits, limited to 15 bits 167 869, margin 134 bits (0.08 %)."""
    deep = 0
    for name, text in catalogue():
        for at in range(0, len(text), BLOCK):
            _, _, depth = check_lengths(lib, histogram(text[at:at + BLOCK]), (name, at))
            deep += depth > 15
    for i, c in random_histograms(200):
        _, _, depth = check_lengths(lib, c, ("random histogram", i))
        deep += depth > 15
    for what, counts in (("fibonacci", fibonacci_counts()), ("lucas", lucas_counts())):
        h = np.zeros(257, dtype=np.uint32)
        h[40:40 + len(counts)] = counts
        h[256] = 1
        cost, best, depth = check_lengths(lib, h, what)
        print(what + ": Huffman", best, "bits at depth", depth, "- the library:", cost, "bits, margin", cost - best)
        if what == "lucas":
            assert depth > 15 and cost > best
    powers = np.zeros(257, dtype=np.uint32)                   # 1, 1, 3, 9 ... 3^19: 21 deep whatever the ties, beyond any block's counts
    powers[100:120] = [3 ** i for i in range(20)]
    powers[256] = 1
    _, _, depth = check_lengths(lib, powers, "powers of three")
    assert depth == 20 and deep >= 1


def test_code_lengths_of_the_plain_histograms(lib):
    one = np.zeros(257, dtype=np.uint32)
    one[ord("G")], one[256] = BLOCK, 1
    lens = lengths(lib, one)
    assert lens[ord("G")] == 1 and lens[256] == 1 and lens.sum() == 2           # one byte value: two symbols of length 1
    flat = np.full(257, 255, dtype=np.uint32)
    flat[256] = 1
    lens = lengths(lib, flat)
    assert sorted(lens) == [8] * 255 + [9] * 2 and lens[256] == 9 and lens[0] == 9      # the tie rule: the lower symbol is the rarer
    assert lib.shk_host_deflate_lengths(np.zeros(257, dtype=np.uint32).ctypes.data, lens.ctypes.data) == -1


def host_file(lib, text):
    out, n = C.c_void_p(), C.c_size_t()
    rc = lib.shk_host_bgzf_compress(text, len(text), C.byref(out), C.byref(n))
    assert rc == 0, rc
    try:
        return C.string_at(out.value, n.value)
    finally:
        lib.shk_host_free(out)


@pytest.mark.parametrize("name", [name for name, _ in catalogue()])
def test_host_files(lib, name):
    text = dict(catalogue())[name]
    data = host_file(lib, text)
    blocks = check_file(data, text)
    if name in STORED_CASES:
        assert all(b["btype"] == 0 for b in blocks)
    if name == "three_blocks":
        assert [b["btype"] for b in blocks] == [2, 0, 2] and len(data) > 65536
    if name.startswith(("acgt", "golden", "fibonacci", "lucas", "one_value")):
        assert all(b["btype"] == 2 for b in blocks if b["isize"] >= 256)            # (a block of a few bytes is smaller stored: the header)
    if name == "empty":
        assert data == EOF_MARKER
    assert data == host_file(lib, text)                                          # the bytes are deterministic
    # the library's own reader
    out, n = C.c_void_p(), C.c_size_t()
    assert lib.shk_host_gunzip(data, len(data), C.byref(out), C.byref(n), None, None) == 0
    try:
        assert C.string_at(out.value, n.value) == text
    finally:
        lib.shk_host_free(out)
    if name.startswith("acgt"):
        print(name, "bits per byte of text:", round(8 * len(data) / len(text), 3), "gzip -6:", round(8 * len(gzip.compress(text, 6)) / len(text), 3))
