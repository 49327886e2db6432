"""The end keys of the device text writer, in the code the kernels share with the host (csrc/end_keys.h, through
shk_host_end_key; no GPU): the packing must be the host writer's pack / pack_rc (outputs.cpp) — the k-mer as a 2k-bit number,
its first base in the top 2 bits, and the same of the reverse complement — and of two table words with one key the host's
choice must win: '+' before '-', then the smaller sorted position."""
import numpy as np
import pytest

from util import int_to_words, kmer_int, revcomp

KS = (15, 31, 33, 63, 65, 255)


def _end_key(lib, seq, k, rc, o=0, pos=0):
    import ctypes as C
    W = (2 * k + 63) // 64
    words = np.zeros(8, dtype=np.uint64)
    entry = C.c_uint64(0)
    assert lib.shk_host_end_key(seq.encode(), k, rc, o, pos, words.ctypes.data, C.byref(entry)) == 0
    assert not words[W:].any()
    return tuple(int(w) for w in words[:W]), entry.value


@pytest.mark.parametrize("k", KS)
def test_end_key_packing_is_the_host_writers(lib, k):
    rng = np.random.default_rng(k)
    W = (2 * k + 63) // 64
    texts = ["A" * k, "T" * k, "C" * k, "A" * (k - 1) + "T", "G" + "A" * (k - 1)]
    texts += ["".join("ACGT"[c] for c in rng.integers(0, 4, k)) for _ in range(40)]
    for s in texts:
        fwd, _ = _end_key(lib, s + "ACGT", k, 0)             # (only the first k bases are read)
        rc, _ = _end_key(lib, s + "ACGT", k, 1)
        assert fwd == int_to_words(kmer_int(s), W), s        # pack: sum of code(p[i]) << 2 (k - 1 - i)
        assert rc == int_to_words(kmer_int(revcomp(s)), W), s   # pack_rc: sum of (3 - code(p[i])) << 2 i
        assert rc == _end_key(lib, revcomp(s), k, 0)[0]


@pytest.mark.parametrize("k", KS)
def test_end_key_table_word_and_tie_rule(lib, k):
    rng = np.random.default_rng(100 + k)
    s = "".join("ACGT"[c] for c in rng.integers(0, 4, k))
    words = {}
    for o in (0, 1):
        for pos in (0, 1, 7, 19999, 2**31 - 1):
            _, e = _end_key(lib, s, k, 0, o, pos)
            assert e != 2**64 - 1                              # all ones is an empty slot
            assert e & 0x7FFFFFFF == pos and (e >> 31) & 1 == o
            words[(o, pos)] = e
    assert len({e >> 32 for e in words.values()}) == 1          # one key, one fingerprint
    # the smallest word is the smallest (orientation, position): '+' before '-', then the smaller contig
    assert sorted(words, key=lambda t: words[t]) == sorted(words)
    # the same key reached as a reverse complement carries the same fingerprint
    _, e = _end_key(lib, revcomp(s), k, 1, 1, 3)
    assert e >> 32 == words[(0, 0)] >> 32


def test_end_key_refuses_bad_parameters(lib):
    import ctypes as C
    words = np.zeros(8, dtype=np.uint64)
    assert lib.shk_host_end_key(b"ACGT", 0, 0, 0, 0, words.ctypes.data, None) != 0
    assert lib.shk_host_end_key(b"ACGT" * 70, 256, 0, 0, 0, words.ctypes.data, None) != 0
    assert lib.shk_host_end_key(b"ACGT", 3, 0, 2, 0, words.ctypes.data, None) != 0
    assert lib.shk_host_end_key(b"ACGT", 3, 0, 0, 2**31, words.ctypes.data, None) != 0
