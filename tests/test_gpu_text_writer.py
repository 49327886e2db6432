"""The device writer from contig text alone (csrc/writer_text_gpu.h) through its stand-alone entry point:
shk_device_assembly_json must give the bytes of its host twin shk_host_assembly_json — strand choice and reverse complement
in place, order with its ties, links from the table of end k-mers with the host's tie rule, records and sequences."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from util import make_dataset, revcomp, run_oracle

pytestmark = pytest.mark.gpu

EMPTY = '{"outfasta":"","ncontigs":0,"outdot":"digraph sparrowhawk {\\n}\\n","outgfa":"H\\tVN:Z:1.0\\n","outgfav2":"H\\tVN:Z:2.0\\n"}'


def _arrays(contigs):
    seqs = "".join(s for s, _ in contigs).encode()
    off = np.zeros(len(contigs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s, _ in contigs])
    kc = np.array([c for _, c in contigs], dtype=np.uint64)
    return seqs, off, kc


def _take(lib, p):
    if not p:
        return None
    try:
        return C.string_at(p).decode()
    finally:
        lib.shk_host_free(p)


def _host_raw(lib, seqs, off, kc, n, k):
    return _take(lib, lib.shk_host_assembly_json(seqs, off.ctypes.data, kc.ctypes.data, n, k))


def _device_raw(lib, seqs, off, kc, n, k):
    why = C.c_char_p()
    out = _take(lib, lib.shk_device_assembly_json(seqs, off.ctypes.data, kc.ctypes.data, n, k, C.byref(why)))
    return out, (why.value or b"").decode()


def _both(lib, contigs, k):
    """the two twins on one input: (host JSON, device JSON)"""
    seqs, off, kc = _arrays(contigs)
    host = _host_raw(lib, seqs, off, kc, len(contigs), k)
    dev, why = _device_raw(lib, seqs, off, kc, len(contigs), k)
    assert host is not None
    assert dev is not None, why
    return host, dev


@pytest.mark.parametrize("k,err", [(31, 0.01), (51, 0.02), (21, 0.03), (161, 0.004), (255, 0.003)])
def test_device_text_writer_equals_the_oracle_writer(lib, k, err):
    """the cases of test_output_writer_equals_the_oracle_writer: the oracle's unitigs (errors left in, tips and bubbles kept)
    on a random strand in a random order; k = 161 and 255 use six- and eight-word end keys"""
    g, fq = make_dataset(30000, 14, read_len=150 if k < 128 else 400, err=err, seed=900 + k)
    o = run_oracle([fq], k=k, min_count=1, min_qual=0, no_bubble_collapse=True, no_dead_end_removal=True)
    o.assemble()
    cs, kcs = o.contigs(), o.contig_kc()
    assert len(cs) > 20
    rng = np.random.default_rng(k)
    items = []
    for i in rng.permutation(len(cs)):
        items.append((revcomp(cs[i]) if rng.integers(0, 2) else cs[i], kcs[i]))
    host, dev = _both(lib, items, k)
    assert dev == host
    assert dev == o.assembly_json()


def _rs(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, n))


def _hand_made():
    """name -> (contigs, k); every sequence is random but for the property its name says"""
    rng = np.random.default_rng(20261)
    kc = lambda: int(rng.integers(1, 100000))
    cases = {}
    cases["one contig"] = ([(_rs(rng, 40), 7)], 31)
    for k in (15, 31):
        cases["one node each, k=%d" % k] = ([(_rs(rng, k), kc()) for _ in range(3)], k)       # (k = 15: shorter than the 16-base sort prefix)
        cases["lengths k .. k+17, k=%d" % k] = ([(_rs(rng, k + d), kc()) for d in range(18)], k)     # every phase of the 8-byte pieces
    x = _rs(rng, 20)
    cases["its own reverse complement"] = ([(_rs(rng, 33), kc()), (x + revcomp(x), kc()), (_rs(rng, 47), kc())], 31)
    # the strand is open until the middle base (odd length: it always differs from its complement) — in the second
    # 64-position step of the wave (141 bases: position 70), and in the first (71 bases: position 35)
    mid = []
    for m in "ACGT":
        x = _rs(rng, 70); mid.append((x + m + revcomp(x), kc()))
        x = _rs(rng, 35); mid.append((x + m + revcomp(x), kc()))
    cases["decided at the middle position"] = (mid, 31)
    # even length: open until the last compared position n/2 - 1 — the last lane of a step (128 bases), the first lane of
    # the next (130), and inside one (40)
    last = []
    for n in (128, 130, 40):
        for y in ("AA", "TT", "CA", "TG"):
            x = _rs(rng, n // 2 - 1); last.append((x + y + revcomp(x), kc()))
    cases["decided at the last compared position"] = (last, 31)
    # ties of the sort: equal length, equal first 16 / first 32 bases, the last base differs.  ('A' in front and no 'T'
    # behind: each is the smaller strand as given, so they still agree after the strand choice)
    p16, p32 = "A" + _rs(rng, 17), "A" + _rs(rng, 39)
    t = [(p16 + _rs(rng, 22) + b, kc()) for b in "GC"]                                           # agree in 18, differ from there
    t += [(p32 + b, kc()) for b in "GAC"]                                                         # three that agree in 40 of 41
    q = "A" + _rs(rng, 35)
    t += [(q + b, kc()) for b in "CA"] + [(_rs(rng, 41), kc())]
    cases["ties settled by full comparison"] = (t, 31)
    k = 31
    u = _rs(rng, k - 1)
    cases["linked to itself"] = ([(u + _rs(rng, 25) + u, kc()), (_rs(rng, 50), kc())], k)
    w = _rs(rng, (k - 1) // 2)
    cases["hairpin"] = ([(_rs(rng, 30) + "C" + w + revcomp(w), kc()), (_rs(rng, 44), kc())], k)
    ov = _rs(rng, k - 1)
    cases["a link and its mirror"] = ([(_rs(rng, 20) + ov, kc()), (ov + _rs(rng, 33), kc())], k)
    ov = _rs(rng, k - 1)
    cases["four links from one end"] = ([(_rs(rng, 25) + ov, kc())] + [(ov + b + _rs(rng, 10 + i), kc()) for i, b in enumerate("ACGT")], k)
    f = _rs(rng, k)
    cases["one first k-mer, two lengths"] = ([(f + _rs(rng, 10), kc()), (f + _rs(rng, 25), kc()), (_rs(rng, 20) + f[:k - 1], kc())], k)
    f = _rs(rng, k)
    cases["one first k-mer, '+' and '-'"] = ([(_rs(rng, 30) + revcomp(f), kc()), (f + _rs(rng, 12), kc()), (_rs(rng, 20) + f[:k - 1], kc())], k)
    return cases


_HAND = _hand_made()


@pytest.mark.parametrize("name", sorted(_HAND))
def test_device_text_writer_hand_made_texts(lib, name):
    contigs, k = _HAND[name]
    rng = np.random.default_rng(len(name))
    for flip_all in (False, True, None):                       # as given, every contig turned, a random strand each
        items = [(revcomp(s) if (flip_all or (flip_all is None and rng.integers(0, 2))) else s, c) for s, c in contigs]
        host, dev = _both(lib, items, k)
        assert dev == host, (name, flip_all)
    if "link" in name or "hairpin" in name or "first k-mer" in name:
        assert "\\nL\\t" in host, name                         # (the case does have a link)


def test_device_text_writer_no_contig(lib):
    seqs, off, kc = _arrays([])
    dev, why = _device_raw(lib, seqs, off, kc, 0, 31)
    assert dev == EMPTY and dev == _host_raw(lib, seqs, off, kc, 0, 31)


def test_device_text_writer_beyond_one_block_and_one_sort_tile(lib):
    """20 000 contigs of 40-60 bases at k = 31: a 1 Mbp random genome chopped at random points, 300 of the cuts with k - 1
    bases of overlap (those pieces are linked), every piece on a random strand"""
    rng = np.random.default_rng(77)
    k, n = 31, 20000
    lens = rng.integers(40, 61, n)
    genome = _rs(rng, int(lens.sum()))
    overlap = np.zeros(n, dtype=bool); overlap[rng.choice(np.arange(1, n), 300, replace=False)] = True
    flips = rng.integers(0, 2, n)
    items, at = [], 0
    for i in range(n):
        a = at - (k - 1) if overlap[i] else at
        s = genome[a:at + int(lens[i])]
        at += int(lens[i])
        items.append((revcomp(s) if flips[i] else s, int(rng.integers(1, 5000))))
    order = rng.permutation(n)
    items = [items[i] for i in order]
    host, dev = _both(lib, items, k)
    assert host.count("\\nL\\t") >= 300
    assert dev == host


def test_device_text_writer_refuses_what_the_host_twin_refuses(lib):
    rng = np.random.default_rng(5)
    k = 31
    seqs = _rs(rng, 200).encode()
    kc = np.array([3, 4, 5], dtype=np.uint64)
    for off in ([0, 80, 60, 200],            # not ascending
                [0, 40, 70, 200],            # a contig of 30 bases, shorter than k
                [0, 40, 40, 200]):           # an empty contig
        off = np.array(off, dtype=np.uint64)
        host = _host_raw(lib, seqs, off, kc, 3, k)
        dev, why = _device_raw(lib, seqs, off, kc, 3, k)
        assert host is None
        assert dev is None and why, off
    off = np.array([0, 40, 100, 200], dtype=np.uint64)      # (and the same call with good offsets is served)
    dev, why = _device_raw(lib, seqs, off, kc, 3, k)
    assert dev is not None and dev == _host_raw(lib, seqs, off, kc, 3, k), why
