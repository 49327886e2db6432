"""Settled arrays for the S10 walk alone (shk_host_unitig_chains / shk_device_unitig_chains): a builder of chains and rings
with their mirror strands, the 300 random cases both test files run, and the inputs the entry points refuse.  Nothing here
walks a chain: the walk the library is pinned against is written in test_unitig_chains_host.py."""
import ctypes as C

import numpy as np

NIL = 0xFFFFFFFF
KS = (31, 63, 127, 255)


class Case:
    """The arrays of one call.  first: [n][W] words, w[0] least significant."""

    def __init__(self, k, first, ln, kc, circ, alive, mirror, succ):
        self.k, self.W, self.n = k, (2 * k + 63) // 64, len(ln)
        self.first = np.ascontiguousarray(first, dtype=np.uint64).reshape(self.n, self.W)
        self.len = np.ascontiguousarray(ln, dtype=np.uint64)
        self.kc = np.ascontiguousarray(kc, dtype=np.uint64)
        self.circ = np.ascontiguousarray(circ, dtype=np.uint8)
        self.alive = np.ascontiguousarray(alive, dtype=np.uint8)
        self.mirror = np.ascontiguousarray(mirror, dtype=np.uint32)
        self.succ = np.ascontiguousarray(succ, dtype=np.uint32)

    def args(self):
        return (self.k, self.n, self.first.ctypes.data, self.len.ctypes.data, self.kc.ctypes.data, self.circ.ctypes.data,
                self.alive.ctypes.data, self.mirror.ctypes.data, self.succ.ctypes.data)

    def copy(self):
        return Case(self.k, self.first.copy(), self.len.copy(), self.kc.copy(), self.circ.copy(), self.alive.copy(),
                    self.mirror.copy(), self.succ.copy())


def chains_text(L, name, case):
    """the text of one entry point, or None where it returns NULL"""
    ptr = getattr(L, name)(*case.args())
    if not ptr:
        return None
    text = C.string_at(ptr).decode()
    L.shk_host_free(ptr)
    return text


def random_firsts(rng, n, k, vary=None):
    """n distinct k-mers as [n][W] words; vary = w: they differ in word w only"""
    W = (2 * k + 63) // 64
    top = 2 * k - 64 * (W - 1)
    while True:
        f = rng.integers(0, 1 << 63, (n, W), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (n, W), dtype=np.uint64)
        if vary is not None:
            keep = f[:, vary].copy()
            f[:] = f[0]
            f[:, vary] = keep
        if top < 64:
            f[:, W - 1] &= np.uint64((1 << top) - 1)
        if len(np.unique(f, axis=0)) == n:
            return f


class Builder:
    """Records by local number, renumbered by a random permutation in build(): succ then jumps across workgroups."""

    def __init__(self, k, seed):
        self.k, self.rng = k, np.random.default_rng(seed)
        self.alive, self.circ, self.succ, self.mirror = [], [], [], []

    def _new(self, count, alive=1, circ=0):
        base = len(self.alive)
        self.alive += [alive] * count; self.circ += [circ] * count
        self.succ += [NIL] * count; self.mirror += [NIL] * count
        return list(range(base, base + count))

    def _link(self, a, b, ring):
        L = len(a)
        for i in range(L):                                   # mirror[a_i] = b_(L+1-i), 1-based
            self.mirror[a[i]] = b[L - 1 - i]
            self.mirror[b[L - 1 - i]] = a[i]
        for s in {id(a): a, id(b): b}.values():
            for i in range(L - 1):
                self.succ[s[i]] = s[i + 1]
            if ring:
                self.succ[s[L - 1]] = s[0]

    def chain_pair(self, L):                                 # one unitig chain on both strands
        a, b = self._new(L), self._new(L)
        self._link(a, b, False)
        return a, b

    def self_chain(self, L):                                 # a chain that is its own mirror strand
        a = self._new(L)
        self._link(a, a, False)
        return a

    def ring_pair(self, L):
        a, b = self._new(L), self._new(L)
        self._link(a, b, True)
        return a, b

    def self_ring(self, L):
        a = self._new(L)
        self._link(a, a, True)
        return a

    def circ_record(self, alive=1):
        return self._new(1, alive, 1)

    def dead_pair(self):                                     # a removed unitig: both strands dead, no links left
        a, b = self._new(1, 0), self._new(1, 0)
        self.mirror[a[0]], self.mirror[b[0]] = b[0], a[0]

    def build(self, shuffle=True, ln=None, kc=None, vary=None):
        n = len(self.alive)
        perm = self.rng.permutation(n) if shuffle else np.arange(n)
        succ = np.full(n, NIL, dtype=np.uint32); mirror = np.full(n, NIL, dtype=np.uint32)
        alive = np.zeros(n, dtype=np.uint8); circ = np.zeros(n, dtype=np.uint8)
        for r in range(n):
            alive[perm[r]], circ[perm[r]] = self.alive[r], self.circ[r]
            if self.succ[r] != NIL:
                succ[perm[r]] = perm[self.succ[r]]
            if self.mirror[r] != NIL:
                mirror[perm[r]] = perm[self.mirror[r]]
        first = random_firsts(self.rng, n, self.k, vary) if n else np.zeros((0, (2 * self.k + 63) // 64), dtype=np.uint64)
        ln = self.rng.integers(1, 3000, n, dtype=np.uint64) if ln is None else np.full(n, ln, dtype=np.uint64)
        kc = self.rng.integers(1, 1 << 40, n, dtype=np.uint64) if kc is None else np.full(n, kc, dtype=np.uint64)
        self.perm = perm
        return Case(self.k, first, ln, kc, circ, alive, mirror, succ)


def random_case(i):
    """case i of the 300: a mixture of everything the builder makes, a few hundred records at the most"""
    rng = np.random.default_rng(91000 + i)
    B = Builder(KS[i % 4], 92000 + i)
    lengths = (1, 1, 1, 2, 2, 3, 4, 5, 7, 8, 9, 16, 17, 31, 33, 64, 65, 70)
    for _ in range(int(rng.integers(1, 9))):
        what = int(rng.integers(0, 8))
        L = int(rng.choice(lengths))
        if what <= 1:
            B.chain_pair(L)
        elif what == 2:
            B.self_chain(L)                                  # (L odd: the middle record is its own mirror)
        elif what == 3:
            B.ring_pair(L)
        elif what == 4:
            B.self_ring(L)
        elif what == 5:
            B.circ_record(int(rng.integers(0, 2)))
        elif what == 6:
            B.dead_pair()
        else:
            for _j in range(int(rng.integers(1, 40))):
                B.chain_pair(1)
    return B.build()


N_RANDOM = 300


def refused_cases():
    """(name, case, the line both entry points answer): one per rule of unitig_chains_check"""
    out = []

    def base():
        B = Builder(31, 5)
        a, b = B.chain_pair(3)
        c = B.circ_record()
        B.dead_pair()                                        # records 7 and 8
        return B.build(shuffle=False), a, b, c[0]
    case, a, b, c = base()
    case.succ[a[2]] = 7                                      # a dead record as successor
    out.append(("successor_dead", case, "a successor that is no alive linear record"))
    case, a, b, c = base()
    case.succ[a[2]] = c
    out.append(("successor_circ", case, "a successor that is no alive linear record"))
    case, a, b, c = base()
    case.succ[a[2]] = 1000
    out.append(("successor_out_of_range", case, "a successor that is no alive linear record"))
    case, a, b, c = base()
    case.succ[a[2]] = a[1]
    out.append(("shared_successor", case, "two records share a successor"))
    case, a, b, c = base()
    case.mirror[a[0]] = b[0]                                 # b[0]'s mirror is a[2]
    out.append(("mirror_unpaired", case, "mirror strands do not pair up"))
    case, a, b, c = base()
    case.mirror[a[1]] = 8                                    # a dead record as mirror strand
    out.append(("mirror_dead", case, "mirror strands do not pair up"))
    case, a, b, c = base()
    case.succ[b[0]] = NIL                                    # a[1] -> a[2] stays, its mirror link b[0] -> b[1] is gone
    out.append(("mirror_link_missing", case, "a link without its mirror link"))
    case, a, b, c = base()
    case.succ[7] = a[0]
    out.append(("dead_with_successor", case, "a dead or circular record with a successor"))
    case, a, b, c = base()
    case.succ[c] = a[0]
    out.append(("circ_with_successor", case, "a dead or circular record with a successor"))
    return [(name, cs, "error: unitig chains: " + msg) for name, cs, msg in out]
