"""A bit-level DEFLATE writer for tests only, written from RFC 1951 (deflate), RFC 1952 (gzip) and the SAM specification
4.1 (BGZF).  It writes what a caller asks for, token by token and code length by code length — also streams no encoder
writes and streams that are not legal; zlib's inflater is the judge of both (tests/test_deflate_streams.py).

Tokens:  an int 0..255                         a literal
         (length, distance)                    a match, coded with the symbols RFC 1951 3.2.5 gives
         ("L", lsym, lextra, dsym, dextra)     a match by its symbols and extra-bit values as they stand (no checks)
         ("S", sym)                            the literal/length symbol `sym` by its code, nothing behind it (no checks)
Bits are packed LSB first; a block is a Python int and its bit count, blocks are joined by shift / or (Stream)."""
import heapq
import struct
import zlib

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT_LENS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST_LENS = [5] * 32                                        # (30 and 31 have codes and no meaning)


def len_symbol(length):
    """(symbol, extra bits, extra value) of a match length 3..258; 258 is symbol 285"""
    if length == 258:
        return 285, 0, 0
    for c in range(27, -1, -1):
        if length >= LEN_BASE[c]:
            return 257 + c, LEN_EXTRA[c], length - LEN_BASE[c]
    raise ValueError(length)


def dist_symbol(distance):
    for c in range(29, -1, -1):
        if distance >= DIST_BASE[c]:
            return c, DIST_EXTRA[c], distance - DIST_BASE[c]
    raise ValueError(distance)


def token_match(t):
    """(length, distance) of a match token; None for the others"""
    if isinstance(t, int) or t[0] == "S":
        return None
    if t[0] == "L":
        return LEN_BASE[t[1] - 257] + t[2], DIST_BASE[t[3]] + t[4]
    return t


def expand(tokens, history=b""):
    """the bytes the tokens stand for, behind `history`"""
    out = bytearray(history)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
            continue
        length, dist = token_match(t)
        if dist > len(out):
            raise ValueError("distance %d with %d bytes so far" % (dist, len(out)))
        start = len(out) - dist
        if dist >= length:
            out += out[start:start + length]
        else:
            out += (bytes(out[start:]) * (length // dist + 1))[:length]
    return bytes(out[len(history):])


def reach(tokens):
    """how many bytes of history the tokens need in front of them"""
    need, pos = 0, 0
    for t in tokens:
        m = token_match(t)
        if isinstance(t, int):
            pos += 1
        elif m:
            need = max(need, m[1] - pos)
            pos += m[0]
    return need


def tokenize(text, history=b"", min_match=4, max_dist=32768, max_len=258):
    """a plain greedy LZ77 parse (last occurrence of the next three bytes): tokens whose expansion behind `history` is `text`"""
    buf = bytes(history) + bytes(text)
    h = len(history)
    last = {}
    for i in range(max(0, h - max_dist), h):
        last[buf[i:i + 3]] = i
    toks, i, n = [], h, len(buf)
    while i < n:
        key = buf[i:i + 3]
        j = last.get(key)
        length = 0
        if j is not None and len(key) == 3 and i - j <= max_dist:
            while length < max_len and i + length < n and buf[j + length] == buf[i + length]:
                length += 1
        if length >= min_match:
            toks.append((length, i - j))
            for q in range(i, i + length):
                last[buf[q:q + 3]] = q
            i += length
        else:
            last[key] = i
            toks.append(buf[i])
            i += 1
    return toks


def symbol_freqs(tokens):
    """(literal/length frequencies[288], distance frequencies[32]) of a token list, end-of-block counted once"""
    lit, dist = [0] * 288, [0] * 32
    for t in tokens:
        if isinstance(t, int):
            lit[t] += 1
        elif t[0] == "S":
            lit[t[1]] += 1
        elif t[0] == "L":
            lit[t[1]] += 1
            dist[t[3]] += 1
        else:
            lit[len_symbol(t[0])[0]] += 1
            dist[dist_symbol(t[1])[0]] += 1
    lit[256] += 1
    return lit, dist


# ---- code lengths ------------------------------------------------------------------------------------------------------
def kraft(lens, maxlen=15):
    """the Kraft sum of a length set in units of 2^-maxlen (2^maxlen: complete)"""
    return sum(1 << (maxlen - l) for l in lens if l)


def huffman_lengths(freqs, maxlen=15):
    """a complete code for the symbols with a frequency, no code longer than maxlen (Huffman's, then shortened where it is
    too deep); one symbol alone gets length 1"""
    syms = [s for s, f in enumerate(freqs) if f > 0]
    lens = [0] * len(freqs)
    if not syms:
        return lens
    if len(syms) == 1:
        lens[syms[0]] = 1
        return lens
    if len(syms) > (1 << maxlen):
        raise ValueError("too many symbols for %d bits" % maxlen)
    heap = [(freqs[s], s, (s,)) for s in syms]
    heapq.heapify(heap)
    tie = len(freqs)
    while len(heap) > 1:
        fa, _, a = heapq.heappop(heap)
        fb, _, b = heapq.heappop(heap)
        for s in a + b:
            lens[s] += 1
        heapq.heappush(heap, (fa + fb, tie, a + b))
        tie += 1
    if max(lens) > maxlen:
        for s in syms:
            lens[s] = min(lens[s], maxlen)
        over = kraft(lens, maxlen) - (1 << maxlen)
        rare_first = sorted(syms, key=lambda s: (freqs[s], s))
        while over > 0:                                    # lengthen the rarest symbol among the deepest below maxlen
            s = max((s for s in rare_first if lens[s] < maxlen), key=lambda s: lens[s])
            lens[s] += 1
            over -= 1 << (maxlen - lens[s])
        while over < 0:                                    # ... and give back what that took too much
            s = max((s for s in reversed(rare_first) if (1 << (maxlen - lens[s])) <= -over and lens[s] > 1), key=lambda s: lens[s])
            over += 1 << (maxlen - lens[s])
            lens[s] -= 1
    assert kraft(lens, maxlen) == 1 << maxlen
    return lens


def lengths_with_max(freqs, maxlen):
    """a complete code for the symbols with a frequency whose longest code has exactly maxlen bits: the maxlen rarest symbols
    hang on a comb below the first bit (lengths 2, 3, ..., maxlen - 1, maxlen, maxlen), the others share the other half"""
    syms = sorted((s for s, f in enumerate(freqs) if f > 0), key=lambda s: (freqs[s], s))
    if len(syms) < maxlen + 1:
        raise ValueError("%d symbols cannot reach %d bits" % (len(syms), maxlen))
    lens = [0] * len(freqs)
    comb, rest = syms[:maxlen], syms[maxlen:]
    for i, s in enumerate(comb):                           # rarest first: the deepest
        lens[s] = maxlen if i < 2 else maxlen + 1 - i
    sub = [freqs[s] if s in set(rest) else 0 for s in range(len(freqs))]
    if len(rest) == 1:
        lens[rest[0]] = 1
    else:
        for s, l in enumerate(huffman_lengths(sub, maxlen - 1)):
            if l:
                lens[s] = l + 1
    assert kraft(lens, maxlen) == 1 << maxlen and max(lens) == maxlen
    return lens


def one_code(symbol=0, n=30):
    """a distance tree of one code of one bit (legal: RFC 1951 3.2.7)"""
    lens = [0] * n
    lens[symbol] = 1
    return lens


def no_codes(n=1):
    """no distance code at all: a block of literals only"""
    return [0] * n


def canonical(lens):
    """symbol -> (code with its bits reversed for an LSB-first stream, length) by RFC 1951 3.2.2; a set that is not a prefix
    code gets codes by the same rule, cut to their lengths"""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 17):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            c = nxt[l] & ((1 << l) - 1)
            nxt[l] += 1
            out[s] = (int(format(c, "0%db" % l)[::-1], 2), l)
    return out


# ---- bits ----------------------------------------------------------------------------------------------------------------
class _Acc:
    """the bits of one block: a small accumulator spilled into bytes, one int at the end"""
    def __init__(self):
        self.buf, self.v, self.n = bytearray(), 0, 0

    def put(self, val, nbits):
        self.v |= val << self.n
        self.n += nbits
        if self.n >= 64:
            k = self.n >> 3
            self.buf += (self.v & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.v >>= 8 * k
            self.n -= 8 * k

    def bits(self):
        return int.from_bytes(self.buf, "little") | (self.v << (8 * len(self.buf))), 8 * len(self.buf) + self.n


def _put_tokens(a, tokens, lit, dist):
    for t in tokens:
        if isinstance(t, int):
            a.put(*lit[t])
        elif t[0] == "S":
            a.put(*lit[t[1]])
        else:
            if t[0] == "L":
                ls, le, lv, ds, de, dv = t[1], LEN_EXTRA[t[1] - 257], t[2], t[3], (DIST_EXTRA + [13, 13])[t[3]], t[4]
            else:
                ls, le, lv = len_symbol(t[0])
                ds, de, dv = dist_symbol(t[1])
            a.put(*lit[ls])
            a.put(lv, le)
            a.put(*dist.get(ds, (0, 0)))                    # (a block without that distance code: the extra bits stand alone)
            a.put(dv, de)
    a.put(*lit.get(256, (0, 0)))                            # (a code without end-of-block: the block just stops)


_FIXED = (canonical(FIXED_LIT_LENS), canonical(FIXED_DIST_LENS))


def fixed_bits(tokens, final, end_of_block=True):
    a = _Acc()
    a.put(int(final) | 1 << 1, 3)
    _put_tokens(a, tokens, *_FIXED)
    v, n = a.bits()
    return (v, n) if end_of_block else (v & ((1 << (n - 7)) - 1), n - 7)


def run_length_ops(seq, mode="greedy", split_at=None):
    """the code-length list as code-length symbols: [(0..15,)] / [(16, rep 3..6)] / [(17, rep 3..10)] / [(18, rep 11..138)].
    "literal": no repeats; "greedy": the longest repeat that fits, runs cross from the literal lengths into the distance
    lengths; "split": greedy, but no run crosses position split_at"""
    if mode == "literal":
        return [(l,) for l in seq]
    ops, i, n = [], 0, len(seq)
    while i < n:
        stop = n if mode == "greedy" or split_at is None or i >= split_at else split_at
        j = i
        while j < stop and seq[j] == seq[i]:
            j += 1
        run = j - i
        if seq[i] == 0:
            while run >= 3:
                r = min(run, 138)
                ops.append((18, r) if r >= 11 else (17, r))
                run -= r
                i += r
        else:
            ops.append((seq[i],))
            run -= 1
            i += 1
            while run >= 3:
                r = min(run, 6)
                ops.append((16, r))
                run -= r
                i += r
        for _ in range(run):
            ops.append((seq[i],))
            i += 1
    return ops


def ops_lengths(ops):
    """the length list a decoder gets from the ops (16 repeats what stands before it; nothing stands before the first)"""
    out = []
    for op in ops:
        if op[0] < 16:
            out.append(op[0])
        elif op[0] == 16:
            out += [out[-1] if out else 0] * op[1]
        else:
            out += [0] * op[1]
    return out


def dynamic_bits(tokens, lit_lens, dist_lens, final, hlit=None, hdist=None, hclen=None, cl_plan=None, cut_at=None):
    """One dynamic block.  lit_lens / dist_lens: the code lengths as they are to be written (nothing is checked: an
    incomplete or over-subscribed set is written as it is).  hlit / hdist: how many of them the header announces (257.. /
    1..; 287, 288 and 31, 32 give the field values 30 and 31).  cl_plan: a dict of
      "mode":    "literal" | "greedy" | "split" (run_length_ops), or
      "ops":     the code-length symbols themselves (whatever lengths they spell; lit_lens / dist_lens then only code the tokens)
      "cl_lens": the 19 lengths of the code-length code (default: a complete code of at most 7 bits for the symbols used)
    hclen: how many of them are written (default: up to the last that is not zero, at least 4).
    cut_at: a list that receives the bit offsets of the header's field boundaries."""
    plan = dict(cl_plan or {})
    lit_lens, dist_lens = list(lit_lens), list(dist_lens)
    if hlit is None:
        hlit = max(257, max((i + 1 for i, l in enumerate(lit_lens) if l), default=0))
    if hdist is None:
        hdist = max(1, max((i + 1 for i, l in enumerate(dist_lens) if l), default=0))
    seq = (lit_lens + [0] * hlit)[:hlit] + (dist_lens + [0] * hdist)[:hdist]
    ops = plan.get("ops") or run_length_ops(seq, plan.get("mode", "greedy"), hlit)
    cl_lens = plan.get("cl_lens")
    if cl_lens is None:
        f = [0] * 19
        for op in ops:
            f[op[0]] += 1
        if sum(1 for x in f if x) == 1:                    # (one symbol alone is no complete code: a second one, unused)
            f[0 if f[0] == 0 else 1] += 1
        cl_lens = huffman_lengths(f, 7)
    if hclen is None:
        hclen = max(4, max(i + 1 for i in range(19) if cl_lens[CL_ORDER[i]]))
    assert all(cl_lens[CL_ORDER[i]] == 0 for i in range(hclen, 19)), "hclen cuts a code-length code length off"
    a = _Acc()
    marks = [] if cut_at is None else cut_at

    def mark():
        marks.append(8 * len(a.buf) + a.n)
    a.put(int(final) | 2 << 1, 3); mark()
    a.put((hlit - 257) & 31, 5); mark()
    a.put((hdist - 1) & 31, 5); mark()
    a.put(hclen - 4, 4); mark()
    for i in range(hclen):
        a.put(cl_lens[CL_ORDER[i]], 3)
    mark()
    cl = canonical(cl_lens)
    for k, op in enumerate(ops):
        a.put(*cl[op[0]])
        if op[0] == 16:
            a.put(op[1] - 3, 2)
        elif op[0] == 17:
            a.put(op[1] - 3, 3)
        elif op[0] == 18:
            a.put(op[1] - 11, 7)
        if k == len(ops) // 2:
            mark()
    mark()
    _put_tokens(a, tokens, canonical(lit_lens), canonical(dist_lens))
    return a.bits()


class Stream:
    """one deflate stream: blocks appended at whatever bit the last one ended"""
    def __init__(self):
        self._done, self._v, self._n = bytearray(), 0, 0

    @property
    def bitpos(self):
        return 8 * len(self._done) + self._n

    def raw(self, v, nbits):
        self._v |= v << self._n
        self._n += nbits
        if self._n >= 1 << 15:
            k = self._n >> 3
            self._done += (self._v & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self._v >>= 8 * k
            self._n -= 8 * k
        return self

    def stored(self, data, final=False, nlen=None, btype=0):
        """a stored block: the three header bits, zero bits up to the byte boundary, LEN, NLEN (the complement of LEN unless
        given), the bytes.  btype = 3 writes the reserved block type with the same layout."""
        data = bytes(data)
        assert len(data) <= 65535
        self.raw(int(final) | btype << 1, 3)
        self.raw(0, -self.bitpos & 7)
        self.raw(int.from_bytes(struct.pack("<HH", len(data), (len(data) ^ 0xFFFF) if nlen is None else nlen) + data, "little"),
                 32 + 8 * len(data))
        return self

    def fixed(self, tokens, final=False):
        return self.raw(*fixed_bits(tokens, final))

    def dynamic(self, tokens, lit_lens, dist_lens, final=False, **kw):
        return self.raw(*dynamic_bits(tokens, lit_lens, dist_lens, final, **kw))

    def bytes(self):
        """the stream so far, its last byte filled with zero bits"""
        k = (self._n + 7) >> 3
        return bytes(self._done) + self._v.to_bytes(k, "little")


# ---- containers ------------------------------------------------------------------------------------------------------------
def gzip_member(deflate_bytes, text):
    """RFC 1952: a member without name, comment or time; CRC-32 and ISIZE are those of `text`"""
    return (b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff" + bytes(deflate_bytes) +
            struct.pack("<II", zlib.crc32(text) & 0xFFFFFFFF, len(text) & 0xFFFFFFFF))


def bgzf_block(deflate_bytes, text):
    """SAM specification 4.1: a gzip member with the 'BC' extra subfield that holds its own size minus one"""
    total = 18 + len(deflate_bytes) + 8
    if total > 65536 or len(text) > 65536:
        raise ValueError("a BGZF block of %d bytes" % total)
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", total - 1) + bytes(deflate_bytes) +
            struct.pack("<II", zlib.crc32(text) & 0xFFFFFFFF, len(text)))


BGZF_EOF = bgzf_block(b"\x03\x00", b"")


def bgzf_file(blocks, eof=True):
    return b"".join(blocks) + (BGZF_EOF if eof else b"")
