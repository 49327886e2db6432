"""The catalogue of DEFLATE streams the three inflaters are tested on (tests/test_deflate_streams.py on the host,
tests/test_gpu_deflate_streams.py on the device): streams written bit by bit with tests/deflate_writer.py, most of them
of a kind zlib's encoder never writes.  catalogue() is a list of (name, deflate_bytes, text, legal), built once; zlib's
inflater pins every entry (legal: it gives `text` and ends in the stream's last byte; not legal: it refuses the stream,
alone or inside its container).  recipes() keeps the blocks of the legal entries so that they can be written again, with
BFINAL cleared, into one long gzip member (Member, host_member, device_member, runs_member)."""
import functools
import random

import deflate_writer as dw

LIT_PB, DIST_PB, HOST_LIT_PB = 10, 9, 11                   # the decoders' table widths (csrc/inflate_gpu.hip, csrc/inflate_mt.cpp)
NEAR, RING, BZ_NEAR, BZ_RING = 1280, 2048, 3584, 4096      # the device decoders' ring limits (csrc/inflate_gpu.hip)
RING_DISTANCES = [NEAR - 1, NEAR, NEAR + 1, NEAR + 100, RING - 1, RING, RING + 1,
                  BZ_NEAR - 1, BZ_NEAR, BZ_NEAR + 1, BZ_NEAR + 100, BZ_RING - 1, BZ_RING, BZ_RING + 1]
GRID_LENGTHS = [3, 63, 64, 65, 128, 258]
GRID_DISTANCES = [1, 2, 3, 4, 5, 7, 31, 32, 33, 63, 64, 65, 127, 129, 257, 258, 259]


def fastq_text(n, seed):
    """n bytes of FASTQ-like text: records of 30 .. 150 bases, qualities in runs"""
    rng = random.Random(seed)
    out, i = [], 0
    while sum(map(len, out)) < n:
        m = rng.choice([30, 75, 100, 150])
        seq = "".join(rng.choice("ACGT") if rng.random() > 0.01 else "N" for _ in range(m))
        q, qual = 40, []
        for _ in range(m):
            if rng.random() < 0.2:
                q = rng.choice([2, 11, 25, 37, 40])
            qual.append(chr(33 + q))
        out.append("@r%d.%d/1\n%s\n+\n%s\n" % (seed, i, seq, "".join(qual)))
        i += 1
    return "".join(out).encode()[:n]


def binary_text(n, seed):
    """every byte value once, then random bytes with repeats of what came before"""
    rng = random.Random(seed)
    out = bytearray(range(256))
    while len(out) < n:
        if rng.random() < 0.3:
            a = rng.randrange(len(out))
            out += out[a:a + rng.randrange(3, 40)]
        else:
            out += bytes(rng.randrange(256) for _ in range(rng.randrange(1, 20)))
    return bytes(out[:n])


# ---- blocks: ("stored", data, kw) | ("fixed", tokens) | ("dynamic", tokens, lit_lens, dist_lens, kw) ---------------------
_bits = {}


def block_tokens(b):
    return list(b[1]) if b[0] == "stored" else b[1]


def emit(stream, b, final):
    """block b at the stream's end (the bits of a Huffman block are made once and kept, with the block)"""
    if b[0] == "stored":
        return stream.stored(b[1], final, **b[2])
    key = (id(b), final)
    if key not in _bits:
        _bits[key] = (b, dw.fixed_bits(b[1], final) if b[0] == "fixed" else dw.dynamic_bits(b[1], b[2], b[3], final, **b[4]))
    return stream.raw(*_bits[key][1])


def write(blocks):
    s = dw.Stream()
    for i, b in enumerate(blocks):
        emit(s, b, i + 1 == len(blocks))
    return s.bytes()


def stored(data, **kw):
    return ("stored", bytes(data), kw)


def fixed(tokens):
    return ("fixed", list(tokens))


def dist_lens_for(fd, dist_max=None):
    used = [s for s, f in enumerate(fd) if f]
    if not used:
        return dw.no_codes()
    if len(used) == 1:
        return dw.one_code(used[0], used[0] + 1)
    return dw.lengths_with_max(fd, dist_max) if dist_max else dw.huffman_lengths(fd, 15)


def dyn(tokens, lit_max=None, dist_max=None, lit_lens=None, dist_lens=None, **kw):
    """a dynamic block whose codes fit the tokens: Huffman's, or with a longest code of exactly lit_max / dist_max bits"""
    tokens = list(tokens)
    fl, fd = dw.symbol_freqs(tokens)
    if lit_lens is None:
        lit_lens = dw.lengths_with_max(fl, lit_max) if lit_max else dw.huffman_lengths(fl, 15)
    if dist_lens is None:
        dist_lens = dist_lens_for(fd, dist_max)
    return ("dynamic", tokens, lit_lens, dist_lens, kw)


def cl_freqs(ops):
    f = [0] * 19
    for op in ops:
        f[op[0]] += 1
    return f


def header_ops(b, mode="greedy"):
    """the code-length symbols of a dynamic block's header as run_length_ops would write them"""
    lit, dist = b[2], b[3]
    hlit = b[4].get("hlit") or max(257, max(i + 1 for i, l in enumerate(lit) if l))
    hdist = b[4].get("hdist") or max(1, max((i + 1 for i, l in enumerate(dist) if l), default=0))
    seq = (list(lit) + [0] * hlit)[:hlit] + (list(dist) + [0] * hdist)[:hdist]
    return dw.run_length_ops(seq, mode, hlit), hlit, hdist


def with_plan(b, **plan):
    kw = dict(b[4])
    kw["cl_plan"] = plan
    return (b[0], b[1], b[2], b[3], kw)


def thirteen_bit_matches(k):
    """12 literals and k matches of 13 bits each in a fixed block (length 11: 7 + 1 bits, distance 4: 5 bits): the block,
    end-of-block included, is 10 + 96 + 13 k bits long"""
    return list(b"ACGTTGCAGGCA") + [(11, 4)] * k


@functools.lru_cache(maxsize=None)
def _build():
    T = fastq_text(40000, 1)
    B = binary_text(3000, 2)
    tok3k = dw.tokenize(T[:3000])
    legal = []

    def add(name, *blocks):
        legal.append((name, list(blocks)))

    # ---- 1. stored blocks
    add("stored_len0_alone", stored(b""))
    add("stored_len0_sync_flush", fixed(dw.tokenize(T[:300])), stored(b""), dyn(dw.tokenize(T[300:900], T[:300])))
    add("stored_len0_ten_in_a_row", fixed(dw.tokenize(T[:200])), *[stored(b"") for _ in range(10)], fixed(dw.tokenize(T[200:400], T[:200])))
    for k in range(8):                                      # the fixed block in front ends at bit (10 + 96 + 13 k) mod 8
        add("stored_from_bit_phase_%d" % ((106 + 13 * k) % 8), fixed(thirteen_bit_matches(k)), stored(T[500:557]))
    for n in (1, 255, 256, 257, 65280):
        add("stored_len_%d" % n, stored(fastq_text(n, 3)))
    # ---- 2. fixed blocks
    add("fixed_empty_final", fixed([]))
    add("fixed_empty_not_final", fixed([]), fixed(dw.tokenize(T[:200])))
    add("fixed_every_literal", fixed(range(256)))
    toks = list(T[:40])
    for sym in range(257, 286):
        e = dw.LEN_EXTRA[sym - 257]
        toks += [("L", sym, 0, 4, 0), T[sym], ("L", sym, (1 << e) - 1, 4, 1), T[sym + 1]]
    add("fixed_every_length_symbol", fixed(toks))
    front = dyn(dw.tokenize(T[:32768]))
    toks = []
    for ds in range(30):
        e = dw.DIST_EXTRA[ds]
        toks += [("L", 258, 0, ds, 0), 65 + ds, ("L", 258, 0, ds, (1 << e) - 1), 10]
    add("fixed_every_distance_symbol", front, fixed(toks))
    # ---- 3. dynamic blocks: the shapes of the codes
    for m in (11, 12, 15):
        add("dyn_literal_code_max_%d" % m, dyn(tok3k, lit_max=m))
    spread = dw.tokenize(T[:1500]) + [t for d in range(20) for t in ((4 + d % 5, dw.DIST_BASE[d]), T[d])]
    for m in (10, 15):
        add("dyn_distance_code_max_%d" % m, dyn(spread, dist_max=m))
    b15 = dyn(tok3k, lit_max=15)
    ops, _, _ = header_ops(b15, "literal")
    b = with_plan(b15, mode="literal", cl_lens=dw.lengths_with_max(cl_freqs(ops), 7))
    add("dyn_code_length_code_7_bits_hclen_19", b)
    add("dyn_hclen_5", dyn(list(range(255)) * 2, lit_lens=[8] * 255 + [0, 8], dist_lens=dw.no_codes(),
                           cl_plan={"mode": "literal", "cl_lens": [1 if s in (0, 8) else 0 for s in range(19)]}, hclen=5))
    lits = list(T[:800])
    add("dyn_hlit_257_no_distance_code", dyn(lits))
    add("dyn_hlit_286_hdist_30", dyn(tok3k, hlit=286, hdist=30))
    runs = [65, (20, 1), 67, (9, 1), 10] * 20
    add("dyn_hdist_1_one_distance_code", dyn(runs))
    add("dyn_one_distance_code_symbol_8", dyn(list(T[:30]) + [t for i in range(40) for t in ((5 + i % 7, 17 + i % 8), T[40 + i])]))
    add("dyn_literal_code_of_two_symbols", dyn([65] * 50, lit_lens=[0] * 65 + [1] + [0] * 190 + [1], dist_lens=dw.no_codes()))
    base = dyn(tok3k)
    ops, _, _ = header_ops(base)
    swapped = []
    for op in ops:                                          # (17 / 18, n) -> (17 / 18, n - 3), (16, 3): the 16 repeats a zero
        if op[0] == 17 and op[1] >= 6 or op[0] == 18 and op[1] >= 14:
            swapped += [(op[0], op[1] - 3), (16, 3)]
        else:
            swapped.append(op)
    assert dw.ops_lengths(swapped) == dw.ops_lengths(ops) and any(a[0] in (17, 18) and b_[0] == 16 for a, b_ in zip(swapped, swapped[1:]))
    add("dyn_16_behind_17_and_18", with_plan(base, ops=swapped))
    small = list(b"ACGT\n@+I")
    rng = random.Random(7)
    toks = [rng.choice(small) for _ in range(260)]
    for i in range(120):
        toks += [(3 + i % 7, 1 + (i * 37) % 250), rng.choice(small)]
    lit16 = [0] * 264
    for s in small + list(range(256, 264)):
        lit16[s] = 4
    b = dyn(toks, lit_lens=lit16, dist_lens=[4] * 16)
    assert any(op == (16, 6) for op in header_ops(b)[0])
    add("dyn_16_run_from_literal_into_distance_lengths", b)
    far = [t for i in range(60) for t in ((4 + i % 5, 5 + i % 20), T[i])]
    b = dyn(list(T[:100]) + far, hlit=286)
    assert b[3][:4] == [0, 0, 0, 0]
    add("dyn_18_run_from_literal_into_distance_lengths", b)
    alphabet = [10] + list(range(48, 59)) + list(range(62, 118))
    toks = alphabet + [rng.choice(alphabet) for _ in range(700)]
    b = dyn(toks)
    ops, _, _ = header_ops(b)
    assert (18, 138) in ops and (17, 3) in ops
    add("dyn_18_run_of_138_and_17_run_of_3", b)
    fl, fd = dw.symbol_freqs(tok3k)
    fl[256], fl[1] = 0.1, 0.2                               # end-of-block and a literal that never comes: the two deepest leaves
    b = dyn(tok3k, lit_lens=dw.lengths_with_max(fl, 15))
    assert b[2][256] == 15 and b[2].count(15) == 2
    add("dyn_end_of_block_is_the_15_bit_code_in_use", b)
    fl, fd = dw.symbol_freqs(tok3k)
    fl[256] = 0
    ll = [l + 1 if l else 0 for l in dw.huffman_lengths(fl, 14)]
    ll[256] = 1
    add("dyn_end_of_block_is_the_one_bit_code", dyn(tok3k, lit_lens=ll))
    # ---- 4. matches
    add("match_258_at_1_second_symbol_fixed", fixed([65, (258, 1)]))
    add("match_258_at_1_second_symbol_dynamic", dyn([65, (258, 1)]))
    toks, pos = [], 0
    for step in (1, 7, 93, 400, 1500):
        toks += list(T[pos:pos + step])
        pos += step
        toks.append((min(258, 3 + step), pos))
        pos += min(258, 3 + step)
    add("match_reaches_the_first_byte", dyn(toks))

    def grid(prefix):
        toks = list(prefix)
        for d in GRID_DISTANCES:
            for n in GRID_LENGTHS:
                toks += [(n, d), prefix[(n + d) % len(prefix)]]
        return toks
    add("match_grid_fixed", fixed(grid(T[:300])))
    add("match_grid_dynamic", dyn(grid(T[:300])))
    for name, dists in (("gz", RING_DISTANCES[:7]), ("bgzf", RING_DISTANCES[7:])):
        toks = dw.tokenize(T[:4300])
        pos, fill = 4300, 4300
        for d in dists:
            for n in (3, 258):
                for off in (0, 255):                        # right behind a flush of 256 bytes, and 255 bytes behind it
                    while pos % 256 != off:
                        toks.append(T[fill])
                        fill += 1
                        pos += 1
                    toks.append((n, d))
                    pos += n
        add("match_at_the_ring_limits_%s" % name, dyn(toks))
    add("match_258_at_32767_and_32768", front, dyn([(258, 32768), 65, (258, 32767), 67, (3, 32768), (3, 32767), 10, (258, 32768)]))
    add("match_258_runs_that_wrap_the_ring", dyn([65] + [(258, 1)] * 20 + [67, 71, 84] + [(258, 4)] * 20 + [10]))
    # ---- 5. sequences of blocks
    order = "SSFFDDSDFS" * 4                                # every ordered pair of the three types, four times
    blocks = []
    for i, kind in enumerate(order):
        piece, hist = T[1000 + 60 * i:1060 + 60 * i], T[1000:1000 + 60 * i]
        blocks.append(stored(piece) if kind == "S" else fixed(dw.tokenize(piece, hist)) if kind == "F" else dyn(dw.tokenize(piece, hist)))
    add("forty_blocks_of_alternating_types", *blocks)
    add("final_empty_stored_block", fixed(dw.tokenize(T[:200])), stored(b""))
    for k, bit in ((4, 7), (1, 0)):                         # (106 + 13 k) + 10 bits: the last one is bit 7 / bit 0 of the last byte
        assert (106 + 13 * k + 10 - 1) % 8 == bit
        add("final_empty_fixed_block_ends_at_bit_%d" % bit, fixed(thirteen_bit_matches(k)), fixed([]))
    # ---- 6. any data: all 256 byte values through 2, 3 and 4
    tokb = dw.tokenize(B, min_match=3)
    add("binary_stored", stored(B))
    add("binary_fixed", fixed(tokb))
    add("binary_dynamic_literal_code_max_15", dyn(tokb, lit_max=15))
    add("binary_dynamic_distance_code_max_10", dyn(tokb + [t for d in range(18) for t in ((3 + d, dw.DIST_BASE[d]), 200 + d)], dist_max=10))
    add("binary_match_grid", dyn(grid(B[:300])))

    out = []
    for name, blocks in legal:
        toks = [t for b in blocks for t in block_tokens(b)]
        out.append((name, write(blocks), dw.expand(toks), True))
    assert len(set(n for n, _ in legal)) == len(legal)
    return out + _illegal(T), dict(legal)


def _illegal(T):
    text = T[2000:2200]
    good = list(text)
    out = []

    def bad(name, deflate_bytes, txt=text):
        out.append((name, bytes(deflate_bytes), txt, False))

    def dyn_bytes(b, **more):
        kw = dict(b[4])
        kw.update(more)
        return dw.Stream().dynamic(b[1], b[2], b[3], True, **kw).bytes()
    base = dyn(dw.tokenize(T[2000:2200] + T[2000:2200]))
    text2 = text + text
    bad("btype_3", dw.Stream().stored(text, True, btype=3).bytes())
    bad("stored_nlen_is_not_the_complement", dw.Stream().stored(text, True, nlen=(len(text) ^ 0xFFFF) ^ 0x0100).bytes())
    for n in (287, 288):
        bad("dyn_hlit_field_%d" % (n - 257), dyn_bytes(base, hlit=n), text2)
    bad("dyn_hdist_field_30", dyn_bytes(base, hdist=31), text2)
    lsym = next(s for s in range(257, 286) if base[2][s])
    b32 = dyn(base[1] + [("L", lsym, 0, 31, 0)], lit_lens=base[2], dist_lens=(base[3] + [0] * 32)[:31] + [max(base[3])], hdist=32)
    bad("dyn_hdist_field_31_with_distance_symbol_31", dyn_bytes(b32), text2)
    deepest = max(range(len(base[2])), key=lambda s: base[2][s])
    over, under = list(base[2]), list(base[2])
    over[deepest] -= 1
    under[deepest] += 1
    bad("dyn_literal_set_over_subscribed", dyn_bytes(dyn(base[1], lit_lens=over, dist_lens=base[3])), text2)
    bad("dyn_literal_set_incomplete", dyn_bytes(dyn(base[1], lit_lens=under, dist_lens=base[3])), text2)
    bad("dyn_distance_set_of_two_incomplete", dyn_bytes(dyn(good, dist_lens=[1, 2])))
    bad("dyn_one_distance_code_of_length_2", dyn_bytes(dyn(good, dist_lens=[2])))
    ops, hlit, hdist = header_ops(base)
    cl = dw.huffman_lengths(cl_freqs(ops), 7)
    cl_under = list(cl)
    cl_under[max(range(19), key=lambda s: cl[s])] += 0 if max(cl) == 7 else 1
    if cl_under == cl:                                      # (already 7 bits deep: drop a code instead)
        cl_under[max(range(19), key=lambda s: cl[s])] = 0
        ops_u = [op for op in ops if cl_under[op[0]]]
    else:
        ops_u = ops
    bad("dyn_code_length_code_incomplete", dyn_bytes(with_plan(base, ops=ops_u, cl_lens=cl_under)), text2)
    zeros = [(18, 138), (18, 120)]                          # 257 + 1 lengths, all zero, by the only code-length code there is
    bad("dyn_code_length_code_of_one_code", dyn_bytes(dyn([], lit_lens=[0] * 256 + [1], dist_lens=[0], cl_plan={"ops": zeros, "cl_lens": [0] * 18 + [1]}, hclen=4)))
    bad("dyn_hclen_4", dyn_bytes(dyn([], lit_lens=[0] * 256 + [1], dist_lens=[0],
                                     cl_plan={"ops": [(18, 138), (17, 10), (18, 110)], "cl_lens": [0, 0, 0] + [0] * 13 + [2, 2, 1]}, hclen=4)))
    bad("dyn_16_is_the_first_length", dyn_bytes(with_plan(base, ops=[(16, 3)] + ops)), text2)
    bad("dyn_run_overshoots_hlit_plus_hdist", dyn_bytes(with_plan(base, ops=ops[:-1] + [(18, 138)])), text2)
    fl, _ = dw.symbol_freqs(base[1])
    fl[256] = 0
    bad("dyn_no_end_of_block_code", dyn_bytes(dyn(base[1], lit_lens=dw.huffman_lengths(fl, 15), dist_lens=base[3])), text2)
    for s in (286, 287):
        bad("fixed_length_symbol_%d" % s, dw.Stream().fixed(good + [("S", s)], True).bytes())
    for s in (30, 31):
        bad("fixed_distance_symbol_%d" % s, dw.Stream().fixed(good + [("L", 257, 0, s, 0)], True).bytes())
    bad("dyn_match_without_distance_codes", dyn_bytes(dyn(good + [(3, 1)] + good, dist_lens=dw.no_codes())), text + text[-1:] * 3 + text)
    bad("distance_too_far_at_the_start", dw.Stream().fixed([(3, 1)] + good, True).bytes())
    bad("distance_too_far_in_mid_stream", dw.Stream().fixed(good + [(3, len(good) + 1)] + good, True).bytes())
    marks = []
    whole = dw.Stream().dynamic(base[1], base[2], base[3], True, cut_at=marks).bytes()
    for i, m in enumerate(marks):                           # the stream ends behind BFINAL/BTYPE, HLIT, HDIST, HCLEN, the code-length
        cut = bytearray(whole[:(m + 7) // 8])                # code, half of the lengths, all of the lengths
        if m % 8:
            cut[-1] &= (1 << (m % 8)) - 1
        bad("dyn_header_cut_at_field_%d" % i, cut, text2)
    bad("one_literal_beyond_isize", dw.Stream().fixed(good + [65], True).bytes())
    bad("a_match_that_overshoots_isize", dw.Stream().fixed(good[:-2] + [(3, 5)], True).bytes(), dw.expand(good[:-2] + [(3, 5)])[:-1])
    bad("one_byte_short_of_isize", dw.Stream().fixed(good[:-1], True).bytes())
    bad("a_byte_behind_the_final_block", dw.Stream().fixed(good, True).bytes() + b"\x00")
    return out


def catalogue():
    return _build()[0]


def recipes():
    return _build()[1]


# ---- one long gzip member for the speculative decoders ---------------------------------------------------------------------
class Member:
    """One deflate stream made of segments, every block with BFINAL cleared but the last.  A segment starts with a dynamic
    "landing" block of FASTQ text (about 1 KB: what the searches for block starts look for) and a small fixed block of
    matches aimed at the landing block's first byte and at the byte in front of it; what follows is the caller's.  The
    landing blocks come in three forms: 0, literals only; 1, a first symbol (258, 32768) — position 0 of the unknown window
    where a chunk starts there; 2, a first symbol (3, 1) — its position 32767.  landings: (byte offset, text so far) of
    every landing block."""
    T = fastq_text(8 * 2300, 11)

    def __init__(self):
        self.s, self.out, self.seg, self.landings, self._land = dw.Stream(), bytearray(), 0, [], {}

    @property
    def at(self):
        return self.s.bitpos // 8

    def add(self, block):
        emit(self.s, block, False)
        self.out += dw.expand(block_tokens(block), bytes(self.out[-32768:]))

    def landing(self, form=None):
        if form is None or len(self.out) < 32768:
            form = self.seg % 3 if len(self.out) >= 32768 else 0
        key = (form, self.seg % 8)
        if key not in self._land:
            piece = list(self.T[2300 * (self.seg % 8):2300 * (self.seg % 8 + 1)])
            self._land[key] = dyn([[], [(258, 32768)], [(3, 1), (4, 3)]][form] + piece)
        self.landings.append((self.at, len(self.out)))
        before = len(self.out)
        self.add(self._land[key])
        q = len(self.out) - before
        if self.seg:                                        # the landing block's first byte, then the byte in front of it
            self.add(fixed([(4, q), (4, q + 5), (5, 2), (258, 32767 if len(self.out) >= 32768 else q)]))
        self.seg += 1

    def stored_over(self, cut):
        """a stored block of text from here to just behind byte offset `cut`: no block start between here and there"""
        self.add(stored(fastq_text(max(cut - self.at, 0) + 8, 100 + self.seg)))

    def refused(self, tokens, counted=b""):
        """a fixed block that a decoder has to refuse; `counted`: what it adds to the text that the trailer describes"""
        self.s.fixed(tokens)
        self.out += counted

    def finish(self, deflate_size):
        """(deflate_bytes, text): stored text up to exactly deflate_size bytes, the last block final"""
        while True:
            left = deflate_size - ((self.s.bitpos + 3 + 7) // 8 + 4)
            assert left >= 0
            filler = fastq_text(min(left, 30000), 200 + self.seg)
            self.s.stored(filler, final=left <= 30000)
            self.out += filler
            self.seg += 1
            if left <= 30000:
                break
        d = self.s.bytes()
        assert len(d) == deflate_size
        return d, bytes(self.out)


class Rotation:
    """the legal catalogue entries whose stream is at most max_block bytes long, in turn; those above once_above once"""
    def __init__(self, max_block, once_above):
        self.rec = recipes()
        self.size = {name: len(d) for name, d, _, ok in catalogue() if ok}
        self.text = {name: len(t) for name, _, t, ok in catalogue() if ok}
        self.names = [n for n in self.rec if self.size[n] <= max_block]
        self.reach = {n: dw.reach([t for b in self.rec[n] for t in block_tokens(b)]) for n in self.names}
        self.once_above, self.turn, self.used = once_above, 0, set()

    def next_into(self, m):
        """the next entry that the text so far can carry, appended to member m; its name, or None"""
        for _ in range(len(self.names)):
            name = self.names[self.turn % len(self.names)]
            self.turn += 1
            if self.reach[name] <= len(m.out) and not (self.size[name] > self.once_above and name in self.used):
                self.used.add(name)
                for b in self.rec[name]:
                    m.add(b)
                return name
        return None


def host_member(deflate_size, cuts):
    """(deflate_bytes, text, member) for csrc/inflate_mt.cpp: two entries behind every landing block, every legal entry in it
    (those above 4000 bytes once); over every byte offset in `cuts` lies a stored block, so that the first block start behind
    the cut is a landing block of form 1"""
    m, rot, cuts = Member(), Rotation(70000, 4000), sorted(cuts)
    while m.at < deflate_size - 78000:
        if cuts and m.at + 14000 >= cuts[0] and len(m.out) >= 32768:      # (14000: more than a segment without a large entry)
            m.stored_over(cuts.pop(0))
            m.landing(1)
        else:
            m.landing()
        rot.next_into(m)
        rot.next_into(m)
    assert not cuts, "the member ended in front of a cut"
    m.entries = rot.used
    return m.finish(deflate_size) + (m,)


def host_member_with_a_short_chunk(deflate_size, cut1, cut2):
    """(deflate_bytes, text, member) for csrc/inflate_mt.cpp on three chunks cut at cut1 and cut2: from in front of cut1 to
    6000 bytes in front of cut2 there are stored blocks only, then one landing block, a stored block over cut2 and a landing
    block of form 1.  The search from cut1 lands 6000 bytes in front of cut2, the one from cut2 right behind it: the chunk
    between them holds less text than a window (member.short_chunk_text), and the matches at 32 767 and 32 768 behind cut2
    reach through it into the chunk in front."""
    m, rot = Member(), Rotation(70000, 4000)
    while m.at < cut1 - 80000:
        m.landing()
        rot.next_into(m)
        rot.next_into(m)
    filler = stored(fastq_text(60000, 300))
    while m.at < cut2 - 70000:
        m.add(filler)
    m.stored_over(cut2 - 6000)
    before = len(m.out)
    m.landing(0)
    m.stored_over(cut2)
    m.short_chunk_text = len(m.out) - before
    m.landing(1)
    m.add(dyn([(258, 32768), 65, (258, 32767), 10, (3, 32768 - m.short_chunk_text)]))
    while m.at < deflate_size - 78000:
        m.landing()
        rot.next_into(m)
    return m.finish(deflate_size) + (m,)


def device_member(deflate_size, refuse=None):
    """(deflate_bytes, text, member) for the device's member decoder: one entry behind every landing block (those above 2500
    bytes once, the block of 65 280 stored bytes left out), and a segment without an entry behind one whose text is more than
    2000 bytes and more than 8 times its stream (a chunk has room for 10 symbols per byte of its stream).
    refuse: "first" — the member starts with a match in front of its first byte; "symbol 30" — segment 40 starts with a
    distance symbol 30; "front" — behind the first landing block beyond 10 240 bytes a match of 3 reaches one byte in front
    of the stream's first (its 3 bytes are counted in the text: the trailer's ISIZE agrees with what a decoder counts).
    member.refused_at: (byte offset, text so far) of that block."""
    m, rot, rest = Member(), Rotation(20000, 2500), False
    m.refused_at = None
    while m.at < deflate_size - 40000:
        if refuse == "first" and m.seg == 0 or refuse == "symbol 30" and m.seg == 40:
            m.refused_at = (m.at, len(m.out))
            m.refused([(3, 1)] if refuse == "first" else [65, ("L", 257, 0, 30, 0)])
        m.landing()
        if refuse == "front" and m.refused_at is None and m.at >= 10240:
            m.refused_at = (m.at, len(m.out))
            m.refused([(3, len(m.out) + 1)], b"???")
        name = None if rest else rot.next_into(m)
        rest = name is not None and rot.text[name] > 2000 and rot.text[name] > 8 * rot.size[name]
    m.entries = rot.used
    return m.finish(deflate_size) + (m,)


def runs_member(deflate_size, runs):
    """(deflate_bytes, text, member): behind every landing block one block of `runs` matches (258, 1)"""
    m, block = Member(), dyn([(258, 1)] * runs)
    while m.at < deflate_size - 40000:
        m.landing()
        m.add(block)
    return m.finish(deflate_size) + (m,)


def shaped_streams(fq):
    """A valid FASTQ text as (BGZF file, gzip member), its pieces written in turn as a dynamic block of literals only (what the
    member decoder's search lands on), a fixed block, a dynamic block whose literal code reaches 15 bits, and a stored block;
    four blocks to a BGZF block."""
    sizes = [2300, 900, 1500, 300]
    blocks, pos, i = [], 0, 0
    while pos < len(fq):
        piece = fq[pos:pos + sizes[i % 4]]
        blocks.append((i % 4, pos, piece))
        pos += len(piece)
        i += 1

    def shape(kind, piece, hist):
        if kind == 0 or len(set(piece)) < 16:
            return dyn(list(piece))
        toks = dw.tokenize(piece, hist)
        return fixed(toks) if kind == 1 else dyn(toks, lit_max=15) if kind == 2 else stored(piece)
    member = dw.Stream()
    for n, (kind, at, piece) in enumerate(blocks):
        emit(member, shape(kind, piece, fq[max(0, at - 4096):at]), n + 1 == len(blocks))
    bg = []
    for g in range(0, len(blocks), 4):
        group, st = blocks[g:g + 4], dw.Stream()
        for n, (kind, at, piece) in enumerate(group):
            emit(st, shape(kind, piece, fq[group[0][1]:at]), n + 1 == len(group))
        bg.append(dw.bgzf_block(st.bytes(), fq[group[0][1]:group[-1][1] + len(group[-1][2])]))
    return dw.bgzf_file(bg), dw.gzip_member(member.bytes(), fq)
