// end_keys.h — the END KEYS of the contigs (SPEC S11), shared by the device text writer (writer_text_gpu.h) and the host.
// A contig links to another where the last k-mer of one orientation, its first base dropped and one base appended, is the
// first k-mer of an orientation of the other (outputs.cpp: pack / pack_rc / put2 / get2).  Here: the packing of such a
// k-mer from ASCII text, its table word, and the rule by which one of several entries with one key survives.
#pragma once
#include "kmer.h"

namespace shk {

SHK_HD uint32_t ek_code(char c) { return c == 'C' ? 1u : (c == 'G' ? 2u : (c == 'T' ? 3u : 0u)); }

// p[0 .. k) as a k-mer (kmer.h: the first base in the top 2 bits of the 2k-bit value) — outputs.cpp's pack
template <int W> SHK_HD Kmer<W> ek_pack(const char *p, uint32_t k) {
    Kmer<W> x = km_zero<W>();
    for (uint32_t i = 0; i < k; i++) km_push_back<W>(x, ek_code(p[i]), (int)k);
    return x;
}
// the reverse complement of p[0 .. k) — outputs.cpp's pack_rc (no km_revcomp: that one needs an odd k)
template <int W> SHK_HD Kmer<W> ek_pack_rc(const char *p, uint32_t k) {
    Kmer<W> x = km_zero<W>();
    for (uint32_t i = 0; i < k; i++) km_push_front<W>(x, 3u - ek_code(p[i]), (int)k);
    return x;
}
// the four k-mers that may follow x: x without its first base, then A (the caller puts C, G, T into the low 2 bits)
template <int W> SHK_HD Kmer<W> ek_successor_a(Kmer<W> x, uint32_t k) { km_push_back<W>(x, 0u, (int)k); return x; }

// One table word: fingerprint (32 bits) | orientation (1) | sorted position of the contig (31).  All ones is "empty", so the
// fingerprint is never all ones.  Entries of one key share their fingerprint: the SMALLEST word is the smallest
// (orientation, sorted position) — the host writer's "'+' before '-', then the smaller contig id".
static constexpr uint64_t EK_EMPTY = ~0ull;
SHK_HD uint64_t ek_fingerprint(uint64_t hash) { const uint64_t f = hash >> 32; return f == 0xFFFFFFFFull ? 0xFFFFFFFEull : f; }
SHK_HD uint64_t ek_entry(uint64_t hash, uint32_t orientation, uint32_t pos) {
    return (ek_fingerprint(hash) << 32) | ((uint64_t)(orientation & 1u) << 31) | (uint64_t)(pos & 0x7FFFFFFFu);
}
SHK_HD uint32_t ek_entry_pos(uint64_t e) { return (uint32_t)e & 0x7FFFFFFFu; }
SHK_HD uint32_t ek_entry_orientation(uint64_t e) { return (uint32_t)(e >> 31) & 1u; }
// of two entries with one key, does `a` win over `b`?
SHK_HD bool ek_wins(uint64_t a, uint64_t b) { return a < b; }
// slots of the table for nc contigs: a power of two >= 4 nc + 4 (two entries per contig: at most half full)
SHK_HD uint64_t ek_table_slots(uint64_t nc) { uint64_t cap = 16; while (cap < 4ull * nc + 4ull) cap <<= 1; return cap; }

}  // namespace shk
