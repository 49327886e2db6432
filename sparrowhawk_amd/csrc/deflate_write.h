// deflate_write.h — the BGZF block ENCODER (SPEC S11a), shared by the device kernels (bgzf_write_gpu.hip) and the host: one
// header, compiled for both, so that both sides give the same bytes by construction (the pattern of end_keys.h).
// A block of the output holds at most 65 280 bytes of text as ONE deflate block of literals only: dynamic Huffman codes
// (BTYPE = 2) over the 256 byte values and end-of-block, no distance code (HDIST = 0, one distance code of length 0: RFC 1951
// §3.2.7), or, where that is not strictly smaller, one stored block (BTYPE = 0).  Here: the code lengths (limited to 15 bits,
// complete, ties resolved by a written rule), the canonical codes, the block header, the choice of form, the framing.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef SHK_HD
#if defined(__HIPCC__)
#define SHK_HD __host__ __device__ __forceinline__
#else
#define SHK_HD inline
#endif
#endif

namespace shk {

static constexpr uint32_t DW_BLOCK_TEXT = 65280;      // bytes of text per block (bgzip's own figure)
static constexpr uint32_t DW_SLOT = 65536;            // a block's deflate data, before the file is laid out
static constexpr int DW_LIT = 257;                    // the literal/length alphabet in use: 256 byte values and end-of-block
static constexpr int DW_EOB = 256;
static constexpr int DW_CL = 19;                      // the code-length alphabet
static constexpr uint32_t DW_STORED_HEAD = 5;         // BFINAL/BTYPE byte, LEN, NLEN
static constexpr uint32_t DW_BGZF_HEAD = 18, DW_BGZF_TAIL = 8, DW_EOF_BYTES = 28;

// ---- the order of the symbols --------------------------------------------------------------------------------------------
// THE TIE RULE.  The used symbols (count > 0) are ordered by count, a lower count first, and among equal counts the lower
// symbol first: a total order, so whoever sorts gets the same result.  order[r] = the symbol of rank r.  Every symbol's rank is
// found on its own (the number of used symbols in front of it): `lane` of `nlanes` takes the symbols lane, lane + nlanes, ...
// — the 64 lanes of a wave on the device, lane 0 of 1 on the host.
SHK_HD void dw_rank(const uint32_t *counts, int n, uint16_t *order, int lane, int nlanes) {
    for (int i = lane; i < n; i += nlanes) {
        const uint32_t c = counts[i];
        if (!c) continue;
        int r = 0;
        for (int j = 0; j < n; j++) { const uint32_t d = counts[j]; r += (d != 0 && (d < c || (d == c && j < i))) ? 1 : 0; }
        order[r] = (uint16_t)i;
    }
}

// working memory of one code (LDS on the device)
struct DwScratch {
    uint16_t order[DW_LIT];
    uint16_t parent[2 * DW_LIT];      // of leaf r (a rank) and of inner node n_used + t
    uint32_t weight[DW_LIT];          // of the inner nodes, in the order they were made
    uint8_t depth[DW_LIT];            // of the inner nodes
    uint32_t bl[16];                  // leaves per code length
};

// ---- the code lengths ----------------------------------------------------------------------------------------------------
// counts[0..n) (their sum below 2^32), s.order as dw_rank left it.  len[i] = 0 for an unused symbol; the used ones get a
// COMPLETE code (Kraft sum exactly 1) of at most maxbits bits — a lone used symbol gets length 1, the one case that cannot be
// complete.  Returns the number of used symbols.
//   1. Huffman's tree by the two-queue method over the ordered leaves: the two smallest of (next leaf, next inner node) are
//      joined, a leaf before an inner node of the same weight, inner nodes in the order they were made.
//   2. Depths beyond maxbits are cut to maxbits; while the code is then over-subscribed, one leaf leaves the longest length
//      and the deepest leaf above it moves one level down, the two becoming brothers there: the Kraft sum (in units of
//      2^-maxbits) falls by exactly 1 a step and ends at 1.
//   3. The lengths go to the symbols by rank: the longest to the rarest.  (Where nothing was cut this costs what Huffman's tree costs.)
SHK_HD int dw_lengths(const uint32_t *counts, int n, int maxbits, DwScratch &s, uint8_t *len) {
    int nu = 0;
    for (int i = 0; i < n; i++) { len[i] = 0; nu += counts[i] ? 1 : 0; }
    if (nu == 0) return 0;
    if (nu == 1) { len[s.order[0]] = 1; return 1; }
    int li = 0, ii = 0, ni = 0;
    for (int t = 0; t < nu - 1; t++) {
        uint32_t w = 0;
        for (int q = 0; q < 2; q++) {
            int node;
            if (li < nu && (ii >= ni || counts[s.order[li]] <= s.weight[ii])) { w += counts[s.order[li]]; node = li++; }
            else { w += s.weight[ii]; node = nu + ii++; }
            s.parent[node] = (uint16_t)(nu + ni);
        }
        s.weight[ni++] = w;
    }
    s.depth[ni - 1] = 0;
    for (int t = ni - 2; t >= 0; t--) s.depth[t] = (uint8_t)(s.depth[s.parent[nu + t] - nu] + 1);
    for (int d = 0; d < 16; d++) s.bl[d] = 0;
    for (int r = 0; r < nu; r++) { int d = (int)s.depth[s.parent[r] - nu] + 1; if (d > maxbits) d = maxbits; s.bl[d]++; }
    uint32_t total = 0;
    for (int d = 1; d <= maxbits; d++) total += s.bl[d] << (maxbits - d);
    while (total > (1u << maxbits)) {
        s.bl[maxbits]--;
        for (int d = maxbits - 1; d > 0; d--) if (s.bl[d]) { s.bl[d]--; s.bl[d + 1] += 2; break; }
        total--;
    }
    int r = 0;
    for (int d = maxbits; d >= 1; d--) for (uint32_t c = 0; c < s.bl[d]; c++) len[s.order[r++]] = (uint8_t)d;
    return nu;
}

// ---- the canonical codes (RFC 1951 §3.2.2), bit-reversed: a Huffman code goes into the stream from its top bit, the stream
// fills bytes from the bottom
SHK_HD uint32_t dw_reverse(uint32_t v, int bits) { uint32_t r = 0; for (int i = 0; i < bits; i++) { r = (r << 1) | (v & 1u); v >>= 1; } return r; }
SHK_HD void dw_codes(const uint8_t *len, int n, uint16_t *code) {
    uint32_t bl[16], next[16];
    for (int d = 0; d < 16; d++) bl[d] = 0;
    for (int i = 0; i < n; i++) bl[len[i]]++;
    bl[0] = 0;
    uint32_t c = 0;
    next[0] = 0;
    for (int d = 1; d < 16; d++) { c = (c + bl[d - 1]) << 1; next[d] = c; }
    for (int i = 0; i < n; i++) code[i] = len[i] ? (uint16_t)dw_reverse(next[len[i]]++, len[i]) : (uint16_t)0;
}

// bits into a zeroed array of dwords, from the bottom of each (n <= 16)
SHK_HD void dw_put(uint32_t *w, uint32_t &nbits, uint32_t v, uint32_t n) {
    if (!n) return;
    const uint32_t i = nbits >> 5, sh = nbits & 31u;
    w[i] |= v << sh;
    if (sh + n > 32u) w[i + 1] |= v >> (32u - sh);
    nbits += n;
}

// ---- the header's run of code lengths ------------------------------------------------------------------------------------
// The 257 literal/length code lengths and the one distance code length (0) are ONE sequence of 258 values (RFC 1951 §3.2.7),
// written in the code-length alphabet by this rule: a non-zero length stands for itself (symbol 16, "repeat", is never used);
// a run of zeros is taken from its front in pieces of at most 138: a piece of 11 .. 138 is symbol 18, one of 3 .. 10 symbol 17,
// and what is left (fewer than 3) single zeros.  f(symbol, extra bits, extra value) is called for every symbol in order.
static constexpr int DW_HEADER_LENGTHS = DW_LIT + 1;
SHK_HD uint8_t dw_length_at(const uint8_t *len, int j) { return j < DW_LIT ? len[j] : (uint8_t)0; }
template <class F> SHK_HD void dw_cl_walk(const uint8_t *len, F &&f) {
    int i = 0;
    while (i < DW_HEADER_LENGTHS) {
        const uint8_t v = dw_length_at(len, i);
        if (v) { f((uint32_t)v, 0u, 0u); i++; continue; }
        int run = 1;
        while (i + run < DW_HEADER_LENGTHS && dw_length_at(len, i + run) == 0) run++;
        i += run;
        while (run >= 11) { const int m = run < 138 ? run : 138; f(18u, 7u, (uint32_t)(m - 11)); run -= m; }
        if (run >= 3) { f(17u, 3u, (uint32_t)(run - 3)); run = 0; }
        for (; run > 0; run--) f(0u, 0u, 0u);
    }
}
SHK_HD int dw_cl_order(int i) {
    // 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15
    return i < 3 ? 16 + i : (i == 3 ? 0 : ((i & 1) ? 8 - (i - 4 + 1) / 2 : 8 + (i - 4) / 2));
}

// what a block is written with
struct DwPlan {
    uint8_t len[DW_LIT];
    uint16_t code[DW_LIT];
    uint8_t cl_len[DW_CL];
    uint16_t cl_code[DW_CL];
    uint32_t hclen;             // code-length code lengths written (4 .. 19)
    uint32_t header_bits;       // BFINAL .. the last code length
    uint32_t huffman_bytes;     // the whole deflate block in the Huffman form
    uint32_t stored;            // 1: the block is a stored block (the Huffman form is not strictly smaller than 5 + the text)
};

// The serial part, from the block's histogram (counts[256] == 1: end-of-block) with s.order filled by dw_rank over the 257
// counts: lengths, codes, the code-length code, the size of the Huffman form and the choice of form.
SHK_HD void dw_plan(const uint32_t *counts, uint32_t n_text, DwScratch &s, DwPlan &p) {
    (void)dw_lengths(counts, DW_LIT, 15, s, p.len);
    dw_codes(p.len, DW_LIT, p.code);
    uint32_t clc[DW_CL];
    for (int i = 0; i < DW_CL; i++) clc[i] = 0;
    uint32_t extra = 0;
    dw_cl_walk(p.len, [&](uint32_t sym, uint32_t xb, uint32_t) { clc[sym]++; extra += xb; });
    dw_rank(clc, DW_CL, s.order, 0, 1);
    (void)dw_lengths(clc, DW_CL, 7, s, p.cl_len);        // (at least two symbols: a non-zero length and the distance code's 0)
    dw_codes(p.cl_len, DW_CL, p.cl_code);
    p.hclen = 4;
    for (int i = 4; i < DW_CL; i++) if (p.cl_len[dw_cl_order(i)]) p.hclen = (uint32_t)i + 1;
    uint32_t bits = 3 + 5 + 5 + 4 + 3 * p.hclen + extra;
    for (int i = 0; i < DW_CL; i++) bits += clc[i] * p.cl_len[i];
    p.header_bits = bits;
    uint64_t body = 0;
    for (int i = 0; i < DW_LIT; i++) body += (uint64_t)counts[i] * p.len[i];
    const uint64_t bytes = ((uint64_t)bits + body + 7) / 8;
    p.huffman_bytes = bytes > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)bytes;
    p.stored = bytes < (uint64_t)DW_STORED_HEAD + n_text ? 0u : 1u;
}

// the header of the Huffman form into zeroed dwords (at most 60 of them); returns its bits (== p.header_bits)
SHK_HD uint32_t dw_put_header(const DwPlan &p, uint32_t *w) {
    uint32_t nbits = 0;
    dw_put(w, nbits, 1u, 1);                  // BFINAL
    dw_put(w, nbits, 2u, 2);                  // BTYPE = 2
    dw_put(w, nbits, 0u, 5);                  // HLIT: 257 codes, exactly up to end-of-block
    dw_put(w, nbits, 0u, 5);                  // HDIST: one distance code (of length 0)
    dw_put(w, nbits, p.hclen - 4u, 4);
    for (uint32_t i = 0; i < p.hclen; i++) dw_put(w, nbits, p.cl_len[dw_cl_order((int)i)], 3);
    dw_cl_walk(p.len, [&](uint32_t sym, uint32_t xb, uint32_t xv) {
        dw_put(w, nbits, p.cl_code[sym], p.cl_len[sym]);
        dw_put(w, nbits, xv, xb);
    });
    return nbits;
}
static constexpr uint32_t DW_HEADER_DWORDS = 64;      // 17 + 19 * 3 + 258 * 7 bits at the most

// ---- CRC-32 (the gzip polynomial, reflected) -----------------------------------------------------------------------------
static constexpr uint32_t DW_CRC_POLY = 0xEDB88320u;
SHK_HD uint32_t dw_crc_entry(uint32_t e) { uint32_t c = e; for (int k = 0; k < 8; k++) c = (c & 1u) ? DW_CRC_POLY ^ (c >> 1) : c >> 1; return c; }
// a * b modulo the polynomial; bit 31 of a word is x^0
SHK_HD uint32_t dw_gf_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; i++) { if (a & (0x80000000u >> i)) p ^= b; b = (b & 1u) ? (b >> 1) ^ DW_CRC_POLY : b >> 1; }
    return p;
}
// x^(8 n) modulo the polynomial
SHK_HD uint32_t dw_gf_x8n(uint64_t n) {
    uint32_t r = 0x80000000u, sq = 0x00800000u;      // x^0, x^8
    for (; n; n >>= 1) { if (n & 1u) r = dw_gf_mul(r, sq); sq = dw_gf_mul(sq, sq); }
    return r;
}
// CRC-32 of A followed by B, from the two (finished) checksums and the length of B
SHK_HD uint32_t dw_crc_join(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) { return dw_gf_mul(dw_gf_x8n(len_b), crc_a) ^ crc_b; }

// ---- the BGZF framing (SAM specification 4.1; the header sparrowhawk_amd/synth.py: bgzf_compress writes) -------------------
// byte i of a block's 18-byte header; total: the size of the whole block (BSIZE = total - 1)
SHK_HD uint8_t dw_bgzf_head_byte(uint32_t i, uint32_t total) {
    switch (i) {
        case 0: return 0x1f; case 1: return 0x8b; case 2: return 8; case 3: return 4;      // ID1 ID2 CM FLG = FEXTRA
        case 9: return 0xff;                                                              // OS: unknown
        case 10: return 6;                                                                // XLEN
        case 12: return 'B'; case 13: return 'C'; case 14: return 2;                      // the subfield, 2 bytes
        case 16: return (uint8_t)((total - 1u) & 0xFFu); case 17: return (uint8_t)((total - 1u) >> 8);
        default: return 0;
    }
}
// byte i of bgzip's empty end-of-file block
SHK_HD uint8_t dw_bgzf_eof_byte(uint32_t i) {
    if (i < 18) return dw_bgzf_head_byte(i, DW_EOF_BYTES);
    return i == 18 ? 3 : 0;                          // an empty fixed-code block (03 00), CRC-32 0, ISIZE 0
}
SHK_HD uint64_t dw_n_blocks(uint64_t n_text) { return (n_text + DW_BLOCK_TEXT - 1) / DW_BLOCK_TEXT; }

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host twin: one block's deflate data, and a whole file --------------------------------------------------------------
// out: room for DW_STORED_HEAD + n bytes + 8; returns the bytes written
inline uint32_t dw_host_block(const uint8_t *text, uint32_t n, uint8_t *out, uint32_t *crc_out) {
    static uint32_t tab[256]; static bool have = false;
    if (!have) { for (uint32_t e = 0; e < 256; e++) tab[e] = dw_crc_entry(e); have = true; }
    uint32_t counts[DW_LIT];
    for (int i = 0; i < DW_LIT; i++) counts[i] = 0;
    uint32_t crc = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < n; i++) { counts[text[i]]++; crc = tab[(crc ^ text[i]) & 0xFFu] ^ (crc >> 8); }
    *crc_out = crc ^ 0xFFFFFFFFu;
    counts[DW_EOB] = 1;
    DwScratch s; DwPlan p;
    dw_rank(counts, DW_LIT, s.order, 0, 1);
    dw_plan(counts, n, s, p);
    if (p.stored) {
        out[0] = 1; out[1] = (uint8_t)(n & 0xFF); out[2] = (uint8_t)(n >> 8); out[3] = (uint8_t)(~n & 0xFF); out[4] = (uint8_t)((~n >> 8) & 0xFF);
        for (uint32_t i = 0; i < n; i++) out[DW_STORED_HEAD + i] = text[i];
        return DW_STORED_HEAD + n;
    }
    uint32_t head[DW_HEADER_DWORDS + 2];
    for (uint32_t i = 0; i < DW_HEADER_DWORDS + 2; i++) head[i] = 0;
    const uint32_t hb = dw_put_header(p, head);
    uint64_t acc = 0; uint32_t have_bits = 0, at = 0;
    auto put = [&](uint32_t v, uint32_t nb) {
        acc |= (uint64_t)v << have_bits; have_bits += nb;
        while (have_bits >= 8) { out[at++] = (uint8_t)(acc & 0xFF); acc >>= 8; have_bits -= 8; }
    };
    for (uint32_t b = 0; b < hb; b += 16) { const uint32_t m = hb - b < 16 ? hb - b : 16; put((uint32_t)((((uint64_t)head[(b >> 5) + 1] << 32 | head[b >> 5]) >> (b & 31u)) & ((1u << m) - 1u)), m); }
    for (uint32_t i = 0; i < n; i++) put(p.code[text[i]], p.len[text[i]]);
    put(p.code[DW_EOB], p.len[DW_EOB]);
    if (have_bits) out[at++] = (uint8_t)(acc & 0xFF);
    return at;
}
// out: room for dw_host_file_bound(n) bytes; returns the size of the file
inline size_t dw_host_file_bound(size_t n) { return (size_t)dw_n_blocks(n) * (DW_BGZF_HEAD + DW_STORED_HEAD + DW_BGZF_TAIL) + n + DW_EOF_BYTES; }
inline size_t dw_host_file(const uint8_t *text, size_t n, uint8_t *out) {
    size_t at = 0;
    for (size_t o = 0; o < n; o += DW_BLOCK_TEXT) {
        const uint32_t m = (uint32_t)(n - o < DW_BLOCK_TEXT ? n - o : DW_BLOCK_TEXT);
        uint32_t crc = 0;
        const uint32_t body = dw_host_block(text + o, m, out + at + DW_BGZF_HEAD, &crc);
        const uint32_t total = DW_BGZF_HEAD + body + DW_BGZF_TAIL;
        for (uint32_t i = 0; i < DW_BGZF_HEAD; i++) out[at + i] = dw_bgzf_head_byte(i, total);
        uint8_t *t = out + at + DW_BGZF_HEAD + body;
        for (int i = 0; i < 4; i++) { t[i] = (uint8_t)(crc >> (8 * i)); t[4 + i] = (uint8_t)(m >> (8 * i)); }
        at += total;
    }
    for (uint32_t i = 0; i < DW_EOF_BYTES; i++) out[at++] = dw_bgzf_eof_byte(i);
    return at;
}
#endif

}  // namespace shk
