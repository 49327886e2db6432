// inflate_gpu.hip — see inflate_gpu.h.  One gzip member (one deflate stream), or a BGZF file (a chain of small ones),
// inflated on gfx950.
//
// The reference's real input is a `.fastq.gz` pair read through flate2's MultiGzDecoder
// (/root/reference/rust/orphos-bridge/src/fastx_wasm.rs:53-70; /root/reference/docs/src/assembly.md:25-28).  A deflate
// stream is serial by construction; the two-pass scheme of pugz / rapidgzip (restated for host threads in inflate_mt.cpp)
// makes it parallel, and thousands of chunks make it a GPU job:
//   k_gz_find_starts   one wave per cut of the compressed stream: 64 bit positions are tested at once (one per lane) for
//                      "a non-final dynamic-Huffman block starts here" — header fields, a complete code-length code, complete
//                      literal/length and distance codes with an end-of-block symbol, all from registers and a 128-byte
//                      per-lane table in LDS; a position that passes is probed by the whole wave (real tables, a few
//                      thousand symbols of the block: text bytes only, distances in range)
//   k_gz_decode        one wave per chunk, from its start to the next chunk's start, WITHOUT the 32 KiB window in front
//                      of it: 16-bit symbols, a back-reference into the unknown window is a MARKER (256 + position in that
//                      window).  The Huffman state is wave-uniform (every lane decodes the same symbol: tables in LDS,
//                      broadcast reads), the copy of a match is done by the 64 lanes together out of an LDS ring that holds
//                      the last 2048 symbols (RING; older ones from HBM); output leaves in coalesced 512-byte flushes
//                      (FLUSH = 256 symbols)
//   k_gz_win_init      the 32 KiB windows in front of the chunks: window c starts as the tail of chunk c - 1, and what is
//   k_gz_win_round     not known there (a marker, a chunk shorter than a window) points into the window in front of c - 1;
//                      round r replaces every pointer into the window 2^r chunks further front by what stands there after
//                      round r - 1 — ceil(log2(chunks)) rounds over all windows at once, no serial step
//   k_gz_resolve       markers -> bytes, 16 -> 8 bits, coalesced;  k_gz_crc  CRC-32 of 64 KiB slices (combined on the host)
// A BGZF (bgzip) file needs none of the speculation: every block is a deflate stream of its own of at most 64 KiB of text,
// with its compressed size in its header and CRC-32 and length of its text in its trailer (SAM specification 4.1):
//   k_bgzf_decode      one wave per non-empty block, the same wave-uniform decoder with its window known: BYTES, through a
//                      4 KiB ring in LDS, straight into the final text at the block's offset (the prefix sum of the lengths);
//                      nothing is produced or stored beyond the block's length, whatever its stream says
//   k_bgzf_crc         CRC-32 of every block's text against its trailer; one word comes back, not a checksum per block
//   k_last_record_start  a BGZF file window by window (BgzfWindows): where the last whole FASTQ record of a window's text ends —
//                      one wave walks the text's tail from the back, a ballot over the newlines of 64 bytes per step
//   k_fasta_header_search  the FASTA twin of the two record-start kernels (RecFmt::Fasta): a grid over the text, 16 bytes a lane,
//                      because a FASTA record is a contig or a chromosome and the search may cross megabytes
// Everything that does not look as expected makes gpu_inflate_member return 1 and the caller inflates on the host: the
// bytes handed on are always the bytes zlib would produce (CRC-32 and ISIZE of the trailer are checked here too).
#include <hip/hip_runtime.h>
#include <zlib.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <mutex>
#include <string>
#include <vector>

#include "inflate_gpu.h"
#include "fastq.h"

namespace shk {
namespace {

constexpr uint32_t GZ_WSIZE = 32768;
constexpr uint32_t GZ_MARK = 256;
constexpr int LIT_PB = 10, DIST_PB = 9, CL_PB = 7;
constexpr uint32_t RING = 2048, RING_MASK = RING - 1, NEAR = RING - 768, FLUSH = 256;
constexpr uint32_t PROBE_SYMS = 1024;

// ---- bit reader over the deflate data (32-bit words, zero-padded behind the end) ------------------------------------
struct DBits {
    const uint32_t *w; uint64_t nbytes;
    uint64_t byte; uint64_t buf; uint32_t cnt;
    __device__ __forceinline__ uint32_t load32(uint64_t at) const {
        const uint64_t i = at >> 2;
        const uint32_t a = w[i], b = w[i + 1], sh = (uint32_t)(at & 3u) * 8u;
        return sh ? (a >> sh) | (b << (32u - sh)) : a;
    }
    __device__ __forceinline__ void refill() { if (cnt <= 32u) { buf |= (uint64_t)load32(byte) << cnt; byte += 4; cnt += 32u; } }
    __device__ __forceinline__ void seek(uint64_t bitpos) { byte = bitpos >> 3; buf = 0; cnt = 0; refill(); refill(); drop((uint32_t)(bitpos & 7u)); }
    __device__ __forceinline__ uint32_t peek(uint32_t n) const { return (uint32_t)(buf & ((1ull << n) - 1ull)); }
    __device__ __forceinline__ void drop(uint32_t n) { buf >>= n; cnt -= n; }
    __device__ __forceinline__ uint32_t get(uint32_t n) { refill(); const uint32_t v = peek(n); drop(n); return v; }     // n <= 32
    __device__ __forceinline__ uint64_t pos() const { return byte * 8ull - cnt; }
    __device__ __forceinline__ bool overrun() const { return pos() > nbytes * 8ull; }
};

// The same stream read by a WAVE whose lanes all decode the same symbol (k_gz_decode, the probe): the next 64 dwords of the
// input sit one per lane in a register (fetched with one coalesced load, the 64 behind them already on their way), and
// a refill is a v_readlane — no memory latency on the symbol-to-symbol chain.
struct UBits {
    const uint32_t *w; uint64_t nbytes;
    uint32_t wbase, di;                       // dword index of the window's first word / of the next word to consume (input < 16 GiB)
    uint32_t lanew, lanew_next;
    uint64_t buf; uint32_t cnt;
    __device__ __forceinline__ uint32_t next_word() {
        uint32_t k = di - wbase;
        if (k >= 64u) { lanew = lanew_next; wbase += 64u; lanew_next = w[(size_t)wbase + 64u + threadIdx.x]; k -= 64u; }
        di++;
        return (uint32_t)__builtin_amdgcn_readlane((int)lanew, __builtin_amdgcn_readfirstlane((int)k));
    }
    __device__ __forceinline__ void refill() { if (cnt <= 32u) { buf |= (uint64_t)next_word() << cnt; cnt += 32u; } }
    __device__ __forceinline__ void seek(uint64_t bitpos) {
        wbase = (uint32_t)(bitpos >> 5); di = wbase; buf = 0; cnt = 0;
        lanew = w[(size_t)wbase + threadIdx.x]; lanew_next = w[(size_t)wbase + 64u + threadIdx.x];
        refill(); refill(); drop((uint32_t)(bitpos & 31u));
    }
    __device__ __forceinline__ uint32_t peek(uint32_t n) const { return (uint32_t)buf & ((1u << n) - 1u); }              // n < 32
    __device__ __forceinline__ void drop(uint32_t n) { buf >>= n; cnt -= n; }
    __device__ __forceinline__ uint32_t get(uint32_t n) { refill(); const uint32_t v = peek(n); drop(n); return v; }     // n < 32
    __device__ __forceinline__ uint64_t pos() const { return (uint64_t)di * 32ull - cnt; }
    __device__ __forceinline__ bool overrun() const { return pos() > nbytes * 8ull; }
};
// length / distance codes -> base value and extra bits, by arithmetic (RFC 1951 3.2.5; a table in constant memory costs a
// scalar load — hundreds of cycles — per lookup on the symbol-to-symbol chain)
__device__ __forceinline__ void len_code(uint32_t c, uint32_t &base, uint32_t &extra) {       // c = symbol - 257, 0 .. 28
    if (c < 8u) { base = 3u + c; extra = 0; }
    else if (c == 28u) { base = 258u; extra = 0; }
    else { extra = (c >> 2) - 1u; base = 3u + ((4u + (c & 3u)) << extra); }
}
__device__ __forceinline__ void dist_code(uint32_t d, uint32_t &base, uint32_t &extra) {      // d = 0 .. 29
    if (d < 4u) { base = 1u + d; extra = 0; }
    else { extra = (d >> 1) - 1u; base = 1u + ((2u + (d & 1u)) << extra); }
}
// the order in which a dynamic block lists the lengths of its code-length code (16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15), 5 bits each
__device__ __forceinline__ uint32_t cl_order(uint32_t i) {
    const unsigned long long lo = 16ull | (17ull << 5) | (18ull << 10) | (0ull << 15) | (8ull << 20) | (7ull << 25) | (9ull << 30) | (6ull << 35) | (10ull << 40) | (5ull << 45) | (11ull << 50) | (4ull << 55);
    const unsigned long long hi = 12ull | (3ull << 5) | (13ull << 10) | (2ull << 15) | (14ull << 20) | (1ull << 25) | (15ull << 30);
    return i < 12u ? (uint32_t)(lo >> (5u * i)) & 31u : (uint32_t)(hi >> (5u * (i - 12u))) & 31u;
}

// ---- canonical Huffman tables of one wave in LDS ---------------------------------------------------------------------
struct HuffLds {
    uint16_t lit_tab[1 << LIT_PB];           // symbol << 4 | code length; 0: a code longer than the table's index
    uint16_t dist_tab[1 << DIST_PB];
    uint16_t cl_tab[1 << CL_PB];
    uint16_t lit_sym[288], dist_sym[32], cl_sym[20];
    uint32_t lit_count[16], dist_count[16], cl_count[16];
    uint32_t lit_maxlen, dist_maxlen, cl_maxlen;
    uint8_t len[328];                        // code lengths of the block being set up
};
struct WaveLds {
    HuffLds h;
    uint16_t ring[RING];                     // the last RING symbols of the chunk's output
};

// Builds the decoding table of one code from len[0..n) (wave-cooperative; one wave per workgroup).  Returns false unless
// the lengths form a complete prefix code (or, allow_single, exactly one code of length 1).
__device__ bool build_code(const uint8_t *len, uint32_t n, bool allow_single, uint16_t *tab, int PB, uint32_t *count,
                           uint16_t *symbol, uint32_t *maxlen_out) {
    const int lane = threadIdx.x;
    if (lane < 16) count[lane] = 0;
    for (uint32_t f = lane; f < (1u << PB); f += 64) tab[f] = 0;
    __syncthreads();
    for (uint32_t i = lane; i < n; i += 64) { const uint32_t l = len[i]; if (l) atomicAdd(&count[l], 1u); }
    __syncthreads();
    uint32_t used = 0, maxlen = 0; int left = 1; bool over = false;
    for (uint32_t l = 1; l < 16; l++) { const uint32_t cl = count[l]; used += cl; if (cl) maxlen = l; left = left * 2 - (int)cl; if (left < 0) over = true; }
    if (!used || over) return false;
    if (left > 0 && !(allow_single && used == 1 && count[1] == 1)) return false;
    // symbols in canonical order: by length, then by value
    uint32_t off = 0;
    for (uint32_t l = 1; l <= maxlen; l++) {
        for (uint32_t base = 0; base < n; base += 64) {
            const uint32_t i = base + lane;
            const bool has = i < n && len[i] == l;
            const unsigned long long m = __ballot(has);
            if (has) symbol[off + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)i;
            off += (uint32_t)__popcll(m);
        }
    }
    __syncthreads();
    // table of the codes up to PB bits (deflate codes are packed LSB first: reversed bit order)
    for (uint32_t idx = lane; idx < used; idx += 64) {
        uint32_t l = 1, start = 0, code = 0;
        for (uint32_t q = 1; q < 15; q++) { const uint32_t cq = count[q]; if (idx < start + cq) break; start += cq; code = (code + cq) << 1; l = q + 1; }
        if (l > (uint32_t)PB) continue;
        const uint32_t cw = code + (idx - start);
        const uint32_t rev = __brev(cw) >> (32u - l);
        const uint16_t e = (uint16_t)((symbol[idx] << 4) | l);
        for (uint32_t f = rev; f < (1u << PB); f += 1u << l) tab[f] = e;
    }
    if (lane == 0) *maxlen_out = maxlen;
    __syncthreads();
    return true;
}

// one symbol (wave-uniform: every lane runs this on the same state); -1: no such code
__device__ __forceinline__ int decode_sym(UBits &b, const uint16_t *tab, int PB, const uint32_t *count, const uint16_t *symbol, uint32_t maxlen) {
    // (every lane reads the same entry: readfirstlane tells the compiler so, and the Huffman state — bit buffer, counters,
    // positions — lives in scalar registers and is worked on by the scalar unit, not 64 times over by the vector unit)
    const uint32_t e = (uint32_t)__builtin_amdgcn_readfirstlane((int)tab[b.peek((uint32_t)PB)]);
    if (e & 15u) { b.drop(e & 15u); return (int)(e >> 4); }
    uint32_t code = 0, first = 0, index = 0;
    uint64_t v = b.buf;
    for (uint32_t l = 1; l <= maxlen; l++) {
        code |= (uint32_t)(v & 1u); v >>= 1;
        const uint32_t cc = (uint32_t)__builtin_amdgcn_readfirstlane((int)count[l]);
        if (code < first + cc) { if (l > b.cnt) return -1; b.drop(l); return __builtin_amdgcn_readfirstlane((int)symbol[index + (code - first)]); }
        index += cc; first += cc; first <<= 1; code <<= 1;
    }
    return -1;
}

// a dynamic block's code definitions at the reader's position -> tables (wave-uniform); false: not a valid header
__device__ bool read_dynamic(UBits &b, HuffLds &h) {
    const int lane = threadIdx.x;
    const uint32_t hlit = b.get(5) + 257, hdist = b.get(5) + 1, hclen = b.get(4) + 4;
    if (hlit > 286 || hdist > 30) return false;
    if (lane < 19) h.len[lane] = 0;
    __syncthreads();
    for (uint32_t i = 0; i < hclen; i++) { const uint32_t v = b.get(3); if (lane == 0) h.len[cl_order(i)] = (uint8_t)v; }
    __syncthreads();
    if (!build_code(h.len, 19, true, h.cl_tab, CL_PB, h.cl_count, h.cl_sym, &h.cl_maxlen)) return false;
    const uint32_t cl_maxlen = (uint32_t)__builtin_amdgcn_readfirstlane((int)h.cl_maxlen);
    __syncthreads();                                           // (h.len is rewritten below)
    uint32_t i = 0, prev = 0;
    const uint32_t total = hlit + hdist;
    while (i < total) {
        b.refill();
        const int s = decode_sym(b, h.cl_tab, CL_PB, h.cl_count, h.cl_sym, cl_maxlen);
        if (s < 0 || b.overrun()) return false;
        if (s < 16) { if (lane == 0) h.len[i] = (uint8_t)s; prev = (uint32_t)s; i++; continue; }
        uint32_t rep, val = 0;
        if (s == 16) { if (i == 0) return false; val = prev; rep = 3 + b.get(2); }
        else if (s == 17) rep = 3 + b.get(3);
        else rep = 11 + b.get(7);
        if (i + rep > total) return false;
        for (uint32_t q = lane; q < rep; q += 64) h.len[i + q] = (uint8_t)val;
        i += rep; prev = val;
    }
    __syncthreads();
    if (h.len[256] == 0) return false;                          // no end-of-block code
    if (!build_code(h.len, hlit, false, h.lit_tab, LIT_PB, h.lit_count, h.lit_sym, &h.lit_maxlen)) return false;
    if (!build_code(h.len + hlit, hdist, true, h.dist_tab, DIST_PB, h.dist_count, h.dist_sym, &h.dist_maxlen)) {
        // (a block without any distance code is legal: all its lengths are zero)
        bool none = true;
        for (uint32_t d = 0; d < hdist; d++) none = none && h.len[hlit + d] == 0;
        if (!none) return false;
        for (uint32_t f = lane; f < (1u << DIST_PB); f += 64) h.dist_tab[f] = 0;
        if (lane < 16) h.dist_count[lane] = 0;
        if (lane == 0) h.dist_maxlen = 0;
        __syncthreads();
    }
    return true;
}
__device__ void fixed_codes(HuffLds &h) {
    const int lane = threadIdx.x;
    for (uint32_t i = lane; i < 288; i += 64) h.len[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
    __syncthreads();
    (void)build_code(h.len, 288, false, h.lit_tab, LIT_PB, h.lit_count, h.lit_sym, &h.lit_maxlen);
    // the fixed distance code is incomplete (30 of 32 five-bit codes): the table is filled directly
    for (uint32_t f = lane; f < (1u << DIST_PB); f += 64) {
        const uint32_t s = __brev(f & 31u) >> 27;
        h.dist_tab[f] = s < 30 ? (uint16_t)((s << 4) | 5u) : (uint16_t)0;
    }
    if (lane < 16) h.dist_count[lane] = 0;
    if (lane == 0) h.dist_maxlen = 0;
    __syncthreads();
}

__device__ __forceinline__ bool text_byte(uint32_t c) { return (c >= 0x20 && c < 0x7F) || c == '\n' || c == '\r' || c == '\t'; }

// ---- the wave probes ONE candidate position: a real dynamic block of text?  (k_gz_find_starts) ------------------------
struct ProbeLds { HuffLds h; };
__device__ bool probe_block(const uint32_t *w, uint64_t nbytes, uint64_t p, ProbeLds &L) {
    UBits b; b.w = w; b.nbytes = nbytes;
    b.seek(p);
    const uint32_t bfinal = b.get(1), btype = b.get(2);
    if (bfinal != 0 || btype != 2) return false;
    if (!read_dynamic(b, L.h)) return false;
    const uint32_t lit_max = (uint32_t)__builtin_amdgcn_readfirstlane((int)L.h.lit_maxlen), dist_max = (uint32_t)__builtin_amdgcn_readfirstlane((int)L.h.dist_maxlen);
    uint32_t produced = 0, nsym = 0;
    for (;;) {
        b.refill();
        const int s = decode_sym(b, L.h.lit_tab, LIT_PB, L.h.lit_count, L.h.lit_sym, lit_max);
        if (s < 0 || b.overrun()) return false;
        nsym++;
        if (s < 256) { if (!text_byte((uint32_t)s)) return false; produced++; }
        else if (s == 256) {
            if (nsym < 64) return false;                        // (a real block of a FASTQ stream holds thousands of symbols)
            const uint32_t nb = b.get(3);                       // the next header must make sense too
            return (nb >> 1) != 3 && !b.overrun();
        } else {
            if (s > 285) return false;
            uint32_t lb, le; len_code((uint32_t)s - 257u, lb, le);
            const uint32_t len = lb + b.get(le);
            b.refill();
            const int ds = decode_sym(b, L.h.dist_tab, DIST_PB, L.h.dist_count, L.h.dist_sym, dist_max);
            if (ds < 0 || ds > 29) return false;
            uint32_t db, de; dist_code((uint32_t)ds, db, de);
            const uint32_t dist = db + b.get(de);
            if (b.overrun() || dist > produced + GZ_WSIZE) return false;
            produced += len;
        }
        if (nsym >= PROBE_SYMS) return true;
    }
}

// per lane: does a dynamic block header at bit position p hold complete codes?  (registers + a 128-byte table of the
// code-length code per lane: cl_tab[entry][lane])
__device__ bool header_plausible(const uint32_t *w, uint64_t nbytes, uint64_t p, uint8_t (*cl_tab)[64]) {
    const int lane = threadIdx.x;
    if ((p >> 3) + 16 >= nbytes) return false;
    // 96 bits from p: the 17 header bits and up to 19 x 3 bits of code-length code lengths
    const uint64_t wi = p >> 5; const uint32_t sh = (uint32_t)(p & 31u);
    const uint32_t d0 = w[wi], d1 = w[wi + 1], d2 = w[wi + 2], d3 = w[wi + 3];
    const uint32_t e0 = sh ? (d0 >> sh) | (d1 << (32u - sh)) : d0, e1 = sh ? (d1 >> sh) | (d2 << (32u - sh)) : d1, e2 = sh ? (d2 >> sh) | (d3 << (32u - sh)) : d2;
    // BFINAL = 0, BTYPE = 2 (bits 0, then 0 1 LSB first: value 4 over three bits), HLIT <= 286, HDIST <= 30
    if ((e0 & 7u) != 4u || ((e0 >> 3) & 31u) > 29u || ((e0 >> 8) & 31u) > 29u) return false;
    const uint32_t hlit = ((e0 >> 3) & 31u) + 257u, hdist = ((e0 >> 8) & 31u) + 1u, hclen = ((e0 >> 13) & 15u) + 4u;
    // the lengths of the code-length code, in the order of the stream: is the code complete?  (the order does not matter for that)
    const uint64_t raw = (((uint64_t)e1 << 32 | e0) >> 17) | ((uint64_t)e2 << 47);
    uint32_t kraft = 0, used = 0;
    for (uint32_t i = 0; i < hclen; i++) { const uint32_t l = (uint32_t)(raw >> (3u * i)) & 7u; if (l) { kraft += 128u >> l; used++; } }
    if (kraft != 128u || used < 2) return false;                // complete (a single code of length 1 is left to the chunk before)
    uint64_t clv = 0;                                           // ... now by symbol: 19 lengths of 3 bits in one register
    for (uint32_t i = 0; i < hclen; i++) clv |= (uint64_t)((uint32_t)(raw >> (3u * i)) & 7u) << (3u * cl_order(i));
    DBits b{w, nbytes, 0, 0, 0};
    b.seek(p + 17u + 3u * hclen);
    // canonical codes -> the lane's 7-bit table (a complete code fills every entry)
    uint64_t next = 0;                                          // next code of length l in byte l
    {
        uint32_t code = 0;
        for (uint32_t l = 1; l <= 7; l++) {
            uint32_t cnt = 0;
            for (uint32_t s = 0; s < 19; s++) cnt += ((uint32_t)(clv >> (3u * s)) & 7u) == l;
            next |= (uint64_t)code << (8u * l);
            code = (code + cnt) << 1;
        }
    }
    for (uint32_t s = 0; s < 19; s++) {
        const uint32_t l = (uint32_t)(clv >> (3u * s)) & 7u;
        if (!l) continue;
        const uint32_t code = (uint32_t)(next >> (8u * l)) & 0xFFu;
        next += 1ull << (8u * l);
        const uint32_t rev = __brev(code) >> (32u - l);
        for (uint32_t f = rev; f < 128u; f += 1u << l) cl_tab[f][lane] = (uint8_t)((s << 3) | l);
    }
    // the literal/length and distance code lengths: only their Kraft sums, the end-of-block code and the counts are kept
    uint32_t i = 0, prev = 0, kl = 0, kd = 0, nd = 0, d_single = 0;
    bool has256 = false;
    const uint32_t total = hlit + hdist;
    auto put = [&](uint32_t at, uint32_t l) {
        if (!l) return;
        if (at < hlit) { kl += 32768u >> l; if (at == 256) has256 = true; }
        else { kd += 32768u >> l; nd++; d_single = l; }
    };
    // (random bits over-subscribe a code within a few dozen lengths: the walk over ~300 lengths ends there)
    while (i < total) {
        b.refill();
        const uint32_t e = cl_tab[b.peek(7)][lane];
        const uint32_t s = e >> 3;
        b.drop(e & 7u);
        if (b.overrun()) return false;
        if (s < 16) { put(i, s); prev = s; i++; if (kl > 32768u || kd > 32768u) return false; continue; }
        uint32_t rep, val = 0;
        if (s == 16) { if (i == 0) return false; val = prev; rep = 3 + b.get(2); }
        else if (s == 17) rep = 3 + b.get(3);
        else rep = 11 + b.get(7);
        if (i + rep > total) return false;
        for (uint32_t q = 0; q < rep; q++) put(i + q, val);
        i += rep; prev = val;
        if (kl > 32768u || kd > 32768u) return false;
    }
    if (!has256 || kl != 32768u) return false;
    if (!(kd == 32768u || nd == 0 || (nd == 1 && d_single == 1))) return false;
    return true;
}

// start[c] (c >= 1): the first bit position >= cut[c] (< cut[c + 1]) where a non-final dynamic block of text starts; ~0: none
__global__ __launch_bounds__(64) void k_gz_find_starts(const uint32_t *__restrict__ w, uint64_t nbytes, uint64_t chunk_bytes, uint32_t n_chunks,
                                                      unsigned long long *__restrict__ start) {
    __shared__ ProbeLds L;
    __shared__ uint8_t cl_tab[128][64];
    const uint32_t c = blockIdx.x + 1;
    if (c >= n_chunks) return;
    const int lane = threadIdx.x;
    const uint64_t from = (uint64_t)c * chunk_bytes * 8ull, limit = min((uint64_t)(c + 1) * chunk_bytes * 8ull, nbytes * 8ull);
    unsigned long long found = ~0ull;
    for (uint64_t base = from; base < limit && found == ~0ull; base += 64) {
        const uint64_t p = base + (uint64_t)lane;
        const bool ok = p < limit && header_plausible(w, nbytes, p, cl_tab);
        unsigned long long m = __ballot(ok);
        while (m) {
            const int l = __ffsll((long long)m) - 1;
            m &= m - 1;
            if (probe_block(w, nbytes, base + (uint64_t)l, L)) { found = base + (uint64_t)l; break; }
            __syncthreads();
        }
    }
    if (lane == 0) start[c] = found;
}

// ---- decode one chunk ------------------------------------------------------------------------------------------------
enum : uint32_t { GZ_FINAL = 1, GZ_ATSTOP = 2, GZ_OVERSHOOT = 3, GZ_CORRUPT = 4, GZ_NO_ROOM = 5 };
struct ChunkOut { unsigned long long n_sym, end_pos; uint32_t status, pad; };

__global__ __launch_bounds__(64) void k_gz_decode(const uint32_t *__restrict__ w, uint64_t nbytes, uint32_t n_chunks,
                                                 const unsigned long long *__restrict__ start, const unsigned long long *__restrict__ sym_off,
                                                 uint16_t *__restrict__ syms, ChunkOut *__restrict__ res) {
    __shared__ WaveLds L;
    const uint32_t c = blockIdx.x;
    if (c >= n_chunks) return;
    const uint32_t lane = threadIdx.x;
    const uint64_t stop_at = c + 1 < n_chunks ? start[c + 1] : ~0ull;
    uint16_t *out = syms + sym_off[c];
    const uint64_t room64 = sym_off[c + 1] - sym_off[c];
    const uint32_t room = (uint32_t)(room64 > 0xFFFF0000ull ? 0xFFFF0000ull : room64);
    const bool known_window = c == 0;
    UBits b; b.w = w; b.nbytes = nbytes;
    b.seek(start[c]);
    uint32_t pos = 0, flushed = 0;                               // symbols produced / already in HBM (a multiple of FLUSH)
    uint32_t status = 0;
    // whenever FLUSH symbols have piled up: out they go (coalesced), and the two checks that need not run per symbol are made:
    // room for what may come before the next flush, and a reader that has not left the input (it is zero-padded far enough
    // for what can be read in between)
    auto flush_full = [&]() -> bool {
        while (pos - flushed >= FLUSH) {
            const uint32_t *r32 = reinterpret_cast<const uint32_t *>(L.ring);
            uint32_t *o32 = reinterpret_cast<uint32_t *>(out + flushed);
            const uint32_t at = (flushed & RING_MASK) >> 1;
#pragma unroll
            for (uint32_t t = 0; t < FLUSH / 2 / 64; t++) o32[t * 64 + lane] = r32[at + t * 64 + lane];
            flushed += FLUSH;
            // (symbols this far back are read from HBM again by far matches — by lanes of this same wave: the stores have to be
            // complete, nothing has to leave the L2)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        }
        if (pos + 2048u > room) { status = GZ_NO_ROOM; return false; }
        if (b.overrun()) { status = GZ_CORRUPT; return false; }
        return true;
    };
    for (;;) {
        if (b.pos() == stop_at) { status = GZ_ATSTOP; break; }
        if (b.pos() > stop_at) { status = GZ_OVERSHOOT; break; }
        const uint32_t bfinal = b.get(1), btype = b.get(2);
        if (b.overrun() || btype == 3) { status = GZ_CORRUPT; break; }
        if (btype == 0) {
            b.drop(b.cnt & 7u);                                  // to the byte boundary
            const uint32_t len = b.get(16), nlen = b.get(16);
            if ((len ^ nlen) != 0xFFFFu || b.overrun()) { status = GZ_CORRUPT; break; }
            bool ok = true;
            for (uint32_t i = 0; i < len && ok; i++) {
                const uint32_t v = b.get(8);
                L.ring[pos & RING_MASK] = (uint16_t)v;
                pos++;
                if (pos - flushed >= FLUSH) ok = flush_full();
            }
            if (!ok) break;
            if (b.overrun()) { status = GZ_CORRUPT; break; }
        } else {
            if (btype == 1) fixed_codes(L.h);
            else if (!read_dynamic(b, L.h)) { status = GZ_CORRUPT; break; }
            const uint32_t lit_max = (uint32_t)__builtin_amdgcn_readfirstlane((int)L.h.lit_maxlen), dist_max = (uint32_t)__builtin_amdgcn_readfirstlane((int)L.h.dist_maxlen);
            bool bad = false;
            for (;;) {
                b.refill();
                const int s = decode_sym(b, L.h.lit_tab, LIT_PB, L.h.lit_count, L.h.lit_sym, lit_max);
                if (s < 0) { bad = true; break; }
                if (s < 256) {
                    L.ring[pos & RING_MASK] = (uint16_t)s;
                    pos++;
                    if (pos - flushed >= FLUSH) { if (!flush_full()) break; }
                    continue;
                }
                if (s == 256) break;
                if (s > 285) { bad = true; break; }
                uint32_t lb, le; len_code((uint32_t)s - 257u, lb, le);
                const uint32_t len = lb + b.get(le);
                b.refill();
                const int ds = decode_sym(b, L.h.dist_tab, DIST_PB, L.h.dist_count, L.h.dist_sym, dist_max);
                if (ds < 0 || ds > 29) { bad = true; break; }
                uint32_t db, de; dist_code((uint32_t)ds, db, de);
                const uint32_t dist = db + b.get(de);
                if ((dist > pos && known_window) || dist > pos + GZ_WSIZE) { bad = true; break; }
                // the copy, by all lanes: position pos + i takes what stands dist back — periodic when the match overlaps itself,
                // so every source lies in front of pos and the lanes do not depend on one another
                for (uint32_t i = lane; i < len; i += 64) {
                    const uint32_t j = i < dist ? i : i % dist;
                    const int src = (int)pos - (int)dist + (int)j;
                    uint16_t v;
                    if (src < 0) v = (uint16_t)(GZ_MARK + (GZ_WSIZE + src));
                    else if (pos - (uint32_t)src <= NEAR) v = L.ring[(uint32_t)src & RING_MASK];
                    else v = out[src];
                    L.ring[(pos + i) & RING_MASK] = v;
                }
                pos += len;
                if (pos - flushed >= FLUSH) { if (!flush_full()) break; }
            }
            if (status) break;
            if (bad) { status = GZ_CORRUPT; break; }
        }
        if (bfinal) { status = GZ_FINAL; break; }
    }
    // what is left in the ring
    for (uint32_t p = flushed + lane; p < pos; p += 64) out[p] = L.ring[p & RING_MASK];
    if (lane == 0) { ChunkOut r; r.n_sym = pos; r.end_pos = b.pos(); r.status = status; r.pad = 0; res[c] = r; }
}

// ---- the windows in front of the chunks ----------------------------------------------------------------------------------
// M[c][j] (c >= 1, j < 32768): byte j of the 32 KiB in front of chunk c (= the last 32768 bytes of everything before it), or
// — not known yet — 256 + a position in the window that many chunks FURTHER FRONT.  k_gz_win_init takes it from the tail
// of chunk c - 1 (a marker there, or a chunk shorter than a window, points into the window in front of c - 1); round r of
// k_gz_win_round replaces every pointer into the window of chunk c - 2^r by what stands there after round r - 1: a byte, or a
// pointer into the window of chunk c - 2^(r+1).  In FASTQ text a marker lives for ever (a quality line is a copy of the one
// before, back to the stream's first), so the chain of dependencies runs through ALL chunks: walked front to back by one
// workgroup it cost 6 us per chunk (24 ms for 4030 chunks); ceil(log2(chunks)) rounds over all windows at once cost ~3.
__global__ __launch_bounds__(1024) void k_gz_win_init(const uint16_t *__restrict__ syms, const unsigned long long *__restrict__ sym_off,
                                                     const ChunkOut *__restrict__ res, uint32_t n_chunks, uint16_t *__restrict__ M) {
    const uint32_t c = blockIdx.x + 1;
    if (c >= n_chunks) return;
    const uint16_t *S = syms + sym_off[c - 1];
    const long long n = (long long)res[c - 1].n_sym;
    uint16_t *W = M + (size_t)c * GZ_WSIZE;
    for (uint32_t j = threadIdx.x; j < GZ_WSIZE; j += 1024) {
        const long long i = n - (long long)GZ_WSIZE + (long long)j;
        W[j] = i >= 0 ? S[i] : (uint16_t)(GZ_MARK + (uint32_t)((long long)j + n));      // the chunk is shorter than a window: the rest comes from ITS window
    }
}
__global__ __launch_bounds__(1024) void k_gz_win_round(const uint16_t *__restrict__ Min, uint16_t *__restrict__ Mout, uint32_t n_chunks, uint32_t step) {
    const uint32_t c = blockIdx.x + 1;
    if (c >= n_chunks) return;
    const uint16_t *A = Min + (size_t)c * GZ_WSIZE;
    uint16_t *O = Mout + (size_t)c * GZ_WSIZE;
    const bool have_src = c > step;                            // window c - step exists (there is none in front of chunk 0)
    const uint16_t *B = Min + (size_t)(have_src ? c - step : 0) * GZ_WSIZE;
    for (uint32_t j = threadIdx.x; j < GZ_WSIZE; j += 1024) {
        uint32_t e = A[j];
        // (no window c - step: a byte in front of the stream's first.  The entry stays a pointer; k_gz_resolve refuses its use)
        if (e >= GZ_MARK && have_src) e = B[(e - GZ_MARK) & (GZ_WSIZE - 1)];
        O[j] = (uint16_t)e;
    }
}

// markers -> bytes: text[out_off[c] + i] = symbol < 256 ? symbol : window c [symbol - 256]   (grid: x over a chunk, y = chunk)
__global__ __launch_bounds__(256) void k_gz_resolve(const uint16_t *__restrict__ syms, const unsigned long long *__restrict__ sym_off,
                                                   const ChunkOut *__restrict__ res, const unsigned long long *__restrict__ out_off,
                                                   const uint16_t *__restrict__ M, uint8_t *__restrict__ text, uint32_t *__restrict__ bad) {
    const uint32_t c = blockIdx.y;
    const uint16_t *S = syms + sym_off[c];
    const unsigned long long n = res[c].n_sym;
    const uint16_t *W = M + (size_t)c * GZ_WSIZE;
    uint8_t *T = text + out_off[c];
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256u) {
        uint32_t s = S[i];
        if (s >= GZ_MARK) {
            if (c == 0) { atomicOr(bad, 2u); s = 0; }
            else { s = W[(s - GZ_MARK) & (GZ_WSIZE - 1)]; if (s >= GZ_MARK) { atomicOr(bad, 4u); s = 0; } }      // (a byte in front of the stream's first: k_gz_win_round)
        }
        T[i] = (uint8_t)s;
    }
}

// CRC-32 (the gzip polynomial, reflected) of slices of `slice` bytes: one thread per slice, byte-wise table in LDS
__global__ __launch_bounds__(256) void k_gz_crc(const uint8_t *__restrict__ text, unsigned long long n, uint32_t slice, uint32_t n_slices,
                                               uint32_t *__restrict__ crc_out) {
    __shared__ uint32_t tab[256];
    {
        uint32_t cc = threadIdx.x;
        for (int k = 0; k < 8; k++) cc = (cc & 1u) ? 0xEDB88320u ^ (cc >> 1) : cc >> 1;
        tab[threadIdx.x] = cc;
    }
    __syncthreads();
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= n_slices) return;
    const unsigned long long a = (unsigned long long)s * slice, e = min(n, a + slice);
    uint32_t crc = 0xFFFFFFFFu;
    unsigned long long p = a;
    // 16 bytes per load (slices start 16-byte aligned: `slice` is a multiple of 16 and the text block is aligned)
    for (; p + 16 <= e; p += 16) {
        const uint4 v = *reinterpret_cast<const uint4 *>(text + p);
        const uint32_t ws[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 4; q++) {
            uint32_t x = ws[q];
#pragma unroll
            for (int r = 0; r < 4; r++) { crc = tab[(crc ^ x) & 0xFFu] ^ (crc >> 8); x >>= 8; }
        }
    }
    for (; p < e; p++) crc = tab[(crc ^ text[p]) & 0xFFu] ^ (crc >> 8);
    crc_out[s] = crc ^ 0xFFFFFFFFu;
}

// ---- BGZF (bgzip): a chain of independent deflate streams of <= 64 KiB of text each --------------------------------------
// Every block announces its compressed size in its header and carries CRC-32 and length (ISIZE) of its text in its trailer
// (SAM specification 4.1), so nothing is searched for and nothing is unknown: no markers, no windows, no second pass.  One
// wave per non-empty block decodes BYTES into an LDS ring and writes them straight into the final text at the block's
// offset (the prefix sum of the ISIZE fields).  The blocks' texts lie back to back, so bounds hold by construction: nothing
// is produced at or beyond ISIZE, and no store touches a byte outside [out_off, out_off + ISIZE).
constexpr uint32_t BZ_RING = 4096, BZ_MASK = BZ_RING - 1, BZ_NEAR = BZ_RING - 512, BZ_GROUP = 256;
enum : uint32_t { BZ_GOOD = 1, BZ_FINAL = 2, BZ_CORRUPT = 3, BZ_TOO_LONG = 4, BZ_TOO_SHORT = 5, BZ_NOT_AT_END = 6 };
struct BgzfDesc { unsigned long long in_off; uint32_t in_len, out_off, isize, crc; };      // deflate bytes in the file / text
struct BgzfLds {
    HuffLds h;
    alignas(4) uint8_t ring[BZ_RING];        // the block's last BZ_RING bytes, indexed by their address in the text (mod BZ_RING)
};

// bad[0]: the first block (atomicMin) that is not good; status[blk]: why
__global__ __launch_bounds__(64) void k_bgzf_decode(const uint32_t *__restrict__ w, const BgzfDesc *__restrict__ desc, uint32_t n_blocks,
                                                   uint8_t *text, uint32_t *__restrict__ status_out, uint32_t *__restrict__ bad) {
    __shared__ BgzfLds L;
    const uint32_t blk = blockIdx.x;
    if (blk >= n_blocks) return;
    const uint32_t lane = threadIdx.x;
    const BgzfDesc d = desc[blk];
    const uint32_t isize = d.isize, a32 = d.out_off;
    const uint64_t in_end = d.in_off + d.in_len;
    uint8_t *out = text + d.out_off;
    UBits b; b.w = w; b.nbytes = in_end;                        // (overrun(): the reader has left THIS block's deflate data)
    b.seek(d.in_off * 8ull);
    uint32_t pos = 0, flushed = 0;                              // bytes produced / already in HBM
    uint32_t status = 0;
    // bytes [lo, hi) of the block, all inside one aligned group of BZ_GROUP bytes of the text, ring -> HBM.  A lane owns one
    // aligned dword of the group: stored whole if it lies inside [lo, hi), byte by byte where the range starts or ends inside
    // it (the neighbouring blocks' waves write the other bytes of such a dword)
    auto store_range = [&](uint32_t lo, uint32_t hi) {
        const uint32_t g = ((a32 + lo) & ~(BZ_GROUP - 1u)) + 4u * lane;      // this lane's dword: its address in the text ...
        const int r = (int)(g - a32);                                      // ... and in the block (may lie in front of it)
        if (r >= (int)lo && r + 4 <= (int)hi) *reinterpret_cast<uint32_t *>(out + r) = *reinterpret_cast<const uint32_t *>(&L.ring[g & BZ_MASK]);
        else {
#pragma unroll
            for (int q = 0; q < 4; q++) if (r + q >= (int)lo && r + q < (int)hi) out[r + q] = L.ring[(g + (uint32_t)q) & BZ_MASK];
        }
    };
    auto group_end = [&](uint32_t at) { return at + BZ_GROUP - ((a32 + at) & (BZ_GROUP - 1u)); };
    // whenever BZ_GROUP bytes have piled up: out go the groups that are complete, and the reader is checked (the input is
    // zero-padded far enough for what can be read in between)
    auto flush_full = [&]() -> bool {
        for (uint32_t e = group_end(flushed); e <= pos; e = group_end(flushed)) { store_range(flushed, e); flushed = e; }
        // (bytes this far back are read from HBM again by far matches — by lanes of this same wave: the stores have to be complete)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        if (b.overrun()) { status = BZ_CORRUPT; return false; }
        return true;
    };
    for (;;) {
        const uint32_t bfinal = b.get(1), btype = b.get(2);
        if (b.overrun() || btype == 3) { status = BZ_CORRUPT; break; }
        if (btype == 0) {
            b.drop(b.cnt & 7u);                                  // to the byte boundary
            const uint32_t len = b.get(16), nlen = b.get(16);
            if ((len ^ nlen) != 0xFFFFu || b.overrun()) { status = BZ_CORRUPT; break; }
            uint64_t at = b.pos() >> 3;                          // the stored bytes: copied by the lanes, 256 at a time
            if (at + len > in_end) { status = BZ_CORRUPT; break; }
            if (len > isize - pos) { status = BZ_TOO_LONG; break; }
            const uint8_t *in8 = reinterpret_cast<const uint8_t *>(w);
            for (uint32_t left = len; left;) {
                const uint32_t m = left < BZ_GROUP ? left : BZ_GROUP;
                for (uint32_t i = lane; i < m; i += 64) L.ring[(a32 + pos + i) & BZ_MASK] = in8[at + i];
                pos += m; at += m; left -= m;
                if (pos - flushed >= BZ_GROUP) (void)flush_full();   // (the reader stands still: it cannot fail here)
            }
            b.seek(at * 8ull);
        } else {
            if (btype == 1) fixed_codes(L.h);
            else if (!read_dynamic(b, L.h)) { status = BZ_CORRUPT; break; }
            const uint32_t lit_max = (uint32_t)__builtin_amdgcn_readfirstlane((int)L.h.lit_maxlen), dist_max = (uint32_t)__builtin_amdgcn_readfirstlane((int)L.h.dist_maxlen);
            bool bad_code = false;
            for (;;) {
                b.refill();
                const int s = decode_sym(b, L.h.lit_tab, LIT_PB, L.h.lit_count, L.h.lit_sym, lit_max);
                if (s < 0) { bad_code = true; break; }
                if (s < 256) {
                    if (pos >= isize) { status = BZ_TOO_LONG; break; }
                    L.ring[(a32 + pos) & BZ_MASK] = (uint8_t)s;
                    pos++;
                    if (pos - flushed >= BZ_GROUP) { if (!flush_full()) break; }
                    continue;
                }
                if (s == 256) break;
                if (s > 285) { bad_code = true; break; }
                uint32_t lb, le; len_code((uint32_t)s - 257u, lb, le);
                const uint32_t len = lb + b.get(le);
                b.refill();
                const int ds = decode_sym(b, L.h.dist_tab, DIST_PB, L.h.dist_count, L.h.dist_sym, dist_max);
                if (ds < 0 || ds > 29) { bad_code = true; break; }
                uint32_t db, de; dist_code((uint32_t)ds, db, de);
                const uint32_t dist = db + b.get(de);
                if (dist > pos) { bad_code = true; break; }      // in front of the block's first byte: a block starts its own history
                if (len > isize - pos) { status = BZ_TOO_LONG; break; }
                // the copy, by all lanes: position pos + i takes what stands dist back — periodic when the match overlaps itself,
                // so every source lies in front of pos and the lanes do not depend on one another
                for (uint32_t i = lane; i < len; i += 64) {
                    const uint32_t j = i < dist ? i : i % dist;
                    const uint32_t src = pos - dist + j;
                    const uint8_t v = pos - src <= BZ_NEAR ? L.ring[(a32 + src) & BZ_MASK] : out[src];
                    L.ring[(a32 + pos + i) & BZ_MASK] = v;
                }
                pos += len;
                if (pos - flushed >= BZ_GROUP) { if (!flush_full()) break; }
            }
            if (status) break;
            if (bad_code) { status = BZ_CORRUPT; break; }
        }
        if (bfinal) { status = BZ_FINAL; break; }
    }
    // what is left in the ring (pos <= isize: inside the block's range)
    while (flushed < pos) { const uint32_t e = min(group_end(flushed), pos); store_range(flushed, e); flushed = e; }
    // good: the final block was reached, exactly ISIZE bytes came out, and the stream ends in the block's last deflate byte
    if (status == BZ_FINAL) status = pos != isize ? BZ_TOO_SHORT : (b.pos() + 7ull) / 8ull != in_end ? BZ_NOT_AT_END : BZ_GOOD;
    if (lane == 0) { status_out[blk] = status; if (status != BZ_GOOD) atomicMin(&bad[0], blk); }
}

// CRC-32 of every block's text against its trailer: one thread per block, four table look-ups per dword (slicing by 4).
// bad[1]: the first block (atomicMin) whose checksum differs
__global__ __launch_bounds__(64) void k_bgzf_crc(const uint8_t *__restrict__ text, const BgzfDesc *__restrict__ desc, uint32_t n_blocks, uint32_t *__restrict__ bad) {
    __shared__ uint32_t tab[4][256];
    for (uint32_t e = threadIdx.x; e < 256; e += 64) {
        uint32_t cc = e;
        for (int k = 0; k < 8; k++) cc = (cc & 1u) ? 0xEDB88320u ^ (cc >> 1) : cc >> 1;
        tab[0][e] = cc;
    }
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < 256; e += 64) {
        uint32_t cc = tab[0][e];
        for (int t = 1; t < 4; t++) { cc = (cc >> 8) ^ tab[0][cc & 0xFFu]; tab[t][e] = cc; }
    }
    __syncthreads();
    const uint32_t blk = blockIdx.x * 64u + threadIdx.x;
    if (blk >= n_blocks) return;
    const BgzfDesc d = desc[blk];
    unsigned long long p = d.out_off;
    const unsigned long long e = p + d.isize;
    uint32_t crc = 0xFFFFFFFFu;
    // a block starts at any byte: byte-wise up to the first 16-byte boundary of the text, then 16 bytes per load
    for (; p < e && (p & 15u); p++) crc = tab[0][(crc ^ text[p]) & 0xFFu] ^ (crc >> 8);
    for (; p + 16 <= e; p += 16) {
        const uint4 v = *reinterpret_cast<const uint4 *>(text + p);
        const uint32_t ws[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t x = crc ^ ws[q];
            crc = tab[3][x & 0xFFu] ^ tab[2][(x >> 8) & 0xFFu] ^ tab[1][(x >> 16) & 0xFFu] ^ tab[0][x >> 24];
        }
    }
    for (; p < e; p++) crc = tab[0][(crc ^ text[p]) & 0xFFu] ^ (crc >> 8);
    if ((crc ^ 0xFFFFFFFFu) != d.crc) atomicMin(&bad[1], blk);
}

// Where the last record of text[0..n) starts that is known to be one — the rule of last_record_start (fastq.cpp), which this
// kernel must agree with byte for byte: a line that begins with '@' and whose line after next begins with '+'; a line whose
// line after next has not begun inside the text is undecided.  One wave walks the tail [from, n) from the back, 64 bytes a
// step: a ballot over the newlines of the step, its bits taken from the top (all of it wave-uniform).  `from` begins a line
// only where it is 0.  out[0] = the start, or ~0 (the host then widens the tail).
__global__ __launch_bounds__(64) void k_last_record_start(const uint8_t *__restrict__ text, unsigned long long n, unsigned long long from,
                                                         unsigned long long *__restrict__ out) {
    const uint32_t lane = threadIdx.x;
    unsigned long long s1 = n, s2 = n, found = ~0ull;      // the starts of the next line and of the line after next (n: none)
    auto line = [&](unsigned long long p) -> bool {        // a line starts at p < n
        if (s2 < n && text[p] == '@' && text[s2] == '+') { found = p; return true; }
        s2 = s1; s1 = p;
        return false;
    };
    for (unsigned long long hi = n; hi > from && found == ~0ull;) {
        const unsigned long long lo = hi - from > 64ull ? hi - 64ull : from;
        const unsigned long long at = lo + lane;
        unsigned long long m = __ballot(at < hi && text[at] == '\n');
        while (m) {
            const int b = 63 - __clzll((long long)m);
            m &= ~(1ull << b);
            const unsigned long long p = lo + (unsigned)b + 1ull;
            if (p < n && line(p)) break;
        }
        hi = lo;
    }
    if (found == ~0ull && from == 0 && n > 0) (void)line(0);
    if (lane == 0) out[0] = found;
}

// The forward twin — the rule of first_record_start (fastq.cpp), which this kernel must agree with byte for byte: the first
// line at or after `from` that begins with '@' and whose line after next begins with '+'.  One wave walks [from, limit)
// from the front, 64 bytes a step: a ballot over the newlines of the step, its bits taken from the bottom; the starts of the
// current line and of the two before it are kept (all of it wave-uniform).  A line is decided when its line after next
// begins — inside [0, n) and behind a newline in front of `limit`; `from` begins a line only where it is 0 or text[from - 1]
// is a newline.  limit <= n.  out[0] = the start, or ~0 when nothing was decided inside [from, limit): the host then widens
// the limit, and at limit == n takes "undecided" as the text's last word.
__global__ __launch_bounds__(64) void k_first_record_start(const uint8_t *__restrict__ text, unsigned long long n, unsigned long long from,
                                                          unsigned long long limit, unsigned long long *__restrict__ out) {
    const uint32_t lane = threadIdx.x;
    const unsigned long long none = ~0ull;
    unsigned long long s1 = none, s2 = none, found = none;       // the starts of the line before the current one and of the one before that
    bool stop = false;                                           // the walk ends with the first start
    auto line = [&](unsigned long long p) -> bool {              // a line starts at p < n
        if (s2 != none && text[s2] == '@' && text[p] == '+') { found = s2; return true; }
        s2 = s1; s1 = p;
        return false;
    };
    if (from < limit && (from == 0 || text[from - 1] == '\n')) stop = line(from);
    for (unsigned long long lo = from; lo < limit && !stop; lo += 64ull) {
        const unsigned long long at = lo + lane;
        unsigned long long m = __ballot(at < limit && text[at] == '\n');
        while (m) {
            const int b = __ffsll((long long)m) - 1;
            m &= m - 1ull;
            const unsigned long long p = lo + (unsigned)b + 1ull;
            if (p < n && line(p)) { stop = true; break; }
        }
    }
    if (lane == 0) out[0] = found;
}

// The FASTA rule — fasta_first_record_start / fasta_last_record_start (fastq.cpp), which this kernel must agree with byte for
// byte: a record starts at p where text[p] == '>' and p begins a line (p == 0 or text[p - 1] == '\n').  A record is a contig
// or a chromosome, so the search may cross megabytes: it is byte-parallel, a grid over text[lo, hi) with 16 bytes per lane.
// The groups of 16 lie at 16-byte aligned ADDRESSES (a span need not begin at one): a group that lies inside [lo, hi) whole is
// one vector load, the head and the tail groups are read byte by byte and never outside [lo, hi).  The byte in front of a
// lane's first byte is one extra load (text[lo - 1] is read where lo > 0: it belongs to the text).  Lanes lie in text order,
// so the first lane of a wave's ballot holds the wave's first start and the last lane its last: one 64-bit atomic per wave
// that found a start.  LAST false: out[0] = min(out[0], p), the host sets ~0 (none).  LAST true: out[0] = max(out[0], p + 1),
// the host sets 0 (none).  hi <= n.
template <bool LAST>
__global__ __launch_bounds__(256) void k_fasta_header_search(const uint8_t *__restrict__ text, unsigned long long lo, unsigned long long hi,
                                                             unsigned long long *__restrict__ out) {
    const unsigned long long head = (unsigned long long)((uintptr_t)(text + lo) & 15u);      // bytes of the first group in front of lo
    const unsigned long long g = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    // the group [i0, i0 + 16) in text offsets, i0 + head counted from lo so that nothing goes below zero
    const unsigned long long rel = g * 16ull;                 // the group begins rel - head bytes behind lo
    const unsigned long long s = rel > head ? lo + (rel - head) : lo;
    unsigned long long e = lo + (rel + 16ull - head);
    if (e > hi) e = hi;
    uint32_t hdr = 0;                                         // bit j: a record starts at s0 + j, s0 = the group's first byte
    if (s < e) {
        const unsigned shift = rel > head ? 0u : (unsigned)(head - rel);      // the bit of byte s (the head group alone begins in front of it)
        uint32_t gt = 0, nl = 0;
        if (e - s == 16ull) {
            const uint4 v = *reinterpret_cast<const uint4 *>(text + s);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const uint32_t c = (w[j >> 2] >> (8 * (j & 3))) & 0xFFu;
                gt |= (uint32_t)(c == '>') << j; nl |= (uint32_t)(c == '\n') << j;
            }
        } else {
            for (unsigned long long p = s; p < e; p++) {
                const uint32_t c = text[p], j = shift + (uint32_t)(p - s);
                gt |= (uint32_t)(c == '>') << j; nl |= (uint32_t)(c == '\n') << j;
            }
        }
        const uint32_t before = (s == 0 || text[s - 1] == '\n') ? 1u << shift : 0u;
        hdr = gt & ((nl << 1) | before);
    }
    const unsigned long long found = __ballot(hdr != 0);
    if (!found) return;
    const unsigned lane = threadIdx.x & 63u;
    const unsigned shift = rel > head ? 0u : (unsigned)(head - rel);
    if (!LAST) {
        if (lane == (unsigned)(__ffsll((long long)found) - 1)) atomicMin(out, s - shift + (unsigned)(__ffs((int)hdr) - 1));
    } else {
        if (lane == 63u - (unsigned)__clzll((long long)found)) atomicMax(out, s - shift + (31u - (unsigned)__clz((int)hdr)) + 1ull);
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
// CRC-32 of A || B from crc(A), crc(B): crc(A) advanced over len(B) zero bytes (a GF(2) matrix), XOR crc(B).  The slices
// have one length, so the matrix is built once (zlib 1.2.11 has no crc32_combine_gen).
struct Gf2 { uint32_t m[32]; };
uint32_t gf2_times(const Gf2 &a, uint32_t v) { uint32_t s = 0; for (int i = 0; v; v >>= 1, i++) if (v & 1u) s ^= a.m[i]; return s; }
Gf2 gf2_square(const Gf2 &a) { Gf2 r; for (int i = 0; i < 32; i++) r.m[i] = gf2_times(a, a.m[i]); return r; }
Gf2 crc_shift_matrix(uint64_t len_bytes) {              // operator "append len_bytes zero bytes"
    Gf2 odd; odd.m[0] = 0xEDB88320u; { uint32_t row = 1; for (int i = 1; i < 32; i++) { odd.m[i] = row; row <<= 1; } }   // one zero BIT
    Gf2 even = gf2_square(odd);                           // two bits
    odd = gf2_square(even);                               // four bits
    Gf2 result; for (int i = 0; i < 32; i++) result.m[i] = 1u << i;      // identity
    Gf2 cur = gf2_square(odd);                            // eight bits = one byte
    for (uint64_t n = len_bytes; n; n >>= 1) {
        if (n & 1u) { Gf2 r; for (int i = 0; i < 32; i++) r.m[i] = gf2_times(cur, result.m[i]); result = r; }
        cur = gf2_square(cur);
    }
    return result;
}

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace

// (a failed call leaves the stream drained: the blocks of the function that returns go back to the pool idle)
#define GZCHK(call) HIPCHK_AS(#call, call, (void)hipStreamSynchronize(st))

namespace {
// the last bytes of a text on the device, for trim_text_end: fetch_tail enqueues the copy, the caller waits (with whatever
// else it waits for)
struct Tail { char b[4096]; size_t n = 0; };
hipError_t fetch_tail(const uint8_t *d_text, uint64_t n, Tail &t, hipStream_t st) {
    t.n = (size_t)std::min<uint64_t>(n, sizeof t.b);
    return t.n ? hipMemcpyAsync(t.b, d_text + (n - t.n), t.n, hipMemcpyDeviceToHost, st) : hipSuccess;
}

// The end of the text d_text[0..n) (t: its tail, arrived) as gpu_upload_text hands a text on (fastq_gpu.hip: trimmed_len):
// "\n\n" and "\n\r\n" at the end lose their last line end, repeatedly, and 32 zero bytes follow what is left (d_text has
// room for them); raw: every byte stays as it is.  0: e bytes of text; 1: more blank lines than are looked at (*why); -5.
int trim_text_end(uint8_t *d_text, uint64_t n, const Tail &t, bool raw, hipStream_t st, uint64_t &e, bool &unterminated, const char *&why, std::string &err) {
    const char *tail = t.b; const size_t tail_n = t.n;
    size_t te = tail_n;
    while (!raw) {
        if (te >= 2 && tail[te - 1] == '\n' && tail[te - 2] == '\n') { te -= 1; continue; }
        if (te >= 3 && tail[te - 1] == '\n' && tail[te - 2] == '\r' && tail[te - 3] == '\n') { te -= 2; continue; }
        break;
    }
    if (te < 8 && n > tail_n) { why = "kilobytes of blank lines at the end"; return 1; }
    e = (n - tail_n) + te;
    unterminated = te == 0 || tail[te - 1] != '\n';
    if (!raw) GZCHK(hipMemsetAsync(d_text + e, 0, 32, st));
    GZCHK(hipStreamSynchronize(st));
    return 0;
}

// The inflated text (d_text: `total` bytes and 64 more, tail: its last bytes, arrived) becomes out's, made ready for the
// parser unless raw (trim_text_end).  0: out owns the block; 1: not taken (*why); -5.
int hand_on_text(PoolBlock &d_text, uint64_t total, const Tail &tail, bool raw, hipStream_t st, GpuText &out, const char *&why, std::string &err) {
    uint64_t e = 0; bool unterminated = false;
    if (const int rc = trim_text_end((uint8_t *)d_text.p, total, tail, raw, st, e, unterminated, why, err)) return rc;
    if (e == 0) { why = "empty text"; return 1; }
    out.pool_bytes = d_text.bytes; out.d = (uint8_t *)d_text.take();      // (out is a plain record: gpu_text_free)
    out.e = (size_t)e; out.unterminated = unterminated;
    return 0;
}

// Blocks [b0, b1) of a walked chain: one wave per non-empty block, then the blocks' checksums.  d_in holds the file from
// byte in_base on (zero padding behind it), the first block's text goes to d_text + text_at; d_desc and d_status have room
// for the run's non-empty blocks, d_bad is 64 bytes.  ms: from the first copy to the verdict; crc_ms, where asked for
// and SHK_GUNZIP_DEBUG is set: the share of it behind the decoder (one more wait); tail, where asked for: the last bytes of
// the run's text, which come back in the verdict's wait.
// 0; 1: a block is not what its trailer says (*why); -5.
int inflate_block_run(const BgzfChain &chain, size_t b0, size_t b1, const void *d_in, uint64_t in_base, uint8_t *d_text, uint64_t text_at,
                      PoolBlock &d_desc, PoolBlock &d_status, PoolBlock &d_bad, hipStream_t st, double &ms, double *crc_ms, Tail *tail, const char *&why, std::string &err) {
    std::vector<BgzfDesc> desc;
    for (size_t b = b0; b < b1; b++) {
        const BgzfChain::Block &k = chain.blocks[b];
        if (k.isize) desc.push_back(BgzfDesc{(unsigned long long)(k.in_off - in_base + k.hdr), k.bsize - k.hdr - 8, (uint32_t)text_at, k.isize, k.crc});
        text_at += k.isize;
    }
    const uint32_t nb = (uint32_t)desc.size();
    if (!nb) return 0;
    const double t1 = now_ms();
    GZCHK(hipMemcpyAsync(d_desc.p, desc.data(), (size_t)nb * sizeof(BgzfDesc), hipMemcpyHostToDevice, st));
    GZCHK(hipMemsetAsync(d_bad.p, 0xFF, 64, st));
    hipLaunchKernelGGL(k_bgzf_decode, dim3(nb), dim3(64), 0, st, (const uint32_t *)d_in, (const BgzfDesc *)d_desc.p, nb, d_text,
                       (uint32_t *)d_status.p, (uint32_t *)d_bad.p);
    GZCHK(hipGetLastError());
    double t2 = 0;
    if (crc_ms && getenv("SHK_GUNZIP_DEBUG")) { GZCHK(hipStreamSynchronize(st)); t2 = now_ms(); }
    hipLaunchKernelGGL(k_bgzf_crc, dim3((nb + 63) / 64), dim3(64), 0, st, (const uint8_t *)d_text, (const BgzfDesc *)d_desc.p, nb, (uint32_t *)d_bad.p);
    GZCHK(hipGetLastError());
    uint32_t h_bad[2] = {0, 0};
    GZCHK(hipMemcpyAsync(h_bad, d_bad.p, 8, hipMemcpyDeviceToHost, st));
    if (tail) GZCHK(fetch_tail(d_text, text_at, *tail, st));
    GZCHK(hipStreamSynchronize(st));                        // (desc is read by the copy until here)
    ms = now_ms() - t1;
    if (t2 != 0) *crc_ms = now_ms() - t2;
    if (h_bad[0] != 0xFFFFFFFFu) {                            // the first block that is not good: what it did
        uint32_t status = 0;
        GZCHK(hipMemcpyAsync(&status, (uint32_t *)d_status.p + h_bad[0], 4, hipMemcpyDeviceToHost, st));
        GZCHK(hipStreamSynchronize(st));
        why = status == BZ_TOO_LONG ? "a BGZF block inflates beyond its ISIZE" : status == BZ_TOO_SHORT ? "a BGZF block ends short of its ISIZE" :
              status == BZ_NOT_AT_END ? "a BGZF block's stream does not end where its data ends" : "a damaged BGZF block";
        return 1;
    }
    if (h_bad[1] != 0xFFFFFFFFu) { why = "CRC-32 mismatch"; return 1; }
    return 0;
}

// gz[0..n) starts with a BGZF block.  Taken only if every byte of the file belongs to the chain of blocks (what follows a
// first BGZF block may be anything: the host reader owns "BGZF block chain broken" and its kin); same results as
// gpu_inflate_member, except that running out of device memory is "not taken" too: the host reader reads these files.
int gpu_inflate_bgzf(const uint8_t *gz, size_t n, int device, hipStream_t st, GpuText &out, std::string &err, GpuInflateStats &S, bool raw, const BgzfChain *walked) {
    auto not_taken = [&](const char *why) { S.why_not = why; return 1; };
    if (n >= ((size_t)1 << 34)) return not_taken("beyond 16 GiB");      // (UBits counts the input in 32-bit dwords)
    BgzfChain own;
    const char *why = "";
    if (!walked && bgzf_walk(gz, n, own, why)) return not_taken(why);
    const BgzfChain &chain = walked ? *walked : own;
    const uint64_t total = chain.text;
    if (total == 0 || total >= ((uint64_t)1 << 32)) return not_taken("empty or beyond 4 GiB");
    const uint32_t nb = (uint32_t)chain.nonempty;
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); err = "hipSetDevice failed"; return -5; }
    const double t_begin = now_ms();
    // ---- upload: the file as it is (26 bytes of header and trailer per block are not worth a repack), zero padding behind
    PoolBlock d_in, d_desc, d_status, d_bad, d_text;
    const size_t in_words = (n + 3) / 4 + 2048 + 256;        // (the same padding as for a plain member: see gpu_inflate_member)
    if (!d_in.get(in_words * 4) || !d_desc.get((size_t)nb * sizeof(BgzfDesc)) || !d_status.get((size_t)nb * 4) || !d_bad.get(64) ||
        !d_text.get((size_t)total + 64))
        return not_taken("out of device memory");
    GZCHK(hipMemsetAsync((char *)d_in.p + (n & ~(size_t)3), 0, in_words * 4 - (n & ~(size_t)3), st));
    GZCHK(hipMemcpyAsync(d_in.p, gz, n, hipMemcpyHostToDevice, st));
    GZCHK(hipMemsetAsync((char *)d_text.p + total, 0, 64, st));
    GZCHK(hipStreamSynchronize(st));
    S.h2d_ms = now_ms() - t_begin;
    // ---- every block, then its checksum; one word each comes back
    double ms = 0, crc_ms = 0;
    Tail tail;
    int rc = inflate_block_run(chain, 0, chain.blocks.size(), d_in.p, 0, (uint8_t *)d_text.p, 0, d_desc, d_status, d_bad, st, ms, &crc_ms, &tail, why, err);
    S.decode_ms = ms - crc_ms; S.resolve_ms = crc_ms;
    if (!rc) rc = hand_on_text(d_text, total, tail, raw, st, out, why, err);
    if (rc) return rc == 1 ? not_taken(why) : rc;
    out.h2d_ms = S.h2d_ms;
    S.blocks = nb; S.text_bytes = total; S.total_ms = now_ms() - t_begin;
    if (getenv("SHK_GUNZIP_DEBUG"))
        fprintf(stderr, "[inflate_gpu] BGZF, %u blocks: upload %.2f ms, decode %.2f, crc %.2f, total %.2f ms for %.3f GB of text\n",
                nb, S.h2d_ms, S.decode_ms, S.resolve_ms, S.total_ms, (double)total / 1e9);
    return 0;
}
}  // namespace

int gpu_inflate_member(const uint8_t *gz, size_t n, int device, void *stream, GpuText &out, std::string &err, GpuInflateStats *stats, bool raw, const BgzfChain *walked) {
    GpuInflateStats local; GpuInflateStats &S = stats ? *stats : local;
    S = GpuInflateStats();
    out = GpuText();
    auto not_taken = [&](const char *why) { S.why_not = why; return 1; };
    // ---- gzip member header (RFC 1952); the trailer is taken to be the last 8 bytes (one member, nothing behind it:
    // checked against where the final block really ends)
    if (n < 18 || gz[0] != 0x1F || gz[1] != 0x8B || gz[2] != 8) return not_taken("not a gzip member");
    const unsigned flg = gz[3];
    size_t p = 10;
    if (flg & 4) {
        if (p + 2 > n) return not_taken("truncated header");
        const size_t xlen = gz[p] | ((size_t)gz[p + 1] << 8);
        // (BGZF: a 'BC' subfield — many small members, one wave each)
        size_t bs = 0;
        if (bgzf_block(gz, n, bs)) return gpu_inflate_bgzf(gz, n, device, (hipStream_t)stream, out, err, S, raw, walked);
        if (xlen >= 6 && p + 2 + xlen <= n && gz[p + 2] == 'B' && gz[p + 3] == 'C') return not_taken("BGZF");      // (a first block cut short)
        p += 2 + xlen;
    }
    if (flg & 8) { while (p < n && gz[p]) p++; p++; }
    if (flg & 16) { while (p < n && gz[p]) p++; p++; }
    if (flg & 2) p += 2;
    if (p + 8 >= n) return not_taken("truncated header");
    const uint8_t *def = gz + p;
    const size_t dn = n - p - 8;                                  // deflate data if this is the only member
    const char *mv = getenv("SHK_GUNZIP_DEVICE_MIN");
    const size_t min_bytes = (mv && *mv) ? (size_t)strtoull(mv, nullptr, 10) : ((size_t)4 << 20);
    if (dn < min_bytes) return not_taken("small member");
    const uint8_t *tr = gz + n - 8;
    const uint32_t want_crc = tr[0] | ((uint32_t)tr[1] << 8) | ((uint32_t)tr[2] << 16) | ((uint32_t)tr[3] << 24);
    const uint32_t want_len = tr[4] | ((uint32_t)tr[5] << 8) | ((uint32_t)tr[6] << 16) | ((uint32_t)tr[7] << 24);
    if ((uint64_t)dn * 64 < want_len) return not_taken("ISIZE out of proportion");      // (text deflates 3-6x; more than 64x is not FASTQ)
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); err = "hipSetDevice failed"; return -5; }
    hipStream_t st = (hipStream_t)stream;
    const double t_begin = now_ms();
    // ---- chunks (SHK_GUNZIP_DEVICE_CHUNK: bytes of compressed data each), at most 16384
    const char *cv = getenv("SHK_GUNZIP_DEVICE_CHUNK");
    // (one wave per chunk, 18 waves to a CU by their LDS: ~4600 chunks are resident at once on 256 CUs — a member of the
    // bench isolate's size is cut so that all its chunks run in one round; smaller members into 32 KiB chunks)
    uint64_t chunk_bytes = (cv && *cv) ? strtoull(cv, nullptr, 10) : std::max<uint64_t>(32u << 10, ((uint64_t)dn / 4200u + 4095u) & ~4095ull);
    if (chunk_bytes < 4096) chunk_bytes = 4096;
    while ((dn + chunk_bytes - 1) / chunk_bytes > 16384) chunk_bytes *= 2;
    const uint32_t C0 = (uint32_t)((dn + chunk_bytes - 1) / chunk_bytes);
    if (C0 < 2) return not_taken("small member");
    // ---- upload (the compressed bytes are all that crosses PCIe), zero padding behind
    PoolBlock d_in, d_start;
    const size_t in_words = (dn + 3) / 4 + 2048 + 256;      // (8 KB of zero padding: the decoder checks for the end of the input once per 512 symbols; + the 128 dwords its reader keeps in flight)
    if (!d_in.get(in_words * 4) || !d_start.get((size_t)(C0 + 1) * 8)) { err = "out of device memory (gzip input)"; return -4; }
    GZCHK(hipMemsetAsync((char *)d_in.p + (dn & ~(size_t)3), 0, in_words * 4 - (dn & ~(size_t)3), st));
    GZCHK(hipMemcpyAsync(d_in.p, def, dn, hipMemcpyHostToDevice, st));
    GZCHK(hipMemsetAsync(d_start.p, 0, (size_t)(C0 + 1) * 8, st));
    GZCHK(hipStreamSynchronize(st));
    S.h2d_ms = now_ms() - t_begin;
    // ---- 1. block starts
    double t1 = now_ms();
    hipLaunchKernelGGL(k_gz_find_starts, dim3(C0 - 1), dim3(64), 0, st, (const uint32_t *)d_in.p, (uint64_t)dn, chunk_bytes, C0, (unsigned long long *)d_start.p);
    GZCHK(hipGetLastError());
    std::vector<unsigned long long> start(C0 + 1, 0);
    GZCHK(hipMemcpyAsync(start.data(), d_start.p, (size_t)C0 * 8, hipMemcpyDeviceToHost, st));
    GZCHK(hipStreamSynchronize(st));
    S.search_ms = now_ms() - t1;
    // (a chunk without a start is merged into its predecessor)
    std::vector<unsigned long long> stv; stv.push_back(0);
    for (uint32_t c = 1; c < C0; c++) if (start[c] != ~0ull && start[c] > stv.back()) stv.push_back(start[c]);
    const uint32_t C = (uint32_t)stv.size();
    if (C < 2 || C * 4u < C0) return not_taken("block starts not found");      // (binary data, stored blocks, fixed codes)
    // ---- 2. every chunk, with markers for what lies in front of it.  Room per chunk: 10 symbols per compressed byte
    // (SHK_GUNZIP_DEVICE_RATIO; FASTQ text deflates 3-6x) + a margin; a chunk that needs more makes the member fall back
    const char *rv = getenv("SHK_GUNZIP_DEVICE_RATIO");
    const uint64_t ratio = (rv && *rv) ? std::max<uint64_t>(2, strtoull(rv, nullptr, 10)) : 10;
    std::vector<unsigned long long> sym_off(C + 1, 0);
    for (uint32_t c = 0; c < C; c++) {
        const uint64_t comp = ((c + 1 < C ? stv[c + 1] : (uint64_t)dn * 8) - stv[c] + 7) / 8;
        const uint64_t room = (comp * ratio + 8192 + 511) & ~511ull;
        sym_off[c + 1] = sym_off[c] + room;
    }
    PoolBlock d_syms, d_soff, d_res, d_bad;
    if (!d_syms.get((size_t)sym_off[C] * 2 + 64) || !d_soff.get((size_t)(C + 1) * 8) || !d_res.get((size_t)C * sizeof(ChunkOut)) || !d_bad.get(64)) {
        err = "out of device memory (gzip symbols)"; return -4;
    }
    t1 = now_ms();
    GZCHK(hipMemcpyAsync(d_start.p, stv.data(), (size_t)C * 8, hipMemcpyHostToDevice, st));
    GZCHK(hipMemcpyAsync(d_soff.p, sym_off.data(), (size_t)(C + 1) * 8, hipMemcpyHostToDevice, st));
    GZCHK(hipMemsetAsync(d_bad.p, 0, 64, st));
    hipLaunchKernelGGL(k_gz_decode, dim3(C), dim3(64), 0, st, (const uint32_t *)d_in.p, (uint64_t)dn, C, (const unsigned long long *)d_start.p,
                       (const unsigned long long *)d_soff.p, (uint16_t *)d_syms.p, (ChunkOut *)d_res.p);
    GZCHK(hipGetLastError());
    std::vector<ChunkOut> res(C);
    GZCHK(hipMemcpyAsync(res.data(), d_res.p, (size_t)C * sizeof(ChunkOut), hipMemcpyDeviceToHost, st));
    GZCHK(hipStreamSynchronize(st));
    S.decode_ms = now_ms() - t1;
    std::vector<unsigned long long> out_off(C + 1, 0);
    for (uint32_t c = 0; c < C; c++) {
        const uint32_t want = c + 1 < C ? GZ_ATSTOP : GZ_FINAL;
        if (res[c].status != want) return not_taken(res[c].status == GZ_NO_ROOM ? "a chunk inflates beyond its room" : "a chunk does not end where the next begins");
        if (c + 1 < C && res[c].end_pos != stv[c + 1]) return not_taken("a chunk does not end where the next begins");
        out_off[c + 1] = out_off[c] + res[c].n_sym;
    }
    const uint64_t total = out_off[C];
    // the final block must end right in front of the trailer (one member, nothing behind it)
    if ((res[C - 1].end_pos + 7) / 8 != (uint64_t)dn) return not_taken("more than one member, or data behind the member");
    if ((uint32_t)total != want_len) return not_taken("ISIZE mismatch");
    if (total == 0 || total >= ((uint64_t)1 << 32)) return not_taken("empty or beyond 4 GiB");
    // ---- 3. windows front to back, 4. markers -> bytes, CRC
    PoolBlock d_ma, d_mb, d_ooff, d_text, d_crc;
    const uint32_t SLICE = 65536;
    const uint32_t n_slices = (uint32_t)((total + SLICE - 1) / SLICE);
    if (!d_ma.get((size_t)C * GZ_WSIZE * 2) || !d_mb.get((size_t)C * GZ_WSIZE * 2) || !d_ooff.get((size_t)(C + 1) * 8) || !d_text.get((size_t)total + 64) ||
        !d_crc.get((size_t)n_slices * 4)) {
        err = "out of device memory (inflated text)"; return -4;
    }
    t1 = now_ms();
    GZCHK(hipMemcpyAsync(d_ooff.p, out_off.data(), (size_t)(C + 1) * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_gz_win_init, dim3(C - 1), dim3(1024), 0, st, (const uint16_t *)d_syms.p, (const unsigned long long *)d_soff.p, (const ChunkOut *)d_res.p, C,
                       (uint16_t *)d_ma.p);
    uint16_t *Mi = (uint16_t *)d_ma.p, *Mo = (uint16_t *)d_mb.p;
    for (uint32_t step = 1; step < C; step *= 2) {
        hipLaunchKernelGGL(k_gz_win_round, dim3(C - 1), dim3(1024), 0, st, (const uint16_t *)Mi, Mo, C, step);
        std::swap(Mi, Mo);
    }
    GZCHK(hipGetLastError());
    if (getenv("SHK_GUNZIP_DEBUG")) { GZCHK(hipStreamSynchronize(st)); S.windows_ms = now_ms() - t1; }
    hipLaunchKernelGGL(k_gz_resolve, dim3(16, C), dim3(256), 0, st, (const uint16_t *)d_syms.p, (const unsigned long long *)d_soff.p, (const ChunkOut *)d_res.p,
                       (const unsigned long long *)d_ooff.p, (const uint16_t *)Mi, (uint8_t *)d_text.p, (uint32_t *)d_bad.p);
    GZCHK(hipMemsetAsync((char *)d_text.p + total, 0, 64, st));
    hipLaunchKernelGGL(k_gz_crc, dim3((n_slices + 255) / 256), dim3(256), 0, st, (const uint8_t *)d_text.p, (unsigned long long)total, SLICE, n_slices, (uint32_t *)d_crc.p);
    GZCHK(hipGetLastError());
    std::vector<uint32_t> crcs(n_slices);
    uint32_t h_bad[2] = {0, 0};
    Tail tail;
    GZCHK(hipMemcpyAsync(crcs.data(), d_crc.p, (size_t)n_slices * 4, hipMemcpyDeviceToHost, st));
    GZCHK(hipMemcpyAsync(h_bad, d_bad.p, 8, hipMemcpyDeviceToHost, st));
    GZCHK(fetch_tail((const uint8_t *)d_text.p, total, tail, st));
    GZCHK(hipStreamSynchronize(st));
    S.resolve_ms = now_ms() - t1;
    if (h_bad[0]) return not_taken("a back-reference in front of the stream");
    // combine the slice checksums
    uint32_t crc = crcs[0];
    if (n_slices > 1) {
        const Gf2 M = crc_shift_matrix(SLICE);
        for (uint32_t s = 1; s + 1 < n_slices; s++) crc = gf2_times(M, crc) ^ crcs[s];
        const uint64_t last = total - (uint64_t)(n_slices - 1) * SLICE;
        crc = (uint32_t)crc32_combine(crc, crcs[n_slices - 1], (z_off_t)last);
    }
    if (crc != want_crc) return not_taken("CRC-32 mismatch");
    const char *why = "";
    if (const int rt = hand_on_text(d_text, total, tail, raw, st, out, why, err)) return rt == 1 ? not_taken(why) : rt;
    out.h2d_ms = S.h2d_ms;
    S.chunks = C; S.text_bytes = total; S.total_ms = now_ms() - t_begin;
    if (getenv("SHK_GUNZIP_DEBUG"))
        fprintf(stderr, "[inflate_gpu] %u chunks (%u cuts): upload %.2f ms, block starts %.2f, decode %.2f, windows (%.2f) + resolve + crc %.2f, total %.2f ms for %.3f GB of text\n",
                C, C0, S.h2d_ms, S.search_ms, S.decode_ms, S.windows_ms, S.resolve_ms, S.total_ms, (double)total / 1e9);
    return 0;
}

// ---- a BGZF file window by window (inflate_gpu.h) -----------------------------------------------------------------------
namespace {
// one upload stream per device for the windows' compressed bytes, kept for the process (as gpu_upload_text keeps its own)
hipError_t window_upload_stream(int device, hipStream_t &s) {
    static std::mutex mu;
    static hipStream_t streams[64] = {};
    std::lock_guard<std::mutex> lk(mu);
    const int di = device >= 0 && device < 64 ? device : 0;
    hipError_t e = hipSuccess;
    if (!streams[di]) e = hipStreamCreateWithFlags(&streams[di], hipStreamNonBlocking);
    s = streams[di];
    return e;
}
const size_t WIN_IN_PAD = (2048 + 256) * 4 + 8;           // zero bytes behind a window's input (see gpu_inflate_member)

// the last record start of d_text[0..n): the tail of 1 MiB first, a wider one while nothing is found — up to max_tail bytes
// (one wave walks it: the windows' caller has no use for a start further front than it can carry)
// k_fasta_header_search over d_text[lo, hi): the result word is set here.  got: the start, or UINT64_MAX
template <bool LAST>
int fasta_header_search(const uint8_t *d_text, uint64_t lo, uint64_t hi, unsigned long long *d_out, hipStream_t st, uint64_t &got, std::string &err) {
    got = UINT64_MAX;
    if (lo >= hi) return 0;
    const uint64_t groups = (hi - lo + 15 + 15) / 16;        // (an unaligned head adds at most one group)
    if (groups > 256ull * 0x7FFFFFFFull) { err = "a FASTA header search beyond the grid"; return -5; }
    GZCHK(hipMemsetAsync(d_out, LAST ? 0 : 0xFF, 8, st));
    hipLaunchKernelGGL(k_fasta_header_search<LAST>, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, st, d_text, (unsigned long long)lo, (unsigned long long)hi, d_out);
    GZCHK(hipGetLastError());
    unsigned long long w = 0;
    GZCHK(hipMemcpyAsync(&w, d_out, 8, hipMemcpyDeviceToHost, st));
    GZCHK(hipStreamSynchronize(st));
    if (LAST) { if (w) got = w - 1; }
    else if (w != ~0ull) got = w;
    return 0;
}

int device_last_start(const uint8_t *d_text, uint64_t n, unsigned long long *d_out, hipStream_t st, uint64_t &at, std::string &err, uint64_t max_tail = UINT64_MAX,
                      RecFmt fmt = RecFmt::Fastq) {
    at = UINT64_MAX;
    if (fmt == RecFmt::Fasta) {
        // the same tails; a line is decided by its own first byte, so what a tail has shown to hold no start is not searched again
        uint64_t hi = n;
        for (uint64_t tail = std::min<uint64_t>(1ull << 20, max_tail);; tail = tail > max_tail / 16 ? max_tail : tail * 16) {
            const uint64_t from = n > tail ? n - tail : 0;
            if (const int rc = fasta_header_search<true>(d_text, from, hi, d_out, st, at, err)) return rc;
            if (at != UINT64_MAX || from == 0 || tail >= max_tail) return 0;
            hi = from;
        }
    }
    for (uint64_t tail = std::min<uint64_t>(1ull << 20, max_tail);; tail = tail > max_tail / 16 ? max_tail : tail * 16) {
        const uint64_t from = n > tail ? n - tail : 0;
        hipLaunchKernelGGL(k_last_record_start, dim3(1), dim3(64), 0, st, d_text, (unsigned long long)n, (unsigned long long)from, d_out);
        GZCHK(hipGetLastError());
        unsigned long long got = 0;
        GZCHK(hipMemcpyAsync(&got, d_out, 8, hipMemcpyDeviceToHost, st));
        GZCHK(hipStreamSynchronize(st));
        if (got != ~0ull) { at = got; return 0; }
        if (from == 0 || tail >= max_tail) return 0;
    }
}

// the first record start of d_text[0..n) at or after `from`: 1 MiB behind `from` first, a wider reach while nothing is
// decided.  at = UINT64_MAX: undecided at the end of the text
int device_first_start(const uint8_t *d_text, uint64_t n, uint64_t from, unsigned long long *d_out, hipStream_t st, uint64_t &at, std::string &err,
                       RecFmt fmt = RecFmt::Fastq) {
    at = UINT64_MAX;
    if (from >= n) return 0;
    if (fmt == RecFmt::Fasta) {
        // the same reaches (a start near `from` stays cheap); each one begins where the one before it ended.  UINT64_MAX: none
        uint64_t lo = from;
        for (uint64_t reach = 1ull << 20;; reach *= 16) {
            const uint64_t limit = n - from > reach ? from + reach : n;
            if (const int rc = fasta_header_search<false>(d_text, lo, limit, d_out, st, at, err)) return rc;
            if (at != UINT64_MAX || limit == n) return 0;
            lo = limit;
        }
    }
    for (uint64_t reach = 1ull << 20;; reach *= 16) {
        const uint64_t limit = n - from > reach ? from + reach : n;
        hipLaunchKernelGGL(k_first_record_start, dim3(1), dim3(64), 0, st, d_text, (unsigned long long)n, (unsigned long long)from, (unsigned long long)limit, d_out);
        GZCHK(hipGetLastError());
        unsigned long long got = 0;
        GZCHK(hipMemcpyAsync(&got, d_out, 8, hipMemcpyDeviceToHost, st));
        GZCHK(hipStreamSynchronize(st));
        if (got != ~0ull) { at = got; return 0; }
        if (limit == n) return 0;
    }
}
}  // namespace

void BgzfWindows::close() {
    if (prefetch_.joinable()) prefetch_.join();
    if (st_ || d_in_[0].p) (void)hipStreamSynchronize((hipStream_t)st_);      // the blocks go back to the pool idle
    for (PoolBlock *b : {&d_in_[0], &d_in_[1], &d_text_[0], &d_text_[1], &d_desc_, &d_status_, &d_bad_}) b->put();
}

int BgzfWindows::open(const uint8_t *gz, const BgzfChain *chain, int device, void *stream, std::string &err) {
    close();
    gz_ = gz; chain_ = chain; device_ = device; st_ = stream;
    h2d_ms = decode_ms = 0; uploaded = 0;
    up_[0] = up_[1] = Upload(); up_w_[0] = up_w_[1] = SIZE_MAX;
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); err = "hipSetDevice failed"; return -5; }
    uint64_t max_in = 0, max_text = 0; uint32_t max_nb = 1;
    for (const BgzfChain::Window &w : chain->windows) {
        max_in = std::max(max_in, w.in_end - w.in_off); max_text = std::max(max_text, w.text); max_nb = std::max(max_nb, w.nonempty);
    }
    // (the pool rounds a size up, or hands out a cached block that is larger: every PoolBlock keeps the size it came with)
    bool ok = true;
    for (int i = 0; i < (chain->windows.size() > 1 ? 2 : 1) && ok; i++)
        ok = d_in_[i].get((size_t)((max_in + 3) & ~3ull) + WIN_IN_PAD) && d_text_[i].get((size_t)(CARRY_MAX + max_text + 64));
    ok = ok && d_desc_.get((size_t)max_nb * sizeof(BgzfDesc)) && d_status_.get((size_t)max_nb * 4) && d_bad_.get(64);
    if (!ok) { close(); return 1; }
    return 0;
}

void BgzfWindows::upload(size_t w) {
    Upload &up = up_[w & 1];
    up = Upload();
    if (hipSetDevice(device_) != hipSuccess) { (void)hipGetLastError(); up.err = "hipSetDevice failed"; up.rc = -5; return; }
    const BgzfChain::Window &win = chain_->windows[w];
    const size_t n = (size_t)(win.in_end - win.in_off);
    uint8_t *d = (uint8_t *)d_in_[w & 1].p;
    hipStream_t s = nullptr;
    const double t0 = now_ms();
    hipError_t e = window_upload_stream(device_, s);
    if (e == hipSuccess) e = hipMemsetAsync(d + (n & ~(size_t)3), 0, ((n + 3) & ~(size_t)3) - (n & ~(size_t)3) + WIN_IN_PAD, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d, gz_ + win.in_off, n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    up.ms = now_ms() - t0;
    if (e != hipSuccess) { up.err = std::string("upload of a BGZF window: ") + hipGetErrorString(e); up.rc = -5; }
    up_w_[w & 1] = w;
}

int BgzfWindows::inflate(size_t w, bool prefetch_next, uint64_t carry, uint64_t &n, const char *&why, std::string &err) {
    hipStream_t st = (hipStream_t)st_;
    const BgzfChain::Window &win = chain_->windows[w];
    // this window's compressed bytes have arrived (they travel now where nobody sent them ahead); the next window's travel while this one is worked on
    if (prefetch_.joinable()) prefetch_.join();
    if (up_w_[w & 1] != w) upload(w);
    if (up_[w & 1].rc) { err = up_[w & 1].err; return up_[w & 1].rc; }
    h2d_ms += up_[w & 1].ms;
    uploaded += win.in_end - win.in_off;
    if (prefetch_next)
        prefetch_ = std::thread([this, w]() {
            try { upload(w + 1); }
            catch (...) { up_[(w + 1) & 1].rc = -4; up_[(w + 1) & 1].err = "out of host memory (uploader)"; }
        });
    if (carry > CARRY_MAX) { why = "a partial record beyond the room for it"; return 1; }
    double ms = 0;
    const int rc = inflate_block_run(*chain_, win.b0, win.b1, d_in_[w & 1].p, win.in_off, text(w), carry, d_desc_, d_status_, d_bad_, st, ms, nullptr, nullptr, why, err);
    decode_ms += ms;
    n = carry + win.text;
    return rc;
}

int BgzfWindows::trim_end(size_t w, uint64_t n, uint64_t &e, bool &unterminated, const char *&why, std::string &err) {
    hipStream_t st = (hipStream_t)st_;
    Tail tail;
    GZCHK(fetch_tail(text(w), n, tail, st));
    GZCHK(hipStreamSynchronize(st));
    return trim_text_end(text(w), n, tail, false, st, e, unterminated, why, err);
}

int BgzfWindows::last_start(size_t w, uint64_t n, uint64_t &at, std::string &err, RecFmt fmt) {
    // the last record start in reach: a start further front leaves more to carry than there is room for
    return device_last_start(text(w), n, (unsigned long long *)d_bad_.p + 4, (hipStream_t)st_, at, err, CARRY_MAX + 64, fmt);
}

int BgzfWindows::first_start(size_t w, uint64_t n, uint64_t from, uint64_t &at, std::string &err, RecFmt fmt) {
    return device_first_start(text(w), n, from, (unsigned long long *)d_bad_.p + 4, (hipStream_t)st_, at, err, fmt);
}

int BgzfWindows::carry_on(size_t w, uint64_t n, uint64_t cut, std::string &err) {
    hipStream_t st = (hipStream_t)st_;
    // the carry goes to the next window's buffer first: the parser wants 32 zero bytes behind the cut
    if (n > cut) GZCHK(hipMemcpyAsync(text(w + 1), text(w) + cut, (size_t)(n - cut), hipMemcpyDeviceToDevice, st));
    GZCHK(hipMemsetAsync(text(w) + cut, 0, 32, st));
    GZCHK(hipStreamSynchronize(st));
    return 0;
}

int BgzfWindows::step(size_t w, bool raw, uint64_t &carry, uint64_t &cut, bool &unterminated, const char *&why, std::string &err) {
    const bool last = w + 1 == chain_->windows.size();
    uint64_t n = 0;
    int rc = inflate(w, !last, carry, n, why, err);
    if (rc) return rc;
    cut = n; unterminated = false;
    if (last) {
        if (!raw) if ((rc = trim_end(w, n, cut, unterminated, why, err))) return rc;
        carry = 0;
        return 0;
    }
    if ((rc = last_start(w, n, cut, err))) return rc;
    if (cut == UINT64_MAX) cut = raw ? n : 0;             // (none.  One record's middle: all of it is carried on, if there is room)
    if (n - cut > CARRY_MAX) {
        if (!raw) { why = "a partial record beyond the room for it"; return 1; }
        cut = n;
    }
    if ((rc = carry_on(w, n, cut, err))) return rc;
    carry = n - cut;
    return 0;
}

// ---- one rank's run of a walked chain, window by window (inflate_gpu.h) ---------------------------------------------------
int BgzfShareWindows::open(const uint8_t *gz, const BgzfChain &chain, uint32_t rank, uint32_t world, uint64_t budget, int device, void *stream,
                           const char *&why, std::string &err, RecFmt fmt) {
    close();
    fmt_ = fmt;
    rank_ = rank; B_ = chain.blocks.size();
    if (rank >= world) { err = "rank beyond world"; return -1; }
    std::vector<uint32_t> isize(B_);
    std::vector<uint64_t> off(B_ + 1, 0);                   // off[b]: the text offset at which block b begins
    for (size_t i = 0; i < B_; i++) { isize[i] = chain.blocks[i].isize; off[i + 1] = off[i] + isize[i]; }
    std::vector<uint64_t> first; uint64_t run_end = 0;
    if (plan_share_windows(isize.data(), B_, world, rank, budget, first, run_end)) { why = "a BGZF block beyond the window budget"; return 1; }
    const size_t b1 = (size_t)run_end, b0 = first.empty() ? b1 : (size_t)first[0];
    c0_ = off[b0]; c1_ = off[b1];
    if (c0_ == c1_) { done_ = true; return 0; }             // (a run without text: s_rank == s_(rank + 1))
    view_.blocks = chain.blocks; view_.text = chain.text; view_.nonempty = chain.nonempty;
    auto window = [&](size_t wb0, size_t wb1) {
        BgzfChain::Window win{wb0, wb1, chain.blocks[wb0].in_off, chain.blocks[wb1 - 1].in_off + chain.blocks[wb1 - 1].bsize, off[wb1] - off[wb0], off[wb0], 0};
        for (size_t b = wb0; b < wb1; b++) win.nonempty += isize[b] != 0;
        view_.windows.push_back(win);
    };
    // the block in front of the run rides with window 0: whether the run's first byte begins a line is written there
    size_t pb = b0;
    while (rank > 0 && pb > 0) { pb--; if (isize[pb]) break; }
    const bool follow = rank + 1 != world && off[B_] > c1_;      // text behind the run: the slice ends in it
    n_own_ = first.size();
    for (size_t w = 0; w < n_own_; w++)
        window(w == 0 ? pb : (size_t)first[w], w + 1 < n_own_ ? (size_t)first[w + 1] : (follow ? b1 : B_ /* empty blocks ride along */));
    // the follow-on blocks of run rank + 1: 2 non-empty ones first, then twice as many while the boundary is undecided, up to
    // CARRY_MAX of text (gpu_bgzf_slice widens its view the same way; here every widening is a small window of its own)
    if (follow) {
        uint64_t text = 0;
        for (size_t tb = b1, extra = 2; tb < B_ && text < BgzfWindows::CARRY_MAX; extra *= 2) {
            size_t te = tb;
            for (size_t got = 0; te < B_ && got < extra && text < BgzfWindows::CARRY_MAX; te++) { text += isize[te]; got += isize[te] != 0; }
            while (te < B_ && !isize[te]) te++;
            window(tb, te);
            tb = te;
        }
    }
    const int rc = bw_.open(gz, &view_, device, stream, err);
    if (rc == 1) why = "out of device memory";
    if (rc) close();
    return rc;
}

void BgzfShareWindows::close() {
    bw_.close(); first_.put();
    view_ = BgzfChain(); n_own_ = w_ = 0; carry_ = consumed_ = windows_ = 0; started_ = done_ = false;
}

int BgzfShareWindows::next(GpuText &piece, uint64_t &at_out, bool &done, const char *&why, std::string &err) {
    hipStream_t st = (hipStream_t)bw_.stream();
    piece = GpuText(); done = false;
    const uint64_t NONE = UINT64_MAX;
    while (true) {
        if (done_ || w_ >= view_.windows.size()) { done_ = done = true; return 0; }
        const size_t w = w_;
        const BgzfChain::Window &win = view_.windows[w];
        const bool is_tail = w >= n_own_, last_in_list = w + 1 == view_.windows.size(), at_end = win.b1 == B_;
        uint64_t n = 0;
        if (const int rc = bw_.inflate(w, !last_in_list && w + 1 <= n_own_, carry_, n, why, err)) return rc;
        windows_++;
        const uint64_t base = win.text_before - carry_;     // where text(w)[0] lies in the file's text
        uint64_t lim = n; bool unterm = false;
        if (last_in_list && at_end) if (const int rc = bw_.trim_end(w, n, lim, unterm, why, err)) return rc;
        // all that is left of this window goes to the front of the next one (nothing could be decided in it)
        auto carry_all = [&](uint64_t from, const char *too_much) -> int {
            if (n - from > BgzfWindows::CARRY_MAX) { why = too_much; return 1; }
            if (const int rc = bw_.carry_on(w, n, from, err)) return rc;
            carry_ = n - from; w_++;
            return 0;
        };
        uint64_t lo = 0;
        if (!started_) {                                    // s_rank: the first record start at or after the run's first byte
            if (rank_ > 0) {
                uint64_t at = NONE;
                if (const int rc = bw_.first_start(w, lim, c0_ - base, at, err, fmt_)) return rc;
                if (at == NONE) {
                    if (last_in_list && at_end) { done_ = done = true; return 0; }      // (no record begins in the run or behind it)
                    if (last_in_list) { why = "no record start within reach"; return 1; }
                    if (const int rc = carry_all(0, "no record start in a whole window")) return rc;
                    continue;
                }
                lo = at;
            }
            started_ = true;
        }
        uint64_t hi = lim; bool fin = true, unt = unterm;
        if (is_tail) {                                      // s_(rank + 1): the first record start at or after the next run's first byte
            uint64_t at = NONE;
            if (const int rc = bw_.first_start(w, lim, std::max(c1_ - base, lo), at, err, fmt_)) return rc;
            if (at == NONE && !(last_in_list && at_end)) {
                if (last_in_list) { why = "no record start within reach behind the run"; return 1; }
                if (const int rc = carry_all(lo, "no record start within reach behind the run")) return rc;
                consumed_ = base + lo;
                continue;
            }
            if (at != NONE) { hi = at; unt = false; }
        } else if (!last_in_list) {                         // a window of the run with more behind it: cut at its last record start
            uint64_t cut = NONE;
            if (const int rc = bw_.last_start(w, n, cut, err, fmt_)) return rc;
            if (cut == NONE || cut < lo) cut = lo;
            if (const int rc = carry_all(cut, "a partial record beyond the room for it")) return rc;
            hi = cut; fin = false; unt = false;
        }
        if (fin) w_ = view_.windows.size();
        if (hi < lo) hi = lo;
        consumed_ = base + hi;
        if (hi == lo) continue;
        at_out = base + lo;
        piece.e = (size_t)(hi - lo); piece.unterminated = fin && unt;
        if (lo == 0) {
            piece.d = bw_.text(w);
            if (fin) GZCHK(hipMemsetAsync(piece.d + hi, 0, 32, st));
        } else {                                            // (the parser wants its text at a 16-byte boundary)
            if (!first_.get((size_t)(hi - lo) + 64)) { why = "out of device memory"; return 1; }
            GZCHK(hipMemcpyAsync(first_.p, bw_.text(w) + lo, (size_t)(hi - lo), hipMemcpyDeviceToDevice, st));
            GZCHK(hipMemsetAsync((uint8_t *)first_.p + (hi - lo), 0, 32, st));
            piece.d = (uint8_t *)first_.p;
        }
        GZCHK(hipStreamSynchronize(st));
        return 0;
    }
}

int gpu_last_record_start(const uint8_t *t, size_t n, int device, uint64_t &at, std::string &err) {
    hipStream_t st = nullptr;
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); err = "hipSetDevice failed"; return -5; }
    PoolBlock d_text, d_out;
    if (!d_text.get(n + 64) || !d_out.get(64)) { err = "out of device memory"; return -4; }
    if (n) GZCHK(hipMemcpyAsync(d_text.p, t, n, hipMemcpyHostToDevice, st));
    const int rc = device_last_start((const uint8_t *)d_text.p, n, (unsigned long long *)d_out.p, st, at, err);
    (void)hipStreamSynchronize(st);
    return rc;
}

int gpu_first_record_start(const uint8_t *t, size_t n, uint64_t from, int device, uint64_t &at, std::string &err) {
    hipStream_t st = nullptr;
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); err = "hipSetDevice failed"; return -5; }
    PoolBlock d_text, d_out;
    if (!d_text.get(n + 64) || !d_out.get(64)) { err = "out of device memory"; return -4; }
    if (n) GZCHK(hipMemcpyAsync(d_text.p, t, n, hipMemcpyHostToDevice, st));
    const int rc = device_first_start((const uint8_t *)d_text.p, n, from, (unsigned long long *)d_out.p, st, at, err);
    (void)hipStreamSynchronize(st);
    return rc;
}

// (the text lies n % 16 bytes behind a 16-byte boundary: texts of every length mod 16 so meet every alignment of the kernel's
// head and tail groups)
int gpu_fasta_record_start(const uint8_t *t, size_t n, bool last, uint64_t from, int device, uint64_t &at, std::string &err) {
    hipStream_t st = nullptr;
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); err = "hipSetDevice failed"; return -5; }
    PoolBlock d_text, d_out;
    if (!d_text.get(n + 64) || !d_out.get(64)) { err = "out of device memory"; return -4; }
    uint8_t *d = (uint8_t *)d_text.p + (n & 15);
    if (n) GZCHK(hipMemcpyAsync(d, t, n, hipMemcpyHostToDevice, st));
    const int rc = last ? device_last_start(d, n, (unsigned long long *)d_out.p, st, at, err, UINT64_MAX, RecFmt::Fasta)
                        : device_first_start(d, n, from, (unsigned long long *)d_out.p, st, at, err, RecFmt::Fasta);
    (void)hipStreamSynchronize(st);
    return rc;
}

// ---- slices for the sharded FASTQ entry point (inflate_gpu.h) -----------------------------------------------------------
int gpu_bgzf_slice(const uint8_t *gz, const BgzfChain &chain, uint32_t rank, uint32_t world, int device, void *stream, DevSpan &out,
                   uint64_t &uploaded, const char *&why, std::string &err, RecFmt fmt) {
    hipStream_t st = (hipStream_t)stream;
    out.blk.put(); out.off = out.len = 0; out.unterminated = false;
    uploaded = 0;
    const size_t B = chain.blocks.size();
    if (rank >= world) { err = "rank beyond world"; return -1; }
    if (chain.text == 0) return 0;                          // (no text: every slice is empty)
    std::vector<uint32_t> isize(B);
    for (size_t i = 0; i < B; i++) isize[i] = chain.blocks[i].isize;
    std::vector<uint64_t> first;
    plan_fastq_slices(isize.data(), B, world, first);
    const size_t b0 = (size_t)first[rank], b1 = (size_t)first[rank + 1];
    // the block in front of the run is inflated too: whether the run's first byte begins a line is written there
    size_t pb = b0;
    while (rank > 0 && pb > 0) { pb--; if (isize[pb]) break; }
    uint64_t lead = 0, own = 0;
    for (size_t b = pb; b < b0; b++) lead += isize[b];
    for (size_t b = b0; b < b1; b++) own += isize[b];
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); err = "hipSetDevice failed"; return -5; }
    const bool last_rank = rank + 1 == world;
    // the follow-on blocks of run rank + 1, in which this slice ends: 2 first, then twice as many, up to CARRY_MAX of text
    for (size_t extra = last_rank ? 0 : 2;; extra *= 2) {
        size_t ve = b1;                                     // the view: blocks [pb, ve)
        uint64_t follow = 0;
        for (size_t got = 0; ve < B && got < extra && follow < BgzfWindows::CARRY_MAX; ve++) { follow += isize[ve]; got += isize[ve] != 0; }
        while (ve < B && !isize[ve]) ve++;                  // (empty blocks at the end of the file ride along: the view then reaches the end)
        const bool at_end = ve == B;
        const uint64_t n_view = lead + own + follow;
        uint32_t nb = 0;
        for (size_t b = pb; b < ve; b++) nb += isize[b] != 0;
        if (!nb) return 0;                                  // (only empty blocks from here to the end of the file)
        const uint64_t in_base = chain.blocks[pb].in_off;
        const size_t in_n = (size_t)(chain.blocks[ve - 1].in_off + chain.blocks[ve - 1].bsize - in_base);
        if (n_view >= (1ull << 32) - 64 || in_n >= ((size_t)1 << 34)) { why = "a slice beyond 4 GiB of text"; return 1; }
        PoolBlock d_in, d_desc, d_status, d_bad, d_text;
        if (!d_in.get(((in_n + 3) & ~(size_t)3) + WIN_IN_PAD) || !d_desc.get((size_t)nb * sizeof(BgzfDesc)) || !d_status.get((size_t)nb * 4) ||
            !d_bad.get(128) || !d_text.get((size_t)n_view + 64)) { why = "out of device memory"; return 1; }
        // (on every way out of this attempt the stream is idle before the blocks go back to the pool: GZCHK waits)
        GZCHK(hipMemsetAsync((char *)d_in.p + (in_n & ~(size_t)3), 0, ((in_n + 3) & ~(size_t)3) - (in_n & ~(size_t)3) + WIN_IN_PAD, st));
        GZCHK(hipMemcpyAsync(d_in.p, gz + in_base, in_n, hipMemcpyHostToDevice, st));
        GZCHK(hipMemsetAsync((char *)d_text.p + n_view, 0, 64, st));
        uploaded += in_n;
        double ms = 0;
        Tail tail;
        if (const int rc = inflate_block_run(chain, pb, ve, d_in.p, in_base, (uint8_t *)d_text.p, 0, d_desc, d_status, d_bad, st, ms, nullptr, at_end ? &tail : nullptr, why, err)) return rc;
        uint64_t e = n_view; bool unterminated = false;
        if (at_end) if (const int rc = trim_text_end((uint8_t *)d_text.p, n_view, tail, false, st, e, unterminated, why, err)) return rc;
        // s_rank inside the own run (or behind it), s_(rank + 1) inside the follow-on text
        uint64_t s[2] = {0, e};
        bool widen = false;
        for (int i = 0; i < 2; i++) {
            if (i == 0 ? rank == 0 : last_rank) continue;
            const uint64_t from = i == 0 ? lead : lead + own;
            uint64_t at = UINT64_MAX;
            if (const int rc = device_first_start((const uint8_t *)d_text.p, e, from, (unsigned long long *)d_bad.p + 8, st, at, err, fmt)) return rc;
            if (at == UINT64_MAX && !at_end) { widen = true; break; }
            s[i] = at == UINT64_MAX ? e : at;
        }
        if (widen) {
            if (follow >= BgzfWindows::CARRY_MAX) { why = "no record start within reach behind the run"; return 1; }
            GZCHK(hipStreamSynchronize(st));
            continue;
        }
        if (rank == 0) s[0] = 0;
        if (s[0] > s[1]) s[0] = s[1];
        out.off = s[0]; out.len = s[1] - s[0];
        out.unterminated = at_end && s[1] == e && unterminated && out.len != 0;
        out.blk = std::move(d_text);
        GZCHK(hipStreamSynchronize(st));
        return 0;
    }
}

int gpu_text_slice(GpuText &text, uint32_t rank, uint32_t world, void *stream, DevSpan &out, std::string &err, RecFmt fmt) {
    hipStream_t st = (hipStream_t)stream;
    out.blk.put(); out.off = out.len = 0; out.unterminated = false;
    if (rank >= world) { err = "rank beyond world"; return -1; }
    const uint64_t e = text.e;
    PoolBlock d_out;
    if (!d_out.get(64)) { err = "out of device memory"; return -4; }
    uint64_t s[2] = {0, e};
    for (int i = 0; i < 2; i++) {
        const uint32_t r = rank + (uint32_t)i;
        if (r == 0 || r == world) continue;
        uint64_t at = UINT64_MAX;
        if (const int rc = device_first_start(text.d, e, slice_cut(e, r, world), (unsigned long long *)d_out.p, st, at, err, fmt)) return rc;
        s[i] = at == UINT64_MAX ? e : at;
    }
    out.off = s[0]; out.len = s[1] - s[0];
    out.unterminated = s[1] == e && text.unterminated && out.len != 0;
    out.blk = PoolBlock(text.d, text.pool_bytes);             // the text's block is the span's now
    text = GpuText();
    return 0;
}

int gpu_span_piece(const DevSpan &span, uint64_t from, uint64_t want, void *stream, GpuText &out, uint64_t &next, std::string &err, RecFmt fmt) {
    hipStream_t st = (hipStream_t)stream;
    out = GpuText();
    next = span.len;
    if (from >= span.len) return 0;
    if (span.len - from > want) {
        PoolBlock d_out;
        if (!d_out.get(64)) { err = "out of device memory"; return -4; }
        uint64_t at = UINT64_MAX;
        // (the search stays inside the piece: it never looks further front than `want` bytes)
        if (const int rc = device_last_start((const uint8_t *)span.blk.p, span.off + from + want, (unsigned long long *)d_out.p, st, at, err, want, fmt)) return rc;
        if (at == UINT64_MAX || at <= span.off + from) {
            if (fmt == RecFmt::Fasta) {                     // one record beyond `want`: next = where it ends, for the caller's message
                if (const int rc = device_first_start((const uint8_t *)span.blk.p, span.off + span.len, span.off + from + 1, (unsigned long long *)d_out.p, st, at, err, fmt)) return rc;
                next = at == UINT64_MAX ? span.len : at - span.off;
            }
            return 1;
        }
        next = at - span.off;
    }
    const uint64_t len = next - from;
    PoolBlock blk;
    if (!blk.get((size_t)len + 64)) { err = "out of device memory for the FASTQ text"; return -4; }
    GZCHK(hipMemcpyAsync(blk.p, (const uint8_t *)span.blk.p + span.off + from, (size_t)len, hipMemcpyDeviceToDevice, st));
    GZCHK(hipMemsetAsync((uint8_t *)blk.p + len, 0, 32, st));
    GZCHK(hipStreamSynchronize(st));
    out.pool_bytes = blk.bytes; out.d = (uint8_t *)blk.take();
    out.e = (size_t)len; out.unterminated = next == span.len && span.unterminated;
    return 0;
}

int gpu_join_spans(const DevSpan *spans, int n_spans, void *stream, GpuText &out, std::string &err) {
    hipStream_t st = (hipStream_t)stream;
    out = GpuText();
    uint64_t total = 0;
    for (int i = 0; i < n_spans; i++) total += spans[i].len + 1;
    PoolBlock blk;
    if (!blk.get((size_t)total + 32)) { err = "out of device memory for the FASTQ text"; return -4; }
    out.pool_bytes = blk.bytes; out.d = (uint8_t *)blk.take();
    uint64_t at = 0;
    for (int i = 0; i < n_spans; i++) {
        if (!spans[i].len) continue;
        if (out.unterminated) { GZCHK(hipMemsetAsync(out.d + at, '\n', 1, st)); at++; }      // (a file that ends without a newline)
        GZCHK(hipMemcpyAsync(out.d + at, (const uint8_t *)spans[i].blk.p + spans[i].off, (size_t)spans[i].len, hipMemcpyDeviceToDevice, st));
        at += spans[i].len;
        out.unterminated = spans[i].unterminated;
    }
    GZCHK(hipMemsetAsync(out.d + at, 0, 32, st));
    GZCHK(hipStreamSynchronize(st));
    out.e = (size_t)at;
    return 0;
}

}  // namespace shk
