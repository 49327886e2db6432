// writer_text_gpu.h — the device writer FROM CONTIG TEXT ALONE: the device twin of the host writer (outputs.cpp:
// build_assembly_text), for callers that hold no graph — the sharded assembly, whose graph lives on other ranks, and
// shk_device_assembly_json.  (included by pipeline.hip inside namespace shk, after writer_gpu.h)
//
// writer_gpu.h takes its links from the one-GPU graph and relies on k_emit to spell every contig on its canonical strand.
// Here the contigs come on an arbitrary strand and nothing but their text is known: the strand is chosen and the text
// turned IN PLACE (SPEC S10), the order is writer_gpu.h's (k_w_keys, the sort, k_w_ties, k_w_rank), the links are found
// the host writer's way — a table of the first k-mers of both orientations of every contig, probed with the four
// successors of every last k-mer (SPEC S11; end_keys.h) — and everything behind the links is writer_gpu.h's again.
// (end_keys.h — the packing of the end k-mers and the table word, shared with the host — is included by pipeline.hip)
#pragma once

__device__ __forceinline__ char w_comp(char c) { return c == 'A' ? 'T' : (c == 'C' ? 'G' : (c == 'G' ? 'C' : 'A')); }

// ---- canonical strand: is revcomp(s) < s?  Decided at the first i with s[i] != comp(s[n-1-i]); such an i and n-1-i come
// in pairs, so the first one lies in the first half (an odd length always has one: its middle base).  One wave per contig,
// 64 positions a step, a ballot for the first difference: a 50-base contig costs one step, a 5 Mbp contig is decided within
// its first bases.  flip[c] = 1: the contig is to be reverse-complemented.
__global__ __launch_bounds__(256) void k_t_strand(const char *__restrict__ text, const WContig *__restrict__ c, uint32_t n,
                                                  uint8_t *__restrict__ flip) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t i = wave; i < n; i += n_waves) {                        // (wave-uniform: all 64 lanes take the same contigs)
        const WContig x = c[i];
        const char *s = text + x.off;
        const unsigned long long len = x.len, half = (len + 1ull) / 2ull;
        uint32_t verdict = 0;
        for (unsigned long long base = 0; base < half; base += 64ull) {
            const unsigned long long j = base + lane;
            char a = 0, b = 0;
            if (j < half) { a = w_comp(s[len - 1ull - j]); b = s[j]; }
            const unsigned long long differ = __ballot(a != b);
            if (differ) {
                const int first = __ffsll((long long)differ) - 1;
                verdict = (uint32_t)__shfl((int)(a < b ? 1 : 0), first);
                break;
            }
        }
        if (lane == 0) flip[i] = (uint8_t)verdict;
    }
}
// the flagged contigs are reverse-complemented in place: the thread of position j < len / 2 swaps and complements j and
// len-1-j, the middle base of an odd length is complemented alone — every byte has exactly one writer, and that writer is
// the only reader of the two bytes.  Work is dealt by 8-byte pieces of the text (c is in text order: bisection, as in
// k_w_copy_seqs), so that a contig of megabases is turned by the whole grid.
__global__ __launch_bounds__(256) void k_t_revcomp(char *__restrict__ text, unsigned long long n_bytes, const WContig *__restrict__ c, uint32_t n,
                                                   const uint8_t *__restrict__ flip) {
    const unsigned long long n_chunks = (n_bytes + 7ull) / 8ull;
    for (unsigned long long q = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; q < n_chunks; q += (unsigned long long)gridDim.x * blockDim.x) {
        unsigned long long p = q * 8ull;
        const unsigned long long pe = p + 8ull < n_bytes ? p + 8ull : n_bytes;
        uint32_t lo = 0, hi = n;                                   // the contig holding byte p
        while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (c[mid].off <= p) lo = mid; else hi = mid; }
        while (p < pe && lo < n) {
            const WContig x = c[lo];
            const unsigned long long len = x.len;
            const unsigned long long end = x.off + len < pe ? x.off + len : pe;
            if (p < x.off) p = x.off;                              // (bytes between two contigs belong to nobody)
            if (flip[lo]) {
                char *s = text + x.off;
                for (; p < end; p++) {
                    const unsigned long long j = p - x.off;
                    if (j < len / 2ull) { const char u = s[j], v = s[len - 1ull - j]; s[j] = w_comp(v); s[len - 1ull - j] = w_comp(u); }
                    else if ((len & 1ull) && j == len / 2ull) s[j] = w_comp(s[j]);
                }
            }
            p = end > p ? end : p;
            lo++;
        }
    }
}

// ---- links from the contig ends (SPEC S11) ------------------------------------------------------------------------------
// the first k-mer of (sorted position r, orientation o): of '-' the reverse complement of the contig's last k-mer
template <int W> __device__ __forceinline__ Kmer<W> t_first_key(const char *__restrict__ text, const WContig &x, uint32_t o, uint32_t k) {
    return o ? ek_pack_rc<W>(text + x.off + (x.len - k), k) : ek_pack<W>(text + x.off, k);
}
// the table: one 64-bit word per slot (end_keys.h: fingerprint | orientation | sorted position), open addressing, linear
// probing, at most half full.  An entry's full key is recomputed from the text, and only when the fingerprints agree.  A slot,
// once taken, keeps its key: of several entries with that key the smallest word survives (atomicMin) — order-free.
template <int W>
__global__ __launch_bounds__(256) void k_t_table_fill(const char *__restrict__ text, const WContig *__restrict__ c, uint32_t n,
                                                      const uint32_t *__restrict__ vals, uint32_t k,
                                                      unsigned long long *__restrict__ table, unsigned long long mask) {
    const unsigned long long total = 2ull * n;
    for (unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (unsigned long long)gridDim.x * blockDim.x) {
        const uint32_t r = (uint32_t)(t >> 1), o = (uint32_t)t & 1u;
        const Kmer<W> key = t_first_key<W>(text, c[vals[r]], o, k);
        const uint64_t h = km_hash<W>(key);
        const unsigned long long e = ek_entry(h, o, r);
        unsigned long long s = h & mask;
        for (unsigned long long probes = 0; probes <= mask; probes++, s = (s + 1ull) & mask) {
            unsigned long long cur = table[s];
            if (cur == EK_EMPTY) { cur = atomicCAS(&table[s], EK_EMPTY, e); if (cur == EK_EMPTY) break; }
            if ((cur >> 32) == (e >> 32) && km_eq<W>(t_first_key<W>(text, c[vals[ek_entry_pos(cur)]], ek_entry_orientation(cur), k), key)) {
                atomicMin(&table[s], e);
                break;
            }
        }
    }
}
template <int W>
__device__ __forceinline__ unsigned long long t_lookup(const char *__restrict__ text, const WContig *__restrict__ c, const uint32_t *__restrict__ vals,
                                                       uint32_t k, const unsigned long long *__restrict__ table, unsigned long long mask, const Kmer<W> &key) {
    const uint64_t h = km_hash<W>(key);
    const unsigned long long f = ek_fingerprint(h);
    unsigned long long s = h & mask;
    for (unsigned long long probes = 0; probes <= mask; probes++, s = (s + 1ull) & mask) {
        const unsigned long long cur = table[s];
        if (cur == EK_EMPTY) return EK_EMPTY;
        if ((cur >> 32) == f && km_eq<W>(t_first_key<W>(text, c[vals[ek_entry_pos(cur)]], ek_entry_orientation(cur), k), key)) return cur;
    }
    return EK_EMPTY;
}
// for every (r, o): the last k-mer of that orientation, its first base dropped, each of A C G T appended — a hit is a link,
// written as the smaller of itself and its mirror (w_link_pack: the word orders as the host's tuple does)
template <int W>
__global__ __launch_bounds__(256) void k_t_links(const char *__restrict__ text, const WContig *__restrict__ c, uint32_t n,
                                                 const uint32_t *__restrict__ vals, uint32_t k,
                                                 const unsigned long long *__restrict__ table, unsigned long long mask,
                                                 unsigned long long *__restrict__ links, unsigned int *__restrict__ n_links, uint32_t cap) {
    const int lane = threadIdx.x & 63;
    const unsigned long long total = 2ull * n;
    const unsigned long long n_round = (total + 63ull) & ~63ull;
    for (unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; t < n_round; t += (unsigned long long)gridDim.x * blockDim.x) {
        unsigned long long found[4]; uint32_t nf = 0;
        if (t < total) {
            const uint32_t r = (uint32_t)(t >> 1), o = (uint32_t)t & 1u;
            const WContig x = c[vals[r]];
            // the last k-mer of '+' is the contig's last, of '-' the reverse complement of its first
            Kmer<W> cand = ek_successor_a<W>(o ? ek_pack_rc<W>(text + x.off, k) : ek_pack<W>(text + x.off + (x.len - k), k), k);
            for (uint32_t b = 0; b < 4; b++) {
                cand.w[0] = (cand.w[0] & ~3ull) | (uint64_t)b;
                const unsigned long long hit = t_lookup<W>(text, c, vals, k, table, mask, cand);
                if (hit == EK_EMPTY) continue;
                const uint32_t rj = ek_entry_pos(hit), oj = ek_entry_orientation(hit);
                const unsigned long long L = w_link_pack(r + 1u, o, rj + 1u, oj), M = w_link_pack(rj + 1u, oj ^ 1u, r + 1u, o ^ 1u);
                found[nf++] = M < L ? M : L;
            }
        }
        // wave-aggregated append (as k_w_links)
        uint32_t incl = nf;
        for (int d = 1; d < 64; d <<= 1) { const uint32_t y = (uint32_t)__shfl_up((int)incl, d); if (lane >= d) incl += y; }
        const uint32_t tot = (uint32_t)__shfl((int)incl, 63);
        uint32_t base = 0;
        if (lane == 63 && tot) base = atomicAdd(n_links, tot);
        base = (uint32_t)__shfl((int)base, 63);
        const uint32_t at = base + incl - nf;
        for (uint32_t q = 0; q < nf; q++) if (at + q < cap) links[at + q] = found[q];
    }
}
