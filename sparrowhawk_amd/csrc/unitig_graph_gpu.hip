// unitig_graph_gpu.hip — SPEC S9 on unitig records as gfx950 kernels: the device twin of UG<W> in unitig_graph.cpp
// (unitig_graph.h says why the rules are exact at this level).  The k-mer-level kernels of graph_part.h are the model:
// 256-thread workgroups, grid-stride loops, candidate lists compacted by ballot, counts that stay on the device, a round
// that decides on a snapshot and applies afterwards.  What differs is the vertex: a record with a length and a summed
// count, whose neighbours are found once through an index of chain starts instead of through adjacency bits.
//
// Every loop is bounded whatever the records say: probes by the capacity of the index, walks by 2k steps (a step adds at
// least one node to a length that may not exceed 2k), lists of tips by the number of tips, rounds by 32.
//
// S10 follows on the device too (the twin of chains_t): predecessors, every record's head, index and node offset by
// pointer jumping — one plain launch per round, each round from one set of arrays into the other, at most
// ceil(log2 n) + 1 of them —, the strand choice at the tails, three exclusive sums over the heads in ascending record
// number (contig index, record offset, text offset), and a placement per record.  What comes home is the flat form of
// UnitigGraphResult; only the ring records (a handful) go through the host's ring loops.  SHK_UNITIG_CHAINS_DEVICE=0
// keeps the earlier way: alive / mirror / succ go home and unitig_chains walks.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include "device_mem.h"
#include "kmer.h"
#include "unitig_graph_gpu.h"

namespace shk {
namespace {

constexpr unsigned long long UG_EMPTY = ~0ull;
// flags word (ctl[0])
constexpr unsigned int UGF_NO_MIRROR = 1u, UGF_SAME_START = 2u, UGF_UNPAIRED = 4u, UGF_PROBE_BOUND = 8u;
// ctl: 8 words of 8 bytes — [0] flags, [1] tip candidates, [2] tips, [3] fork candidates, [4] nodes removed as tips,
// [5] nodes removed as bubble branches (this round)
constexpr int CTL_FLAGS = 0, CTL_NCAND = 1, CTL_NTIPS = 2, CTL_NFORK = 3, CTL_TIP_NODES = 4, CTL_BUB_NODES = 5, CTL_WORDS = 8;

struct UTip { uint32_t start, junction, nrec, next; unsigned long long len, sum; };

// The records as structure-of-arrays (word w of record r's first k-mer: F[w * n + r]) and the links found for them.
template <int W> struct UGraph {
    const uint64_t *F, *T, *len, *kc;
    const uint8_t *circ;
    uint32_t *mirror;                          // [n]
    uint32_t *outn;                            // [n][4], ascending record numbers, UG_NIL padded
    uint8_t *alive;                            // [n]
    uint32_t n;
    int k;

    __device__ __forceinline__ Kmer<W> first(uint32_t r) const {
        Kmer<W> x;
#pragma unroll
        for (int i = 0; i < W; i++) x.w[i] = F[(size_t)i * n + r];
        return x;
    }
    __device__ __forceinline__ Kmer<W> last(uint32_t r) const {
        Kmer<W> x;
#pragma unroll
        for (int i = 0; i < W; i++) x.w[i] = T[(size_t)i * n + r];
        return x;
    }
    // the alive out-neighbours of r's last node: bit b of the mask says entry b of o is one (UG::outs without the compaction;
    // the order of the entries is the host's)
    __device__ __forceinline__ uint32_t outs(uint32_t r, uint4 &o) const {
        o = make_uint4(UG_NIL, UG_NIL, UG_NIL, UG_NIL);
        if (circ[r]) return 0u;
        o = *reinterpret_cast<const uint4 *>(outn + (size_t)r * 4);
        uint32_t m = 0;
        if (o.x != UG_NIL && alive[o.x]) m |= 1u;
        if (o.y != UG_NIL && alive[o.y]) m |= 2u;
        if (o.z != UG_NIL && alive[o.z]) m |= 4u;
        if (o.w != UG_NIL && alive[o.w]) m |= 8u;
        return m;
    }
    __device__ __forceinline__ uint32_t outdeg(uint32_t r) const { uint4 o; return (uint32_t)__popc(outs(r, o)); }
    // in-degree of r's first node: the out-degree of its mirror strand's last node
    __device__ __forceinline__ uint32_t indeg(uint32_t r) const { return circ[r] ? 0u : outdeg(mirror[r]); }
    // the one alive out-neighbour (outs() returned a mask of one bit)
    static __device__ __forceinline__ uint32_t only(const uint4 &o, uint32_t m) {
        return (m & 1u) ? o.x : (m & 2u) ? o.y : (m & 4u) ? o.z : o.w;
    }
    static __device__ __forceinline__ uint32_t entry(const uint4 &o, int b) { return b == 0 ? o.x : b == 1 ? o.y : b == 2 ? o.z : o.w; }
};

__device__ __forceinline__ void ug_compact(bool p, uint32_t value, uint32_t *__restrict__ list, unsigned int *__restrict__ count) {
    const int lane = threadIdx.x & 63;
    const unsigned long long m = __ballot(p);
    if (!m) return;
    unsigned int base = 0;
    if (lane == 0) base = atomicAdd(count, (unsigned int)__popcll(m));
    base = __shfl(base, 0);
    if (p) list[base + __popcll(m & ((1ull << lane) - 1ull))] = value;
}

// ------------------------------------------------------------------------------------------
// the index of chain starts and the links (UG::init)
// ------------------------------------------------------------------------------------------
template <int W>
__global__ __launch_bounds__(256) void k_ug_insert(UGraph<W> g, unsigned long long *__restrict__ slot, uint64_t cap,
                                                   unsigned int *__restrict__ flags) {
    const uint64_t cmask = cap - 1;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < g.n; r += gridDim.x * blockDim.x) {
        g.alive[r] = 1;
        if (g.circ[r]) continue;                                  // rings have no ends: not indexed
        const Kmer<W> f = g.first(r);
        const uint64_t h = ug_hash_of<W>(ug_prefix<W>(f));
        const unsigned long long mine = (h & 0xFFFFFFFF00000000ull) | (unsigned long long)r;
        uint64_t i = h & cmask, probes = 0;
        for (; probes < cap; probes++, i = (i + 1) & cmask) {
            unsigned long long e = __atomic_load_n(&slot[i], __ATOMIC_RELAXED);
            if (e == UG_EMPTY) { e = atomicCAS(&slot[i], UG_EMPTY, mine); if (e == UG_EMPTY) break; }
            // (e is the slot's entry) a record with the same start: of two such records the later one meets the earlier
            if ((e >> 32) == (mine >> 32) && km_eq<W>(g.first((uint32_t)e), f)) { atomicOr(flags, UGF_SAME_START); break; }
        }
        if (probes == cap) atomicOr(flags, UGF_PROBE_BOUND);
    }
}

template <int W>
__global__ __launch_bounds__(256) void k_ug_links(UGraph<W> g, const unsigned long long *__restrict__ slot, uint64_t cap,
                                                  unsigned int *__restrict__ flags) {
    const uint64_t cmask = cap - 1;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < g.n; r += gridDim.x * blockDim.x) {
        if (g.circ[r]) continue;
        const Kmer<W> t = g.last(r);
        // the mirror strand: the record that starts with revcomp(my last k-mer)
        const Kmer<W> want = km_revcomp<W>(t, g.k);
        const uint64_t hw = ug_hash_of<W>(ug_prefix<W>(want));
        uint32_t m = UG_NIL;
        uint64_t i = hw & cmask, probes = 0;
        for (; probes < cap; probes++, i = (i + 1) & cmask) {
            const unsigned long long e = slot[i];
            if (e == UG_EMPTY) break;
            if ((e >> 32) == (hw >> 32) && km_eq<W>(g.first((uint32_t)e), want)) { m = (uint32_t)e; break; }
        }
        if (probes == cap) atomicOr(flags, UGF_PROBE_BOUND);
        if (m == UG_NIL) { atomicOr(flags, UGF_NO_MIRROR); continue; }
        g.mirror[r] = m;
        // the out-neighbours: the records whose first k-1 bases are my last k-1 bases, kept sorted while they are found
        // (the order of the slots must not show: f0 <= f1 <= f2 <= f3, UG_NIL is the largest number)
        const Kmer<W> sfx = ug_suffix<W>(t, g.k);
        const uint64_t hs = ug_hash_of<W>(sfx);
        uint32_t f0 = UG_NIL, f1 = UG_NIL, f2 = UG_NIL, f3 = UG_NIL, c = 0;
        for (i = hs & cmask, probes = 0; probes < cap; probes++, i = (i + 1) & cmask) {
            const unsigned long long e = slot[i];
            if (e == UG_EMPTY) break;
            if (c < 4 && (e >> 32) == (hs >> 32) && km_eq<W>(ug_prefix<W>(g.first((uint32_t)e)), sfx)) {
                uint32_t x = (uint32_t)e, lo;
                lo = min(f0, x); x = max(f0, x); f0 = lo;
                lo = min(f1, x); x = max(f1, x); f1 = lo;
                lo = min(f2, x); x = max(f2, x); f2 = lo;
                f3 = min(f3, x);
                c++;
            }
        }
        if (probes == cap) atomicOr(flags, UGF_PROBE_BOUND);
        *reinterpret_cast<uint4 *>(g.outn + (size_t)r * 4) = make_uint4(f0, f1, f2, f3);
    }
}

template <int W>
__global__ __launch_bounds__(256) void k_ug_pairs(UGraph<W> g, unsigned int *__restrict__ flags) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < g.n; r += gridDim.x * blockDim.x) {
        if (g.circ[r]) continue;
        const uint32_t m = g.mirror[r];
        if (m >= g.n) continue;                                   // (no mirror: UGF_NO_MIRROR is up already)
        if (g.mirror[m] != r) atomicOr(flags, UGF_UNPAIRED);
    }
}

// ------------------------------------------------------------------------------------------
// tips (UG::tip_round)
// ------------------------------------------------------------------------------------------
template <int W>
__global__ __launch_bounds__(256) void k_ug_tip_candidates(UGraph<W> g, uint32_t *__restrict__ cand, unsigned int *__restrict__ n_cand) {
    const uint64_t T_LEN = 2ull * (uint64_t)g.k;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t n_round = ((uint64_t)g.n + stride - 1) / stride * stride;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_round; i += stride) {
        bool p = false;
        if (i < g.n) {
            const uint32_t r = (uint32_t)i;
            p = g.alive[r] && !g.circ[r] && g.len[r] <= T_LEN && g.outdeg(r) == 1 && g.indeg(r) == 0;
        }
        ug_compact(p, (uint32_t)i, cand, n_cand);
    }
}

template <int W>
__global__ __launch_bounds__(256) void k_ug_tip_walk(UGraph<W> g, const uint32_t *__restrict__ cand, const unsigned int *__restrict__ n_cand_p,
                                                     UTip *__restrict__ tips, unsigned int *__restrict__ n_tips, uint32_t *__restrict__ tip_head) {
    const uint64_t T_LEN = 2ull * (uint64_t)g.k;
    const uint32_t n_cand = *n_cand_p;
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < n_cand; c += gridDim.x * blockDim.x) {
        const uint32_t v = cand[c];
        unsigned long long len = g.len[v], sum = g.kc[v];
        uint32_t cur = v, nrec = 1, J = UG_NIL;
        for (uint64_t step = 0; step < T_LEN; step++) {           // (T_LEN more records of >= 1 node each cannot stay within T_LEN)
            uint4 o;
            const uint32_t m = g.outs(cur, o);
            if (__popc(m) != 1) break;                            // not a tip
            const uint32_t nx = UGraph<W>::only(o, m);
            if (g.indeg(nx) >= 2) { J = nx; break; }
            nrec++; len += g.len[nx]; sum += g.kc[nx]; cur = nx;
            if (len > T_LEN) break;                               // not a tip
        }
        if (J == UG_NIL) continue;
        const uint32_t t = atomicAdd(n_tips, 1u);
        UTip rec; rec.start = v; rec.junction = J; rec.nrec = nrec; rec.len = len; rec.sum = sum;
        rec.next = atomicExch(&tip_head[J], t);
        tips[t] = rec;
    }
}

// per junction on the snapshot: t < d -> all go, t == d -> the best stays; best by (len, sum, smaller canonical first k-mer),
// then — the host keeps the first of fully equal tips, and its candidates ascend — the lower start record
template <int W>
__global__ __launch_bounds__(256) void k_ug_tip_decide(UGraph<W> g, const UTip *__restrict__ tips, const unsigned int *__restrict__ n_tips_p,
                                                       const uint32_t *__restrict__ tip_head, uint8_t *__restrict__ kill) {
    const uint32_t n_tips = *n_tips_p;
    for (uint32_t a = blockIdx.x * blockDim.x + threadIdx.x; a < n_tips; a += gridDim.x * blockDim.x) {
        const UTip me = tips[a];
        const uint32_t d = g.indeg(me.junction);
        int om;
        const Kmer<W> mine = km_canonical<W>(g.first(me.start), g.k, om);
        uint32_t t = 0, walked = 0; bool best = true;
        for (uint32_t b = tip_head[me.junction]; b < n_tips && walked < n_tips; b = tips[b].next, walked++) {
            t++;
            if (b == a) continue;
            const UTip o = tips[b];
            bool better;                                          // is o better than me?
            if (o.len != me.len) better = o.len > me.len;
            else if (o.sum != me.sum) better = o.sum > me.sum;
            else {
                int oo;
                const Kmer<W> theirs = km_canonical<W>(g.first(o.start), g.k, oo);
                if (km_less<W>(theirs, mine)) better = true;
                else if (km_less<W>(mine, theirs)) better = false;
                else better = o.start < me.start;
            }
            if (better) best = false;
        }
        kill[a] = (t == d && best) ? 0 : 1;
    }
}

template <int W>
__global__ __launch_bounds__(256) void k_ug_tip_remove(UGraph<W> g, const UTip *__restrict__ tips, const unsigned int *__restrict__ n_tips_p,
                                                       const uint8_t *__restrict__ kill, uint8_t *__restrict__ mark) {
    const uint32_t n_tips = *n_tips_p;
    for (uint32_t a = blockIdx.x * blockDim.x + threadIdx.x; a < n_tips; a += gridDim.x * blockDim.x) {
        if (!kill[a]) continue;
        const UTip me = tips[a];
        uint32_t cur = me.start;
        for (uint32_t i = 0; i < me.nrec; i++) {                  // the path again (alive is the snapshot's until k_ug_apply)
            mark[cur] = 1;
            if (i + 1 == me.nrec) break;
            uint4 o;
            const uint32_t m = g.outs(cur, o);
            if (__popc(m) != 1) break;
            cur = UGraph<W>::only(o, m);
        }
    }
}

// ------------------------------------------------------------------------------------------
// bubbles (UG::bubble_round)
// ------------------------------------------------------------------------------------------
template <int W>
__global__ __launch_bounds__(256) void k_ug_fork_candidates(UGraph<W> g, uint32_t *__restrict__ cand, unsigned int *__restrict__ n_cand) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t n_round = ((uint64_t)g.n + stride - 1) / stride * stride;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_round; i += stride) {
        bool p = false;
        if (i < g.n) { const uint32_t r = (uint32_t)i; p = g.alive[r] && !g.circ[r] && g.outdeg(r) >= 2; }
        ug_compact(p, (uint32_t)i, cand, n_cand);
    }
}

// a * b > c * d, a * b == c * d in 128 bits (sums of counts are u64, lengths <= 2k)
__device__ __forceinline__ void ug_cross(unsigned long long a, unsigned long long b, unsigned long long c, unsigned long long d, bool &gt, bool &eq) {
    const unsigned long long lh = __umul64hi(a, b), ll = a * b, rh = __umul64hi(c, d), rl = c * d;
    eq = lh == rh && ll == rl;
    gt = lh != rh ? lh > rh : ll > rl;
}

template <int W>
__global__ __launch_bounds__(256) void k_ug_bubble(UGraph<W> g, const uint32_t *__restrict__ cand, const unsigned int *__restrict__ n_cand_p,
                                                   uint8_t *__restrict__ mark) {
    const uint64_t T_LEN = 2ull * (uint64_t)g.k;
    const uint32_t n_cand = *n_cand_p;
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < n_cand; c += gridDim.x * blockDim.x) {
        const uint32_t S = cand[c];
        uint4 ob;
        const uint32_t om = g.outs(S, ob);
        uint32_t first[4], end[4], nrec[4];
        unsigned long long len[4], sum[4];
        bool ok[4];
#pragma unroll
        for (int b = 0; b < 4; b++) {
            ok[b] = false; first[b] = UG_NIL; end[b] = UG_NIL; nrec[b] = 0; len[b] = 0; sum[b] = 0;
            if (!((om >> b) & 1u)) continue;
            const uint32_t bn = UGraph<W>::entry(ob, b);
            if (g.indeg(bn) != 1) continue;
            first[b] = bn;
            unsigned long long l = g.len[bn], s = g.kc[bn];
            uint32_t cur = bn, nr = 1;
            if (l <= T_LEN) {                                     // (else: too long inside the first chain)
                for (uint64_t step = 0; step < T_LEN; step++) {
                    uint4 o;
                    const uint32_t m = g.outs(cur, o);
                    if (__popc(m) != 1) break;                    // dead end or fork
                    const uint32_t nx = UGraph<W>::only(o, m);
                    if (g.indeg(nx) >= 2) { end[b] = nx; ok[b] = true; break; }
                    nr++; l += g.len[nx]; s += g.kc[nx]; cur = nx;
                    if (l > T_LEN) break;                         // too long
                }
            }
            nrec[b] = nr; len[b] = l; sum[b] = s;
        }
#pragma unroll
        for (int a = 0; a < 4; a++) {
            if (!ok[a]) continue;
            const uint32_t E = end[a];
            {   // evaluated only from the side with key(S) <= key(rc(E)): S = last node of record S, E = first node of record E
                int os, oe;
                const Kmer<W> ks = km_canonical<W>(g.last(S), g.k, os), ke = km_canonical<W>(g.first(E), g.k, oe);
                const int oe_m = 1 - oe;
                bool le;
                if (km_less<W>(ks, ke)) le = true; else if (km_less<W>(ke, ks)) le = false; else le = os <= oe_m;
                if (!le) continue;
            }
            int grp = 0; bool best = true;
            int o1;
            const Kmer<W> fa = km_canonical<W>(g.first(first[a]), g.k, o1);
#pragma unroll
            for (int b = 0; b < 4; b++) {
                if (!ok[b] || end[b] != E) continue;
                grp++;
                if (b == a) continue;
                bool gt, eq, better;                              // is b better than a?  exact means by cross-multiplication
                ug_cross(sum[b], len[a], sum[a], len[b], gt, eq);
                if (!eq) better = gt;
                else if (len[b] != len[a]) better = len[b] < len[a];
                else { int o2; better = km_less<W>(km_canonical<W>(g.first(first[b]), g.k, o2), fa); }
                if (better) best = false;
            }
            if (grp >= 2 && !best) {
                uint32_t cur = first[a];
                for (uint32_t i = 0; i < nrec[a]; i++) {
                    mark[cur] = 1;
                    if (i + 1 == nrec[a]) break;
                    uint4 o;
                    const uint32_t m = g.outs(cur, o);
                    if (__popc(m) != 1) break;
                    cur = UGraph<W>::only(o, m);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// apply (UG::kill): one thread per mirror pair, taken at min(r, mirror[r]) — a record that is its own mirror counts once
// ------------------------------------------------------------------------------------------
template <int W>
__global__ __launch_bounds__(256) void k_ug_apply(UGraph<W> g, uint8_t *__restrict__ mark, unsigned long long *__restrict__ nodes) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < g.n; r += gridDim.x * blockDim.x) {
        if (g.circ[r]) continue;
        const uint32_t m = g.mirror[r];
        if (m < r || m >= g.n) continue;
        if (!(mark[r] | mark[m])) continue;
        mark[r] = 0; mark[m] = 0;
        if (!g.alive[r]) continue;
        g.alive[r] = 0; g.alive[m] = 0;
        atomicAdd(nodes, (unsigned long long)g.len[r]);
    }
}

// ------------------------------------------------------------------------------------------
// S10 on what is left (UG::simple_succ)
// ------------------------------------------------------------------------------------------
template <int W>
__global__ __launch_bounds__(256) void k_ug_succ(UGraph<W> g, uint32_t *__restrict__ succ) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < g.n; r += gridDim.x * blockDim.x) {
        uint32_t s = UG_NIL;
        if (g.alive[r] && !g.circ[r]) {
            uint4 o;
            const uint32_t m = g.outs(r, o);
            if (__popc(m) == 1) {
                const uint32_t cand = UGraph<W>::only(o, m);
                if (g.indeg(cand) == 1) {
                    const Kmer<W> f = g.first(cand), t = g.last(r);
                    if (!km_eq<W>(f, t) && !km_eq<W>(f, km_revcomp<W>(t, g.k))) s = cand;
                }
            }
        }
        succ[r] = s;
    }
}

// ------------------------------------------------------------------------------------------
// S10, the walk (chains_t in unitig_graph.cpp): heads, ranks by pointer jumping, the strand choice, the placement
// ------------------------------------------------------------------------------------------
// What the walk reads: the records' first k-mers (word w of record r: F[w * n + r]), lengths and counts, and the settled
// links.  succ is injective on the alive linear records, so they form paths (a head ... a tail) and cycles.
struct UChainIn {
    const uint64_t *F, *len, *kc;
    const uint8_t *circ, *alive;
    const uint32_t *mirror, *succ;
    uint32_t n;
    int k;
    __device__ __forceinline__ bool linear(uint32_t r) const { return alive[r] && !circ[r]; }
};
// The rank of a record while it is being found: `up` is an ancestor (the record itself at a head), idx the records from up
// to it, nodes / kc the sums over [up, r).  One round replaces up by up's up and adds up's sums: the distance doubles, a
// record is finished once its up is a head (pred == UG_NIL).  A round reads one set of arrays and writes the other.
struct URank { uint32_t *up, *idx; unsigned long long *nodes, *kc; };
// ctl of the walk: [0] ring records, [1] contigs, [2] their records, [3] their text, [UC_ROUND0 + j] records unfinished
// after round j (j = 0: before the first)
constexpr int UC_NRING = 0, UC_NCONTIG = 1, UC_NREC = 2, UC_NTEXT = 3, UC_ROUND0 = 8, UC_MAX_ROUNDS = 34, UC_WORDS = UC_ROUND0 + UC_MAX_ROUNDS + 2;

// one atomic per wave: count the lanes with p (every lane of the wave calls)
__device__ __forceinline__ void ug_count(bool p, unsigned long long *count) {
    const unsigned long long m = __ballot(p);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(count, (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(256) void k_uc_pred(UChainIn g, uint32_t *__restrict__ pred) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < g.n; r += gridDim.x * blockDim.x) {
        const uint32_t s = g.succ[r];
        if (s < g.n) pred[s] = r;                                 // (a record has one simple predecessor)
    }
}

__global__ __launch_bounds__(256) void k_uc_init(UChainIn g, const uint32_t *__restrict__ pred, URank a, unsigned long long *__restrict__ unfinished) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t n_round = ((uint64_t)g.n + stride - 1) / stride * stride;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_round; i += stride) {
        bool open = false;
        if (i < g.n) {
            const uint32_t r = (uint32_t)i;
            uint32_t p = g.linear(r) ? pred[r] : UG_NIL;
            if (p >= g.n) p = UG_NIL;
            if (p == UG_NIL) { a.up[r] = r; a.idx[r] = 0; a.nodes[r] = 0; a.kc[r] = 0; }
            else { a.up[r] = p; a.idx[r] = 1; a.nodes[r] = g.len[p]; a.kc[r] = g.kc[p]; open = pred[p] != UG_NIL; }
        }
        ug_count(open, unfinished);
    }
}

__global__ __launch_bounds__(256) void k_uc_jump(UChainIn g, const uint32_t *__restrict__ pred, URank a, URank b, unsigned long long *__restrict__ unfinished) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t n_round = ((uint64_t)g.n + stride - 1) / stride * stride;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_round; i += stride) {
        bool open = false;
        if (i < g.n && g.linear((uint32_t)i)) {
            const uint32_t r = (uint32_t)i;
            uint32_t u = a.up[r], x = a.idx[r];
            unsigned long long nodes = a.nodes[r], kc = a.kc[r];
            if (u < g.n && pred[u] != UG_NIL) {                   // not finished: up's rank is read from the same snapshot
                const uint32_t uu = a.up[u];
                x += a.idx[u]; nodes += a.nodes[u]; kc += a.kc[u];
                u = uu;
                open = u < g.n && pred[u] != UG_NIL;
            }
            b.up[r] = u; b.idx[r] = x; b.nodes[r] = nodes; b.kc[r] = kc;
        }
        ug_count(open, unfinished);
    }
}

// at the tails: the chain's totals, filed under its head — if this strand is the one handed on (S10: the chain that is its
// own mirror strand, else the strand with the smaller first k-mer).  h_cnt / h_text are zero everywhere else.
template <int W>
__global__ __launch_bounds__(256) void k_uc_tails(UChainIn g, const uint32_t *__restrict__ pred, URank a, uint32_t *__restrict__ h_cnt,
                                                  unsigned long long *__restrict__ h_nodes, unsigned long long *__restrict__ h_kc,
                                                  unsigned long long *__restrict__ h_text) {
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < g.n; t += gridDim.x * blockDim.x) {
        if (!g.linear(t) || g.succ[t] != UG_NIL) continue;
        const uint32_t h = a.up[t];
        if (h >= g.n || pred[h] != UG_NIL) continue;              // (no head within the rounds: left to the ring list)
        const uint32_t mf = g.mirror[t];
        bool emit = mf == h;
        if (!emit && mf < g.n) {
            Kmer<W> x, y;
#pragma unroll
            for (int i = 0; i < W; i++) { x.w[i] = g.F[(size_t)i * g.n + h]; y.w[i] = g.F[(size_t)i * g.n + mf]; }
            emit = km_less<W>(x, y);
        }
        if (!emit) continue;
        const unsigned long long nodes = a.nodes[t] + g.len[t];
        h_cnt[h] = a.idx[t] + 1u; h_nodes[h] = nodes; h_kc[h] = a.kc[t] + g.kc[t]; h_text[h] = nodes + (unsigned long long)(g.k - 1);
    }
}

struct UcIsHead { __host__ __device__ __forceinline__ uint32_t operator()(const uint32_t &c) const { return c ? 1u : 0u; } };

// (the scans ran over n + 1 entries, the last one zero: entry n of each is the total)
__global__ void k_uc_totals(uint32_t n, const uint32_t *__restrict__ c_idx, const uint32_t *__restrict__ rec_off,
                            const unsigned long long *__restrict__ text_off, unsigned long long *__restrict__ ctl) {
    if (blockIdx.x == 0 && threadIdx.x == 0) { ctl[UC_NCONTIG] = c_idx[n]; ctl[UC_NREC] = rec_off[n]; ctl[UC_NTEXT] = text_off[n]; }
}

__global__ __launch_bounds__(256) void k_uc_contigs(uint32_t n, const uint32_t *__restrict__ h_cnt, const unsigned long long *__restrict__ h_nodes,
                                                    const unsigned long long *__restrict__ h_kc, const uint32_t *__restrict__ c_idx,
                                                    const uint32_t *__restrict__ rec_off, const unsigned long long *__restrict__ text_off,
                                                    UnitigFlatContig *__restrict__ lin) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) {
        const uint32_t cnt = h_cnt[r];
        if (!cnt) continue;
        const uint32_t c = c_idx[r];
        if (c >= n) continue;
        UnitigFlatContig o;
        o.len_nodes = h_nodes[r]; o.kc = h_kc[r]; o.text_off = text_off[r]; o.rec_off = rec_off[r]; o.head = r; o.n_recs = cnt;
        lin[c] = o;
    }
}

// every record: its placement, its slot in the flat record list — or its entry in the list of ring records (alive, and on no
// chain with a head)
__global__ __launch_bounds__(256) void k_uc_place(UChainIn g, const uint32_t *__restrict__ pred, URank a, const uint32_t *__restrict__ h_cnt,
                                                  const uint32_t *__restrict__ rec_off, const unsigned long long *__restrict__ text_off,
                                                  UnitigPlace *__restrict__ place, uint32_t *__restrict__ recs_flat,
                                                  UnitigRingRec *__restrict__ rings, unsigned long long *__restrict__ n_ring) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t n_round = ((uint64_t)g.n + stride - 1) / stride * stride;
    const int lane = threadIdx.x & 63;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_round; i += stride) {
        bool ring = false;
        const uint32_t r = (uint32_t)i;
        if (i < g.n) {
            UnitigPlace pl; pl.off = ~0ull; pl.node_off = 0;
            if (g.alive[r]) {
                if (g.circ[r]) ring = true;
                else {
                    const uint32_t h = a.up[r];
                    if (h >= g.n || pred[h] != UG_NIL) ring = true;
                    else {
                        const uint32_t cnt = h_cnt[h], x = a.idx[r];
                        if (x < cnt) {                            // (cnt == 0: the mirror strand's chain, dropped)
                            const uint64_t slot = (uint64_t)rec_off[h] + x;
                            if (slot < g.n) { recs_flat[slot] = r; pl.off = text_off[h]; pl.node_off = a.nodes[r]; }
                        }
                    }
                }
            }
            place[r] = pl;
        }
        const unsigned long long m = __ballot(ring);
        if (!m) continue;
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(n_ring, (unsigned long long)__popcll(m));
        base = __shfl(base, 0);
        if (ring) {
            const unsigned long long at = base + __popcll(m & ((1ull << lane) - 1ull));
            if (at < g.n) { UnitigRingRec o; o.r = r; o.succ = g.succ[r]; o.mirror = g.mirror[r]; rings[at] = o; }
        }
    }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
#define UGCHK(call) HIPCHK_AS("unitig graph on the device: " #call, call, (void)0)

// workgroups per launch: two per CU of a 256-CU card (8 waves per CU keep the dependent reads of the probes and walks in
// flight), the rest of the records by the grid stride — from 131 072 records on every thread takes more than one
unsigned ug_grid(uint64_t n) {
    const uint64_t b = (n + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > 512 ? 512 : b));
}

// SHK_UNITIG_CHAINS_DEVICE=0: the chains are walked by the host's unitig_chains, from alive / mirror / succ copied home
bool chains_on_device() { const char *e = getenv("SHK_UNITIG_CHAINS_DEVICE"); return !(e && *e == '0'); }
// (hipcub counts its items in an int; the scans run over n + 1 of them)
constexpr size_t UC_MAX_RECS = 0x7FFFFFFEu;

// the three exclusive sums over the heads, in ascending record number: contig index, offset into the flat record list,
// text offset.  tmp == nullptr: nothing runs, bytes := the largest temporary block one of them asks for
hipError_t uc_scans(void *tmp, size_t &bytes, const uint32_t *h_cnt, const unsigned long long *h_text, uint32_t *c_idx, uint32_t *rec_off,
                    unsigned long long *text_off, int items, hipStream_t st) {
    hipcub::TransformInputIterator<uint32_t, UcIsHead, const uint32_t *> is_head(h_cnt, UcIsHead());
    size_t b0 = bytes, b1 = bytes, b2 = bytes;
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(tmp, b0, is_head, c_idx, items, st);
    if (e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(tmp, b1, h_cnt, rec_off, items, st);
    if (e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(tmp, b2, h_text, text_off, items, st);
    if (!tmp) bytes = std::max(b0, std::max(b1, b2));
    return e;
}

// The device blocks of the walk, out of the caller's scope (taken together with its own, before any work), and the host ends
// of the walk's copies: the caller declares this in front of its PoolScope, so that they outlive the scope's drain.
struct ChainBlocks {
    uint32_t *pred = nullptr, *c_idx = nullptr, *rec_off = nullptr, *flat = nullptr;
    URank rk[2];
    unsigned long long *h_text = nullptr, *text_off = nullptr, *ctl = nullptr;
    UnitigFlatContig *lin = nullptr; UnitigPlace *place = nullptr; UnitigRingRec *rings = nullptr;
    void *tmp = nullptr; size_t tmp_bytes = 0;
    unsigned long long h_ctl[UC_WORDS];
    std::vector<UnitigRingRec> h_rings;
    bool get(PoolScope &sc, size_t n) {
        std::string oom;
        if (uc_scans(nullptr, tmp_bytes, nullptr, nullptr, nullptr, nullptr, nullptr, (int)(n + 1), nullptr) != hipSuccess) return false;
        for (int i = 0; i < 2; i++)
            if (!(rk[i].up = sc.get<uint32_t>(n, oom)) || !(rk[i].idx = sc.get<uint32_t>(n + 1, oom)) ||
                !(rk[i].nodes = sc.get<unsigned long long>(n, oom)) || !(rk[i].kc = sc.get<unsigned long long>(n, oom))) return false;
        return (pred = sc.get<uint32_t>(n, oom)) && (h_text = sc.get<unsigned long long>(n + 1, oom)) && (c_idx = sc.get<uint32_t>(n + 1, oom)) &&
               (rec_off = sc.get<uint32_t>(n + 1, oom)) && (text_off = sc.get<unsigned long long>(n + 1, oom)) && (lin = sc.get<UnitigFlatContig>(n, oom)) &&
               (place = sc.get<UnitigPlace>(n, oom)) && (flat = sc.get<uint32_t>(n, oom)) && (rings = sc.get<UnitigRingRec>(n, oom)) &&
               (tmp = sc.get<uint8_t>(tmp_bytes, oom)) && (ctl = sc.get<unsigned long long>(UC_WORDS, oom));
    }
};

// The walk: out.lin / recs_flat / place / lin_text from the device, the rings through unitig_ring_chains.  The caller holds
// the blocks, and its scope drains the stream on the way out.  One host read per jumping round (the count of unfinished
// records), one of the totals, then the results.
template <int W> int chains_walk_t(const UChainIn &g, const std::vector<UnitigRec> &recs, ChainBlocks &b, hipStream_t st,
                                   UnitigGraphResult &out, std::string &err) {
    const size_t n = g.n;
    const dim3 grid(ug_grid(n)), block(256);
    unsigned long long *ctl = b.ctl, *h_ctl = b.h_ctl;
    uint32_t *pred = b.pred;
    const URank *rk = b.rk;
    std::vector<UnitigRingRec> &rings = b.h_rings;
    UGCHK(hipMemsetAsync(ctl, 0, UC_WORDS * 8, st));
    UGCHK(hipMemsetAsync(pred, 0xFF, n * 4, st));
    hipLaunchKernelGGL(k_uc_pred, grid, block, 0, st, g, pred);
    hipLaunchKernelGGL(k_uc_init, grid, block, 0, st, g, (const uint32_t *)pred, rk[0], ctl + UC_ROUND0);
    UGCHK(hipGetLastError());
    UGCHK(hipMemcpyAsync(h_ctl + UC_ROUND0, ctl + UC_ROUND0, 8, hipMemcpyDeviceToHost, st));
    UGCHK(hipStreamSynchronize(st));
    // every round finishes at least one record of a chain with a head while there is one (the unfinished record nearest
    // to its head has a finished up); the records of a cycle never finish.  So: none left, or a count that did not
    // move — the rest are rings — or ceil(log2 n) + 1 rounds, which no chain of n records needs.
    int max_rounds = 1;
    while (max_rounds < UC_MAX_ROUNDS - 1 && (1ull << (max_rounds - 1)) < n) max_rounds++;
    int cur = 0;
    unsigned long long open = h_ctl[UC_ROUND0];
    for (int round = 1; round <= max_rounds && open; round++) {
        hipLaunchKernelGGL(k_uc_jump, grid, block, 0, st, g, (const uint32_t *)pred, rk[cur], rk[cur ^ 1], ctl + UC_ROUND0 + round);
        UGCHK(hipGetLastError());
        UGCHK(hipMemcpyAsync(h_ctl + UC_ROUND0 + round, ctl + UC_ROUND0 + round, 8, hipMemcpyDeviceToHost, st));
        UGCHK(hipStreamSynchronize(st));
        cur ^= 1;
        const unsigned long long now = h_ctl[UC_ROUND0 + round];
        if (now == open) break;
        open = now;
    }
    // the other set of arrays is free from here on: the totals by head go there
    const URank a = rk[cur], o = rk[cur ^ 1];
    uint32_t *h_cnt = o.idx, *c_idx = b.c_idx, *rec_off = b.rec_off;
    unsigned long long *h_nodes = o.nodes, *h_kc = o.kc, *h_text = b.h_text, *text_off = b.text_off;
    UGCHK(hipMemsetAsync(h_cnt, 0, (n + 1) * 4, st));
    UGCHK(hipMemsetAsync(h_text, 0, (n + 1) * 8, st));
    hipLaunchKernelGGL(k_uc_tails<W>, grid, block, 0, st, g, (const uint32_t *)pred, a, h_cnt, h_nodes, h_kc, h_text);
    UGCHK(hipGetLastError());
    size_t tmp_bytes = b.tmp_bytes;
    UGCHK(uc_scans(b.tmp, tmp_bytes, h_cnt, h_text, c_idx, rec_off, text_off, (int)(n + 1), st));
    hipLaunchKernelGGL(k_uc_totals, dim3(1), dim3(64), 0, st, (uint32_t)n, (const uint32_t *)c_idx, (const uint32_t *)rec_off, (const unsigned long long *)text_off, ctl);
    hipLaunchKernelGGL(k_uc_contigs, grid, block, 0, st, (uint32_t)n, (const uint32_t *)h_cnt, (const unsigned long long *)h_nodes, (const unsigned long long *)h_kc,
                       (const uint32_t *)c_idx, (const uint32_t *)rec_off, (const unsigned long long *)text_off, b.lin);
    hipLaunchKernelGGL(k_uc_place, grid, block, 0, st, g, (const uint32_t *)pred, a, (const uint32_t *)h_cnt, (const uint32_t *)rec_off,
                       (const unsigned long long *)text_off, b.place, b.flat, b.rings, ctl + UC_NRING);
    UGCHK(hipGetLastError());
    UGCHK(hipMemcpyAsync(h_ctl, ctl, 4 * 8, hipMemcpyDeviceToHost, st));
    UGCHK(hipStreamSynchronize(st));
    const size_t n_ring = (size_t)h_ctl[UC_NRING], n_contig = (size_t)h_ctl[UC_NCONTIG], n_rec = (size_t)h_ctl[UC_NREC];
    if (n_ring > n || n_contig > n || n_rec > n) { err = "unitig graph on the device: the walk of the chains counted more than there is"; return -5; }
    out.flat = true;
    out.lin_text = h_ctl[UC_NTEXT];
    out.lin.resize(n_contig); out.recs_flat.resize(n_rec); out.place.resize(n);
    rings.resize(n_ring);
    if (n_contig) UGCHK(hipMemcpyAsync(out.lin.data(), b.lin, n_contig * sizeof(UnitigFlatContig), hipMemcpyDeviceToHost, st));
    if (n_rec) UGCHK(hipMemcpyAsync(out.recs_flat.data(), b.flat, n_rec * 4, hipMemcpyDeviceToHost, st));
    UGCHK(hipMemcpyAsync(out.place.data(), b.place, n * sizeof(UnitigPlace), hipMemcpyDeviceToHost, st));
    if (n_ring) UGCHK(hipMemcpyAsync(rings.data(), b.rings, n_ring * sizeof(UnitigRingRec), hipMemcpyDeviceToHost, st));
    UGCHK(hipStreamSynchronize(st));
    return unitig_ring_chains(recs, std::move(rings), out, err);
}

template <int W> int assemble_device_t(int k, const std::vector<UnitigRec> &recs, bool tips, bool bubbles, hipStream_t st,
                                       UnitigGraphResult &out, std::string &err) {
    const bool dbg = getenv("SHK_UG_DEBUG") != nullptr;            // stage times on stderr, as the host code prints them
    auto t0 = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (!dbg) return;
        (void)hipStreamSynchronize(st);
        const auto t1 = std::chrono::steady_clock::now();
        fprintf(stderr, "[unitig graph, device] %-10s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
        t0 = t1;
    };
    const size_t n = recs.size();
    out = UnitigGraphResult();
    if (n >= (size_t)UG_NIL) { err = "unitig graph: more records than 32-bit record numbers"; return -1; }
    const bool walk = chains_on_device() && n <= UC_MAX_RECS;     // S10 here as well; else the host's walk
    if (n == 0) {                                                 // (nothing to launch; the host makes one empty round)
        if (tips || bubbles) out.rounds = 1;
        out.flat = walk;                                          // (no record: the flat form is the empty one)
        return 0;
    }
    uint64_t cap = 64;
    while (cap < (uint64_t)n * 2 + 16) cap <<= 1;
    // (host ends of the copies: declared first, so that they outlive the drain of the stream on every way out)
    std::vector<uint64_t> h_rec;
    std::vector<uint8_t> h_circ, alive;
    std::vector<uint32_t> mirror, succ;
    unsigned long long h_ctl[CTL_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
    ChainBlocks cb;
    // ---- device blocks: all of them before any work, so that "no memory" leaves nothing behind.  They go back to the pool
    // when this function returns, behind the scope's drain: nothing may still be running on them then
    const size_t rec_words = (size_t)(2 * W + 2) * n;             // first[W][n], last[W][n], len[n], kc[n]
    PoolScope sc(st);
    std::string oom;
    uint64_t *d_rec; uint8_t *d_circ, *d_alive, *d_mark, *d_kill; unsigned long long *d_slot, *d_ctl; uint32_t *d_mirror, *d_outn, *d_succ, *d_cand, *d_head; UTip *d_tips;
    if (!(d_rec = sc.get<uint64_t>(rec_words, oom)) || !(d_circ = sc.get<uint8_t>(n, oom)) || !(d_slot = sc.get<unsigned long long>((size_t)cap, oom)) ||
        !(d_mirror = sc.get<uint32_t>(n, oom)) || !(d_outn = sc.get<uint32_t>(n * 4, oom)) || !(d_alive = sc.get<uint8_t>(n, oom)) ||
        !(d_mark = sc.get<uint8_t>(n, oom)) || !(d_succ = sc.get<uint32_t>(n, oom)) || !(d_cand = sc.get<uint32_t>(n, oom)) ||
        !(d_tips = sc.get<UTip>(n, oom)) || !(d_kill = sc.get<uint8_t>(n, oom)) || !(d_head = sc.get<uint32_t>(n, oom)) ||
        !(d_ctl = sc.get<unsigned long long>(CTL_WORDS, oom)) || (walk && !cb.get(sc, n))) {
        (void)hipGetLastError();
        return 1;
    }
    // ---- records as structure-of-arrays (several host threads from the size on at which the host code uses them)
    h_rec.resize(rec_words); h_circ.resize(n);
    {
        unsigned T = 1;
        if (n >= 65536) { T = std::thread::hardware_concurrency(); T = T < 1 ? 1 : (T > 16 ? 16 : T); }
        auto fill = [&](size_t a, size_t b) {
            uint64_t *F = h_rec.data(), *L = F + (size_t)W * n, *len = L + (size_t)W * n, *kc = len + n;
            for (size_t r = a; r < b; r++) {
                const UnitigRec &R = recs[r];
                for (int w = 0; w < W; w++) { F[(size_t)w * n + r] = R.first[w]; L[(size_t)w * n + r] = R.last[w]; }
                len[r] = R.len; kc[r] = R.kc; h_circ[r] = R.circ ? 1 : 0;
            }
        };
        std::vector<std::thread> ts;
        for (unsigned t = 1; t < T; t++) ts.emplace_back(fill, n * t / T, n * (t + 1) / T);
        fill(0, n / T);
        for (auto &t : ts) t.join();
    }
    lap("transpose");
    UGCHK(hipMemcpyAsync(d_rec, h_rec.data(), rec_words * 8, hipMemcpyHostToDevice, st));
    UGCHK(hipMemcpyAsync(d_circ, h_circ.data(), n, hipMemcpyHostToDevice, st));
    UGCHK(hipMemsetAsync(d_slot, 0xFF, (size_t)cap * 8, st));
    UGCHK(hipMemsetAsync(d_mirror, 0xFF, n * 4, st));
    UGCHK(hipMemsetAsync(d_outn, 0xFF, n * 16, st));
    UGCHK(hipMemsetAsync(d_mark, 0, n, st));
    UGCHK(hipMemsetAsync(d_ctl, 0, CTL_WORDS * 8, st));
    lap("upload");
    UGraph<W> g;
    g.F = d_rec; g.T = g.F + (size_t)W * n; g.len = g.T + (size_t)W * n; g.kc = g.len + n;
    g.circ = d_circ; g.mirror = d_mirror; g.outn = d_outn; g.alive = d_alive;
    g.n = (uint32_t)n; g.k = k;
    unsigned long long *ctl = d_ctl;
    unsigned int *flags = (unsigned int *)(ctl + CTL_FLAGS);
    unsigned int *n_cand = (unsigned int *)(ctl + CTL_NCAND), *n_tips = (unsigned int *)(ctl + CTL_NTIPS), *n_fork = (unsigned int *)(ctl + CTL_NFORK);
    uint8_t *mark = d_mark;
    const dim3 grid(ug_grid(n)), block(256);
    // ---- index and links; one read of the flags
    hipLaunchKernelGGL(k_ug_insert<W>, grid, block, 0, st, g, d_slot, cap, flags);
    hipLaunchKernelGGL(k_ug_links<W>, grid, block, 0, st, g, d_slot, cap, flags);
    hipLaunchKernelGGL(k_ug_pairs<W>, grid, block, 0, st, g, flags);
    UGCHK(hipGetLastError());
    UGCHK(hipMemcpyAsync(h_ctl, ctl, 8, hipMemcpyDeviceToHost, st));
    UGCHK(hipStreamSynchronize(st));
    lap("init");
    {
        const unsigned int f = (unsigned int)h_ctl[CTL_FLAGS];
        if (f & UGF_SAME_START) { err = "unitig graph: two chains start at the same oriented node"; return -1; }
        if (f & UGF_NO_MIRROR) { err = "unitig graph: a chain without its mirror strand"; return -1; }
        if (f & UGF_UNPAIRED) { err = "unitig graph: mirror strands do not pair up"; return -1; }
        if (f & UGF_PROBE_BOUND) { err = "unitig graph: a probe of the index of chain starts did not end"; return -1; }
    }
    // ---- S9 rounds: one host read per round, of the two node counts
    if (tips || bubbles) {
        for (int round = 0; round < 32; round++) {                // MAX_ROUNDS (S9)
            UGCHK(hipMemsetAsync(ctl + 1, 0, (CTL_WORDS - 1) * 8, st));
            if (tips) {
                UGCHK(hipMemsetAsync(d_head, 0xFF, n * 4, st));
                hipLaunchKernelGGL(k_ug_tip_candidates<W>, grid, block, 0, st, g, d_cand, n_cand);
                hipLaunchKernelGGL(k_ug_tip_walk<W>, grid, block, 0, st, g, d_cand, n_cand, d_tips, n_tips, d_head);
                hipLaunchKernelGGL(k_ug_tip_decide<W>, grid, block, 0, st, g, d_tips, n_tips, d_head, d_kill);
                hipLaunchKernelGGL(k_ug_tip_remove<W>, grid, block, 0, st, g, d_tips, n_tips, d_kill, mark);
                hipLaunchKernelGGL(k_ug_apply<W>, grid, block, 0, st, g, mark, ctl + CTL_TIP_NODES);
            }
            if (bubbles) {                                        // on the graph the tip round left
                hipLaunchKernelGGL(k_ug_fork_candidates<W>, grid, block, 0, st, g, d_cand, n_fork);
                hipLaunchKernelGGL(k_ug_bubble<W>, grid, block, 0, st, g, d_cand, n_fork, mark);
                hipLaunchKernelGGL(k_ug_apply<W>, grid, block, 0, st, g, mark, ctl + CTL_BUB_NODES);
            }
            UGCHK(hipGetLastError());
            UGCHK(hipMemcpyAsync(h_ctl + CTL_TIP_NODES, ctl + CTL_TIP_NODES, 16, hipMemcpyDeviceToHost, st));
            UGCHK(hipStreamSynchronize(st));
            const uint64_t a = h_ctl[CTL_TIP_NODES], b = h_ctl[CTL_BUB_NODES];
            out.tips_removed += a; out.bubbles_removed += b; out.rounds++;
            if (a + b == 0) break;
        }
    }
    lap("rounds");
    // ---- simple successors; then the walk of the chains, here —
    hipLaunchKernelGGL(k_ug_succ<W>, grid, block, 0, st, g, d_succ);
    UGCHK(hipGetLastError());
    if (walk) {
        lap("succ");
        UChainIn in;
        in.F = g.F; in.len = g.len; in.kc = g.kc; in.circ = g.circ; in.alive = g.alive; in.mirror = g.mirror; in.succ = d_succ;
        in.n = g.n; in.k = k;
        const int rc = chains_walk_t<W>(in, recs, cb, st, out, err);
        lap("chains");
        return rc;
    }
    // ---- or alive / mirror / succ go home, and the host's own walk makes the contigs
    alive.resize(n); mirror.resize(n); succ.resize(n);
    UGCHK(hipMemcpyAsync(alive.data(), d_alive, n, hipMemcpyDeviceToHost, st));
    UGCHK(hipMemcpyAsync(mirror.data(), d_mirror, n * 4, hipMemcpyDeviceToHost, st));
    UGCHK(hipMemcpyAsync(succ.data(), d_succ, n * 4, hipMemcpyDeviceToHost, st));
    UGCHK(hipStreamSynchronize(st));
    lap("succ");
    const int rc = unitig_chains(k, recs, alive, std::move(mirror), succ, out, err);
    lap("chains");
    return rc;
}

// the walk alone, from settled arrays: first k-mers, lengths, counts and the links go up, the walk runs
template <int W> int chains_device_t(int k, const std::vector<UnitigRec> &recs, const std::vector<uint8_t> &alive, const std::vector<uint32_t> &mirror,
                                     const std::vector<uint32_t> &succ, hipStream_t st, UnitigGraphResult &out, std::string &err) {
    const size_t n = recs.size();
    out = UnitigGraphResult();
    if (alive.size() != n || mirror.size() != n || succ.size() != n) { err = "unitig graph: arrays of another size than the records"; return -1; }
    if (n > UC_MAX_RECS) { err = "unitig graph: more records than the walk on the device takes"; return -1; }
    if (n == 0) { out.flat = true; return 0; }
    std::vector<uint64_t> h_rec;                                  // (declared first: outlives the drain of the stream)
    std::vector<uint8_t> h_circ;
    const size_t rec_words = (size_t)(W + 2) * n;                 // first[W][n], len[n], kc[n]
    ChainBlocks cb;
    PoolScope sc(st);                                             // (drains the stream before the blocks go back)
    std::string oom;
    uint64_t *d_rec; uint8_t *d_circ, *d_alive; uint32_t *d_mirror, *d_succ;
    if (!(d_rec = sc.get<uint64_t>(rec_words, oom)) || !(d_circ = sc.get<uint8_t>(n, oom)) || !(d_alive = sc.get<uint8_t>(n, oom)) ||
        !(d_mirror = sc.get<uint32_t>(n, oom)) || !(d_succ = sc.get<uint32_t>(n, oom)) || !cb.get(sc, n)) {
        (void)hipGetLastError();
        return 1;
    }
    h_rec.resize(rec_words); h_circ.resize(n);
    {
        uint64_t *F = h_rec.data(), *len = F + (size_t)W * n, *kc = len + n;
        for (size_t r = 0; r < n; r++) {
            const UnitigRec &R = recs[r];
            for (int w = 0; w < W; w++) F[(size_t)w * n + r] = R.first[w];
            len[r] = R.len; kc[r] = R.kc; h_circ[r] = R.circ ? 1 : 0;
        }
    }
    UGCHK(hipMemcpyAsync(d_rec, h_rec.data(), rec_words * 8, hipMemcpyHostToDevice, st));
    UGCHK(hipMemcpyAsync(d_circ, h_circ.data(), n, hipMemcpyHostToDevice, st));
    UGCHK(hipMemcpyAsync(d_alive, alive.data(), n, hipMemcpyHostToDevice, st));
    UGCHK(hipMemcpyAsync(d_mirror, mirror.data(), n * 4, hipMemcpyHostToDevice, st));
    UGCHK(hipMemcpyAsync(d_succ, succ.data(), n * 4, hipMemcpyHostToDevice, st));
    UChainIn in;
    in.F = d_rec; in.len = in.F + (size_t)W * n; in.kc = in.len + n;
    in.circ = d_circ; in.alive = d_alive;
    in.mirror = d_mirror; in.succ = d_succ;
    in.n = (uint32_t)n; in.k = k;
    return chains_walk_t<W>(in, recs, cb, st, out, err);
}

// the device of the call, for its length
struct OnDevice {
    int before = 0, device; bool ok;
    explicit OnDevice(int d) : device(d) { ok = hipGetDevice(&before) == hipSuccess && (before == device || hipSetDevice(device) == hipSuccess); }
    ~OnDevice() { if (ok && before != device) (void)hipSetDevice(before); }
};

}  // namespace

int unitig_chains_device(int k, const std::vector<UnitigRec> &recs, const std::vector<uint8_t> &alive, const std::vector<uint32_t> &mirror,
                         const std::vector<uint32_t> &succ, int device, void *stream, UnitigGraphResult &out, std::string &err) {
    OnDevice on(device);
    if (!on.ok) { err = std::string("unitig graph on the device: no such device: ") + hipGetErrorString(hipGetLastError()); return -5; }
    hipStream_t st = (hipStream_t)stream;
    switch ((2 * k + 63) / 64) {
        case 1: return chains_device_t<1>(k, recs, alive, mirror, succ, st, out, err);
        case 2: return chains_device_t<2>(k, recs, alive, mirror, succ, st, out, err);
        case 3: return chains_device_t<3>(k, recs, alive, mirror, succ, st, out, err);
        case 4: return chains_device_t<4>(k, recs, alive, mirror, succ, st, out, err);
        case 5: return chains_device_t<5>(k, recs, alive, mirror, succ, st, out, err);
        case 6: return chains_device_t<6>(k, recs, alive, mirror, succ, st, out, err);
        case 7: return chains_device_t<7>(k, recs, alive, mirror, succ, st, out, err);
        case 8: return chains_device_t<8>(k, recs, alive, mirror, succ, st, out, err);
    }
    err = "k too large"; return -1;
}

int unitig_assemble_device(int k, const std::vector<UnitigRec> &recs, bool tips, bool bubbles, int device, void *stream,
                           UnitigGraphResult &out, std::string &err) {
    int before = 0;
    if (hipGetDevice(&before) != hipSuccess || (before != device && hipSetDevice(device) != hipSuccess)) {
        err = std::string("unitig graph on the device: no such device: ") + hipGetErrorString(hipGetLastError());
        return -5;
    }
    hipStream_t st = (hipStream_t)stream;
    int rc;
    switch ((2 * k + 63) / 64) {
        case 1: rc = assemble_device_t<1>(k, recs, tips, bubbles, st, out, err); break;
        case 2: rc = assemble_device_t<2>(k, recs, tips, bubbles, st, out, err); break;
        case 3: rc = assemble_device_t<3>(k, recs, tips, bubbles, st, out, err); break;
        case 4: rc = assemble_device_t<4>(k, recs, tips, bubbles, st, out, err); break;
        case 5: rc = assemble_device_t<5>(k, recs, tips, bubbles, st, out, err); break;
        case 6: rc = assemble_device_t<6>(k, recs, tips, bubbles, st, out, err); break;
        case 7: rc = assemble_device_t<7>(k, recs, tips, bubbles, st, out, err); break;
        case 8: rc = assemble_device_t<8>(k, recs, tips, bubbles, st, out, err); break;
        default: err = "k too large"; rc = -1;
    }
    if (before != device) (void)hipSetDevice(before);
    return rc;
}

}  // namespace shk
