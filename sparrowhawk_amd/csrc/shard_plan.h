// shard_plan.h — the host planning of the sharded assembly (shard_graph.h, DESIGN.md "Multi-GPU"): plain arithmetic on the
// records that came home, between the device steps of Pipeline<W>::shard_assemble.  No HIP in here: a host compiler takes
// this header alone (tests/cpp/shard_plan_main.cpp runs it under AddressSanitizer and UBSan, by hand-made cases).
//
// Every function here sees the same input on every rank (the gathered chain records, the all-reduced end words, the
// all-gathered ring reports), so its verdict is every rank's: the caller sets sh_agreed_ beside each error.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

#include "kmer.h"
#include "pipeline.h"
#include "unitig_graph.h"

namespace shk {

// per unitig (a chain of local chains): reported by its last record — the tail of a linear one, the record in front of the
// smallest index of a ring (shard_graph.h: k_stitch_tails)
struct UHead { uint32_t root, tail, circ, pad; unsigned long long len, kc; };
// first / last k-mer of a unitig, asked of the rank that holds that chain (k_fill_ends)
struct EndReq { uint32_t uid, which /* 0 first, 1 last */, chain /* local chain */, pad; };
// where a unitig record's nodes go in the contig text (k_shard_emit)
struct ULayout { unsigned long long off /* byte offset of the contig text; ~0: not emitted */, node_off, ring_len /* 0: linear */, rot; };
// a contig of the text the device writer works on (writer_gpu.h)
struct WContig { unsigned long long off, kc; uint32_t len /* bases */, slot /* chain record */; };

// a loop over millions of host records (the unitigs of a metagenome) on several threads
template <typename F> void host_par_ranges(size_t n, F &&fn) {
    const unsigned hw = std::thread::hardware_concurrency();
    const unsigned T = n < 262144 ? 1u : std::min(16u, std::max(1u, hw));
    if (T == 1) { fn((size_t)0, n); return; }
    std::vector<std::thread> ts;
    for (unsigned t = 1; t < T; t++) ts.emplace_back([&fn, n, t, T] { fn(n * t / T, n * (t + 1) / T); });
    fn((size_t)0, n / T);
    for (auto &t : ts) t.join();
}

// The unitigs in the order of their first chain: order[u] = index into uheads, uid_of_slot its inverse.
// (the first chains are distinct numbers below M: a table instead of a sort — a metagenome has millions of unitigs)
// -6: two unitigs with one first chain (a root that is no chain, or seen twice).
inline int plan_order(const std::vector<UHead> &uheads, uint64_t M, std::vector<uint32_t> &order, std::vector<uint32_t> &uid_of_slot) {
    const uint32_t n_u = (uint32_t)uheads.size();
    order.assign(n_u, 0);
    {
        std::vector<uint32_t> slot_at((size_t)M + 1, 0xFFFFFFFFu);
        for (uint32_t i = 0; i < n_u; i++) {
            if (uheads[i].root >= M || slot_at[uheads[i].root] != 0xFFFFFFFFu) return -6;
            slot_at[uheads[i].root] = i;
        }
        uint32_t at = 0;
        for (uint32_t c0 = 0; c0 < M; c0++) if (slot_at[c0] != 0xFFFFFFFFu) order[at++] = slot_at[c0];
    }
    uid_of_slot.assign(n_u, 0);
    for (uint32_t u = 0; u < n_u; u++) uid_of_slot[order[u]] = u;
    return 0;
}

// The ends this rank holds — its chains are [lo, hi) of the gathered list: ascending unitig, first before last.
inline void plan_end_requests(const std::vector<UHead> &uheads, const std::vector<uint32_t> &order, uint64_t lo, uint64_t hi, uint32_t world,
                              std::vector<EndReq> &reqs) {
    const uint32_t n_u = (uint32_t)order.size();
    reqs.clear();
    reqs.reserve(world == 1 ? 2 * (size_t)n_u : 2 * (size_t)n_u / world + 1024);
    for (uint32_t u = 0; u < n_u; u++) {
        const UHead &h = uheads[order[u]];
        if (h.root >= lo && h.root < hi) reqs.push_back(EndReq{u, 0u, (uint32_t)(h.root - lo), 0u});
        if (h.tail >= lo && h.tail < hi) reqs.push_back(EndReq{u, 1u, (uint32_t)(h.tail - lo), 0u});
    }
}

// recs[u] from uheads[order[u]] and the all-reduced end words, ends[(u * 2 + which) * W + w]
template <int W>
void plan_records(const std::vector<UHead> &uheads, const std::vector<uint32_t> &order, const std::vector<uint64_t> &ends, std::vector<UnitigRec> &recs) {
    const size_t n_u = order.size();
    recs.assign(n_u, UnitigRec());
    host_par_ranges(n_u, [&](size_t a, size_t b) {
        for (size_t u = a; u < b; u++) {
            const UHead &h = uheads[order[u]];
            for (int w = 0; w < W; w++) { recs[u].first[w] = ends[(u * 2 + 0) * W + w]; recs[u].last[w] = ends[(u * 2 + 1) * W + w]; }
            recs[u].len = h.len; recs[u].kc = h.kc; recs[u].circ = h.circ;
        }
    });
}

// Rings: what the ranks offer per ring (all_rep: world x n_rings x {W key words, orientation, position}; all ones in word
// W: none) -> mk[need_min[i]] = the smallest.  Keys compare from word W - 1 down, then the orientation; on a full tie the
// lower rank stays.  A ring that no rank reports stays !valid.
template <int W>
void plan_ring_min_keys(const std::vector<uint64_t> &all_rep, uint32_t world, const std::vector<uint32_t> &need_min, std::vector<UnitigMinKey> &mk) {
    const uint32_t n_rings = (uint32_t)need_min.size();
    for (uint32_t i = 0; i < n_rings; i++) {
        UnitigMinKey best;
        for (uint32_t r = 0; r < world; r++) {
            const uint64_t *o = &all_rep[((size_t)r * n_rings + i) * (W + 2)];
            if (o[W] == ~0ull) continue;
            UnitigMinKey cand; cand.valid = true; cand.o = (uint32_t)o[W]; cand.pos = o[W + 1];
            for (int w = 0; w < W; w++) cand.key[w] = o[w];
            bool less = !best.valid;
            if (!less) {
                bool decided = false;
                for (int w = W - 1; w >= 0 && !decided; w--) if (cand.key[w] != best.key[w]) { less = cand.key[w] < best.key[w]; decided = true; }
                if (!decided) less = cand.o < best.o;
            }
            if (less) best = cand;
        }
        mk[need_min[i]] = best;
    }
}

// The layout: contig text offsets, and for every unitig record where its nodes go (lay[n_u] is a sentinel: not emitted).
// (the walk on the device hands over the linear contigs flat, with every record's placement: the linear contigs come
// first, the rings — res.contigs — behind them, their text from the linear contigs' total on)
struct ContigLayout {
    std::vector<ULayout> lay;            // n_u + 1
    std::vector<uint64_t> c_off;         // per contig: its text offset
    uint64_t text_bytes = 0;
    size_t n_lin = 0, n_contigs = 0;     // the flat linear contigs in front; all contigs
};
// -6: the flat form of the unitig graph does not fit the records.
inline int plan_layout(int k, const UnitigGraphResult &res, const std::vector<UnitigRec> &recs, ContigLayout &L) {
    const size_t n_u = recs.size();
    L.n_lin = res.flat ? res.lin.size() : 0; L.n_contigs = L.n_lin + res.contigs.size();
    if (res.flat && (res.place.size() != n_u || res.recs_flat.size() > n_u)) return -6;
    std::vector<ULayout> &lay = L.lay;
    lay.assign(n_u + 1, ULayout());
    L.text_bytes = 0;
    L.c_off.assign(L.n_contigs, 0);
    if (res.flat) {
        host_par_ranges(n_u, [&](size_t a, size_t b) {
            for (size_t r = a; r < b; r++) { ULayout &l = lay[r]; l.off = res.place[r].off; l.node_off = res.place[r].node_off; l.ring_len = 0; l.rot = 0; }
        });
        { ULayout &l = lay[n_u]; l.off = ~0ull; l.node_off = 0; l.ring_len = 0; l.rot = 0; }
        host_par_ranges(L.n_lin, [&](size_t a, size_t b) { for (size_t i = a; i < b; i++) L.c_off[i] = res.lin[i].text_off; });
        L.text_bytes = res.lin_text;
    } else
        for (auto &l : lay) { l.off = ~0ull; l.node_off = 0; l.ring_len = 0; l.rot = 0; }
    for (size_t i = 0; i < res.contigs.size(); i++) {
        const UnitigContig &ct = res.contigs[i];
        L.c_off[L.n_lin + i] = L.text_bytes;
        uint64_t node_off = 0;
        for (uint32_t r : ct.recs) {
            lay[r].off = L.text_bytes; lay[r].node_off = node_off; lay[r].ring_len = ct.ring ? ct.len_nodes : 0; lay[r].rot = ct.ring ? ct.rot : 0;
            node_off += recs[r].len;
        }
        L.text_bytes += ct.len_nodes + (uint64_t)(k - 1);
    }
    return 0;
}

// contig i of the result, in text order: the flat linear ones, then res.contigs
struct ContigSize { uint64_t len_nodes, kc; };
inline ContigSize plan_contig(const UnitigGraphResult &res, size_t n_lin, size_t i) {
    if (i < n_lin) return ContigSize{res.lin[i].len_nodes, res.lin[i].kc};
    return ContigSize{res.contigs[i - n_lin].len_nodes, res.contigs[i - n_lin].kc};
}
// The contigs for the device writer (24 bytes each to upload).  0, or why the writer declines: 1 — a contig of 2^32 bases
// or more, 2 — the contigs do not lie back to back in the text.
inline int plan_writer_contigs(int k, const UnitigGraphResult &res, const ContigLayout &L, std::vector<WContig> &hc) {
    const size_t n_contigs = L.n_contigs;
    hc.assign(n_contigs, WContig());
    std::atomic<int> bad{0};
    host_par_ranges(n_contigs, [&](size_t a, size_t b) {
        for (size_t i = a; i < b; i++) {
            const ContigSize ct = plan_contig(res, L.n_lin, i);
            const uint64_t bases = ct.len_nodes + (uint64_t)(k - 1);
            if (bases > 0xFFFFFFFFull) bad.store(1);
            else if (L.c_off[i] + bases != (i + 1 < n_contigs ? L.c_off[i + 1] : L.text_bytes)) bad.store(2);
            hc[i].off = L.c_off[i]; hc[i].kc = ct.kc; hc[i].len = (uint32_t)bases; hc[i].slot = (uint32_t)i;
        }
    });
    return bad.load();
}
// The contigs for the host writer: their text lies at text + c_off[i].
inline void plan_raw_contigs(int k, const UnitigGraphResult &res, const ContigLayout &L, const char *text, std::vector<RawContig> &out) {
    out.resize(L.n_contigs);
    host_par_ranges(L.n_contigs, [&](size_t a, size_t b) {
        for (size_t i = a; i < b; i++) {
            const ContigSize ct = plan_contig(res, L.n_lin, i);
            RawContig &rcg = out[i]; rcg.kc = ct.kc;
            rcg.ext = text + L.c_off[i]; rcg.ext_n = ct.len_nodes + (uint64_t)(k - 1);
        }
    });
}

}  // namespace shk
