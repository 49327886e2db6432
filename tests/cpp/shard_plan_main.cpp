// The host planning of the sharded assembly (csrc/shard_plan.h) on cases made by hand: no GPU, no HIP, a few records each.
// Built with -fsanitize=address,undefined by tests/test_shard_plan_host.py; prints "ok" and returns 0, or names the line
// that failed.
#include <stdio.h>
#include <atomic>
#include <string>
#include <vector>

#include "shard_plan.h"

using namespace shk;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond)                                                                       \
    do {                                                                                  \
        g_checks++;                                                                       \
        if (!(cond)) { g_failed++; fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

static UHead head(uint32_t root, uint32_t tail, uint32_t circ = 0, unsigned long long len = 1, unsigned long long kc = 1) {
    UHead h; h.root = root; h.tail = tail; h.circ = circ; h.pad = 0; h.len = len; h.kc = kc;
    return h;
}
template <class T> static bool same(const std::vector<T> &a, std::initializer_list<T> b) { return a == std::vector<T>(b); }

static void test_order() {
    std::vector<uint32_t> order, uid_of_slot;
    std::vector<UHead> uh = {head(4, 4), head(0, 1), head(3, 3)};
    CHECK(plan_order(uh, 6, order, uid_of_slot) == 0);
    CHECK(same<uint32_t>(order, {1, 2, 0}));                  // by first chain: 0, 3, 4
    CHECK(same<uint32_t>(uid_of_slot, {2, 0, 1}));            // its inverse
    for (uint32_t u = 0; u < 3; u++) CHECK(uid_of_slot[order[u]] == u);
    uh = {head(4, 4), head(0, 1), head(4, 5)};                // a root seen twice
    CHECK(plan_order(uh, 6, order, uid_of_slot) == -6);
    uh = {head(6, 6)};                                        // root == M: no such chain
    CHECK(plan_order(uh, 6, order, uid_of_slot) == -6);
    uh = {head(5, 5)};                                        // (the last chain is one)
    CHECK(plan_order(uh, 6, order, uid_of_slot) == 0 && same<uint32_t>(order, {0}));
    uh.clear();
    CHECK(plan_order(uh, 6, order, uid_of_slot) == 0 && order.empty() && uid_of_slot.empty());
    CHECK(plan_order(uh, 0, order, uid_of_slot) == 0 && order.empty() && uid_of_slot.empty());
}

static bool req_is(const EndReq &q, uint32_t uid, uint32_t which, uint32_t chain) { return q.uid == uid && q.which == which && q.chain == chain && q.pad == 0; }

static void test_end_requests() {
    // six chains, lbase = {0, 2, 6}: rank 0 holds chains 0 and 1, rank 1 chains 2 .. 5
    const std::vector<uint64_t> lbase = {0, 2, 6};
    // unitig 0: chains 0 -> 3 (root and tail on different ranks); 1: chain 1 alone; 2: chain 2 alone; 3: chains 4 -> 5
    const std::vector<UHead> uh = {head(4, 5), head(0, 3), head(2, 2), head(1, 1)};
    std::vector<uint32_t> order, uid_of_slot;
    CHECK(plan_order(uh, 6, order, uid_of_slot) == 0 && same<uint32_t>(order, {1, 3, 2, 0}));
    std::vector<EndReq> r0, r1;
    plan_end_requests(uh, order, lbase[0], lbase[1], 2, r0);
    plan_end_requests(uh, order, lbase[1], lbase[2], 2, r1);
    CHECK(r0.size() == 3);
    if (r0.size() == 3) {
        CHECK(req_is(r0[0], 0, 0, 0));                         // unitig 0: its first chain only
        CHECK(req_is(r0[1], 1, 0, 1) && req_is(r0[2], 1, 1, 1));      // one chain: root == tail, both ends, first before last
    }
    CHECK(r1.size() == 5);
    if (r1.size() == 5) {
        CHECK(req_is(r1[0], 0, 1, 1));                         // unitig 0's tail: chain 3 is this rank's second
        CHECK(req_is(r1[1], 2, 0, 0) && req_is(r1[2], 2, 1, 0));
        CHECK(req_is(r1[3], 3, 0, 2) && req_is(r1[4], 3, 1, 3));
    }
    int seen[4][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
    for (const auto *r : {&r0, &r1}) for (const EndReq &q : *r) { CHECK(q.uid < 4 && q.which < 2); if (q.uid < 4 && q.which < 2) seen[q.uid][q.which]++; }
    for (int u = 0; u < 4; u++) CHECK(seen[u][0] == 1 && seen[u][1] == 1);      // every (unitig, end) exactly once
    // one rank: everything
    plan_end_requests(uh, order, 0, 6, 1, r0);
    CHECK(r0.size() == 8 && req_is(r0[0], 0, 0, 0) && req_is(r0[1], 0, 1, 3) && req_is(r0[7], 3, 1, 5));
    // a call that finds requests from before
    plan_end_requests({}, {}, 0, 6, 1, r0);
    CHECK(r0.empty());
}

template <int W> static void test_records() {
    const std::vector<UHead> uh = {head(2, 2, 1, 70, 700), head(0, 1, 0, 50, 500), head(1, 0, 0, 60, 600)};
    std::vector<uint32_t> order, uid_of_slot;
    CHECK(plan_order(uh, 3, order, uid_of_slot) == 0 && same<uint32_t>(order, {1, 2, 0}));
    std::vector<uint64_t> ends((size_t)3 * 2 * W + 1);
    for (size_t j = 0; j < ends.size(); j++) ends[j] = 1000 + j;
    std::vector<UnitigRec> recs(7);                           // (what was there goes)
    plan_records<W>(uh, order, ends, recs);
    CHECK(recs.size() == 3);
    for (size_t u = 0; u < recs.size(); u++) {
        for (int w = 0; w < 8; w++) {
            CHECK(recs[u].first[w] == (w < W ? 1000 + (u * 2 + 0) * W + w : 0));
            CHECK(recs[u].last[w] == (w < W ? 1000 + (u * 2 + 1) * W + w : 0));
        }
        const UHead &h = uh[order[u]];
        CHECK(recs[u].len == h.len && recs[u].kc == h.kc && recs[u].circ == h.circ);
    }
    CHECK(recs[0].len == 50 && recs[1].len == 60 && recs[2].len == 70 && recs[2].circ == 1 && recs[0].circ == 0);
}

static void test_ring_merge() {
    constexpr int W = 2;
    const uint32_t world = 3, n_rings = 6;
    std::vector<uint64_t> rep((size_t)world * n_rings * (W + 2), ~0ull);       // nobody reports anything
    auto put = [&](uint32_t rank, uint32_t ring, uint64_t w0, uint64_t w1, uint64_t o, uint64_t pos) {
        uint64_t *p = &rep[((size_t)rank * n_rings + ring) * (W + 2)];
        p[0] = w0; p[1] = w1; p[2] = o; p[3] = pos;
    };
    put(1, 0, 11, 12, 1, 100);                                                 // ring 0: one rank only
    /* ring 1: no rank */
    put(0, 2, 5, 9, 0, 200); put(1, 2, 5, 8, 0, 201);                          // ring 2: word W - 1 decides
    put(0, 3, 7, 3, 0, 300); put(1, 3, 0, 4, 0, 301); put(2, 3, 6, 3, 0, 302); // ring 3: word 0 decides among ranks 0 and 2; rank 1 loses by word 1
    put(0, 4, 1, 1, 1, 400); put(1, 4, 1, 1, 0, 401);                          // ring 4: equal keys, the orientation decides
    put(0, 5, 2, 2, 1, 500); put(1, 5, 2, 2, 1, 501); put(2, 5, 2, 2, 1, 502); // ring 5: a full tie
    const std::vector<uint32_t> need_min = {3, 0, 5, 1, 4, 2};                 // ring i is record need_min[i]
    std::vector<UnitigMinKey> mk(7);
    plan_ring_min_keys<W>(rep, world, need_min, mk);
    auto is = [&](uint32_t rec, uint64_t w0, uint64_t w1, uint32_t o, uint64_t pos) {
        const UnitigMinKey &m = mk[rec];
        return m.valid && m.key[0] == w0 && m.key[1] == w1 && m.o == o && m.pos == pos;
    };
    CHECK(is(3, 11, 12, 1, 100));
    CHECK(!mk[0].valid);                                                       // ring 1
    CHECK(is(5, 5, 8, 0, 201));
    CHECK(is(1, 6, 3, 0, 302));
    CHECK(is(4, 1, 1, 0, 401));
    CHECK(is(2, 2, 2, 1, 500));                                                // the lower rank stays
    CHECK(!mk[6].valid);                                                       // a record that is no ring
    // the same tie with the ranks' reports swapped around: still the lowest rank that reports
    put(0, 5, ~0ull, ~0ull, ~0ull, ~0ull);
    plan_ring_min_keys<W>(rep, world, need_min, mk);
    CHECK(is(2, 2, 2, 1, 501));
}

// k = 5.  Eight records of 3, 2, 4, 1, 5, 2, 7, 6 nodes.  Contig A = records {0, 1}, B = {2, 3, 4}, the ring R = {5, 7}
// spelled from node 3 on; record 6 belongs to no contig.  Text: A 5 + 4 = 9 bytes at 0, B 10 + 4 = 14 at 9, R 8 + 4 = 12 at 23.
static const int K = 5;
static std::vector<UnitigRec> layout_recs() {
    std::vector<UnitigRec> recs(8);
    const uint64_t len[8] = {3, 2, 4, 1, 5, 2, 7, 6};
    for (int r = 0; r < 8; r++) recs[r].len = len[r];
    return recs;
}
static UnitigContig contig(std::initializer_list<uint32_t> recs, uint64_t len_nodes, uint64_t kc, bool ring = false, uint64_t rot = 0) {
    UnitigContig c; c.recs = recs; c.len_nodes = len_nodes; c.kc = kc; c.ring = ring; c.rot = rot;
    return c;
}
static UnitigGraphResult result_not_flat() {
    UnitigGraphResult res;
    res.contigs = {contig({0, 1}, 5, 50), contig({2, 3, 4}, 10, 100), contig({5, 7}, 8, 80, true, 3)};
    return res;
}
static UnitigGraphResult result_flat() {
    UnitigGraphResult res;
    res.flat = true;
    res.lin = {UnitigFlatContig{5, 50, 0, 0, 0, 2}, UnitigFlatContig{10, 100, 9, 2, 2, 3}};
    res.recs_flat = {0, 1, 2, 3, 4};
    res.place = {{0, 0}, {0, 3}, {9, 0}, {9, 4}, {9, 5}, {~0ull, 0}, {~0ull, 0}, {~0ull, 0}};
    res.lin_text = 23;
    res.contigs = {contig({5, 7}, 8, 80, true, 3)};
    return res;
}
static bool lay_is(const ULayout &l, uint64_t off, uint64_t node_off, uint64_t ring_len, uint64_t rot) {
    return l.off == off && l.node_off == node_off && l.ring_len == ring_len && l.rot == rot;
}
static void check_layout(const ContigLayout &L, size_t n_lin) {
    CHECK(L.n_lin == n_lin && L.n_contigs == 3);
    CHECK(same<uint64_t>(L.c_off, {0, 9, 23}));
    CHECK(L.text_bytes == (5 + 4) + (10 + 4) + (8 + 4));
    CHECK(L.lay.size() == 9);
    if (L.lay.size() != 9) return;
    CHECK(lay_is(L.lay[0], 0, 0, 0, 0) && lay_is(L.lay[1], 0, 3, 0, 0));
    CHECK(lay_is(L.lay[2], 9, 0, 0, 0) && lay_is(L.lay[3], 9, 4, 0, 0) && lay_is(L.lay[4], 9, 5, 0, 0));
    CHECK(lay_is(L.lay[5], 23, 0, 8, 3) && lay_is(L.lay[7], 23, 2, 8, 3));
    CHECK(lay_is(L.lay[6], ~0ull, 0, 0, 0));                  // a record of no contig
    CHECK(lay_is(L.lay[8], ~0ull, 0, 0, 0));                  // the sentinel
}

static void test_layout() {
    const std::vector<UnitigRec> recs = layout_recs();
    ContigLayout L;
    CHECK(plan_layout(K, result_not_flat(), recs, L) == 0);
    check_layout(L, 0);
    CHECK(plan_layout(K, result_flat(), recs, L) == 0);       // (into the same object: nothing of the first call stays)
    check_layout(L, 2);
    UnitigGraphResult res = result_flat();
    res.place.pop_back();
    CHECK(plan_layout(K, res, recs, L) == -6);                // place.size() != n_u
    res = result_flat();
    res.place.push_back(UnitigPlace{~0ull, 0});
    CHECK(plan_layout(K, res, recs, L) == -6);
    res = result_flat();
    res.recs_flat.assign(9, 0);
    CHECK(plan_layout(K, res, recs, L) == -6);                // recs_flat.size() > n_u
    res.recs_flat.assign(8, 0);
    CHECK(plan_layout(K, res, recs, L) == 0);
    // no unitig at all
    CHECK(plan_layout(K, UnitigGraphResult(), std::vector<UnitigRec>(), L) == 0);
    CHECK(L.n_contigs == 0 && L.text_bytes == 0 && L.c_off.empty() && L.lay.size() == 1 && lay_is(L.lay[0], ~0ull, 0, 0, 0));
}

static void test_contig_lists() {
    const std::vector<UnitigRec> recs = layout_recs();
    const uint64_t nodes[3] = {5, 10, 8}, kc[3] = {50, 100, 80}, off[3] = {0, 9, 23};
    std::vector<RawContig> raw[2];
    for (int flat = 0; flat < 2; flat++) {
        const UnitigGraphResult res = flat ? result_flat() : result_not_flat();
        ContigLayout L;
        CHECK(plan_layout(K, res, recs, L) == 0);
        for (size_t i = 0; i < 3; i++) { const ContigSize c = plan_contig(res, L.n_lin, i); CHECK(c.len_nodes == nodes[i] && c.kc == kc[i]); }
        std::vector<WContig> hc(1);
        CHECK(plan_writer_contigs(K, res, L, hc) == 0);
        CHECK(hc.size() == 3);
        for (size_t i = 0; i < hc.size() && i < 3; i++) CHECK(hc[i].slot == i && hc[i].len == nodes[i] + K - 1 && hc[i].off == off[i] && hc[i].kc == kc[i]);
        static const char text[64] = {0};
        plan_raw_contigs(K, res, L, text, raw[flat]);
        CHECK(raw[flat].size() == 3);
        for (size_t i = 0; i < raw[flat].size() && i < 3; i++) {
            const RawContig &c = raw[flat][i];
            CHECK(c.ext == text + off[i] && c.ext_n == nodes[i] + K - 1 && c.kc == kc[i] && c.own.empty());
        }
        // not back to back: one byte between the first contig and the second
        ContigLayout L2 = L;
        L2.c_off[1] += 1;
        CHECK(plan_writer_contigs(K, res, L2, hc) == 2);
        L2 = L;
        L2.text_bytes += 1;                                   // ... or behind the last
        CHECK(plan_writer_contigs(K, res, L2, hc) == 2);
    }
    // 2^32 bases: one node more than fits 32 bits (the ring, which both forms keep in res.contigs)
    for (int flat = 0; flat < 2; flat++) {
        UnitigGraphResult res = flat ? result_flat() : result_not_flat();
        ContigLayout L;
        res.contigs.back().len_nodes = (1ull << 32) - (K - 1) - 1;                // 2^32 - 1 bases: fits
        CHECK(plan_layout(K, res, recs, L) == 0);
        std::vector<WContig> hc;
        CHECK(plan_writer_contigs(K, res, L, hc) == 0 && hc.back().len == 0xFFFFFFFFu);
        res.contigs.back().len_nodes += 1;                                        // 2^32 bases
        CHECK(plan_layout(K, res, recs, L) == 0);
        CHECK(plan_writer_contigs(K, res, L, hc) == 1);
    }
    {
        UnitigGraphResult res = result_flat();                                    // ... and a linear contig of the flat form
        ContigLayout L;
        res.lin[0].len_nodes = (1ull << 32) - (K - 1);
        CHECK(plan_layout(K, res, recs, L) == 0);
        std::vector<WContig> hc;
        CHECK(plan_writer_contigs(K, res, L, hc) == 1);
    }
}

// every index once: n = 262144 is the first size that uses threads
static void test_threads() {
    for (size_t n : {(size_t)262143, (size_t)262144}) {
        std::vector<uint8_t> hits(n, 0);
        std::atomic<int> calls{0};
        host_par_ranges(n, [&](size_t a, size_t b) { calls++; for (size_t i = a; i < b; i++) hits[i]++; });
        size_t wrong = 0;
        for (size_t i = 0; i < n; i++) wrong += hits[i] != 1;
        CHECK(wrong == 0);
        const unsigned hw = std::thread::hardware_concurrency();
        CHECK(calls.load() == (n < 262144 ? 1 : (int)std::min(16u, std::max(1u, hw))));
    }
    int calls = 0;
    host_par_ranges(0, [&](size_t a, size_t b) { calls++; CHECK(a == 0 && b == 0); });
    CHECK(calls == 1);
}

int main() {
    test_order();
    test_end_requests();
    test_records<1>();
    test_records<3>();
    test_ring_merge();
    test_layout();
    test_contig_lists();
    test_threads();
    if (g_failed) { fprintf(stderr, "%d of %d checks failed\n", g_failed, g_checks); return 1; }
    printf("ok: %d checks\n", g_checks);
    return 0;
}
