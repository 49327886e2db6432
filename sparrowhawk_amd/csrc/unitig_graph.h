// unitig_graph.h — SPEC S9 (tips, bubbles) and S10 (maximal chains of simple links) on the graph of UNITIGS instead of
// the graph of k-mers.  Used by the sharded assembly (DESIGN.md "Multi-GPU"): the k-mer-level work — adjacency, the
// contraction of non-branching paths into unitigs — is spread over the ranks on their GPUs; what is left is a graph
// with one vertex per unitig (a handful for an isolate), small enough to be corrected identically on every rank's
// host.  Replaces, for that path, the phases `assembly:correct_graph` and the top level of `assembly:collapse_graph`
// (/root/reference/www/src/components/pages/AssemblyPage.vue:598-602).
//
// Why this is exact.  A unitig is a maximal chain of SIMPLE links (S10); every other edge of the k-mer graph leaves
// the LAST node of a chain and enters the FIRST node of a chain (a node with a simple successor has no other
// out-edge, one with a simple predecessor no other in-edge).  So the whole graph is: chains, plus overlaps between
// chain ends — and those follow from the first and last k-mer of every chain alone.  The walks of S9 stop or go on
// by out-/in-degrees, which inside a chain are 1/1 by construction, and count nodes, which a chain contributes as
// its length; removals take whole chains (a tip starts at a node without predecessor and ends before a junction; a
// bubble branch starts behind a fork and ends before a junction).  Run on chain records the rules are the same rules.
#pragma once
#include <stdint.h>
#include <string>
#include <vector>

#include "kmer.h"

namespace shk {

static constexpr uint32_t UG_NIL = 0xFFFFFFFFu;

// The k-mer arithmetic of the index of chain starts, shared by the host code (unitig_graph.cpp) and its device twin
// (unitig_graph_gpu.hip): the first k-1 bases of a k-mer as a 2(k-1)-bit integer, the last k-1 bases, and the placement hash.
template <int W> SHK_HD Kmer<W> ug_prefix(const Kmer<W> &x) {
    Kmer<W> r;
#pragma unroll
    for (int i = 0; i < W; i++) r.w[i] = (x.w[i] >> 2) | (i + 1 < W ? x.w[i + 1] << 62 : 0ull);
    return r;
}
template <int W> SHK_HD Kmer<W> ug_suffix(const Kmer<W> &x, int k) {
    Kmer<W> r = x;
    const int bits = 2 * (k - 1);
#pragma unroll
    for (int i = 0; i < W; i++) {
        const int lo = 64 * i;
        if (bits <= lo) r.w[i] = 0;
        else if (bits < lo + 64) r.w[i] &= (1ull << (bits - lo)) - 1ull;
    }
    return r;
}
SHK_HD uint64_t ug_mix(uint64_t x) { x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31; return x; }
template <int W> SHK_HD uint64_t ug_hash_of(const Kmer<W> &p) {
    uint64_t h = 0x9E3779B97F4A7C15ull;
#pragma unroll
    for (int i = 0; i < W; i++) h = ug_mix(h ^ p.w[i]);
    return h;
}

// One STRAND of a unitig: the chain v_1 -> ... -> v_n as it is spelled.  Its mirror strand rc(v_n) -> ... -> rc(v_1) is
// a record of its own (first = revcomp(last of this one)).  K-mers: 2k-bit integers, first base most significant, in
// W = ceil(2k/64) words, w[0] least significant (kmer.h), spelled in the orientation of the strand.
struct UnitigRec {
    uint64_t first[8] = {0, 0, 0, 0, 0, 0, 0, 0}, last[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t len = 0;            // nodes
    uint64_t kc = 0;             // sum of their counts
    uint32_t circ = 0;           // the chain closes on itself: no ends, no edges to anything else
};
// the smallest oriented node key(x, o) = (canonical k-mer, orientation) among the nodes of a record, and where it sits
struct UnitigMinKey {
    uint64_t key[8] = {~0ull, ~0ull, ~0ull, ~0ull, ~0ull, ~0ull, ~0ull, ~0ull};
    uint32_t o = 1;
    uint64_t pos = 0;            // its position in the record's chain (0 = first node)
    bool valid = false;
};
struct UnitigContig {
    std::vector<uint32_t> recs;  // strand records in the order they are spelled
    bool ring = false;
    uint64_t rot = 0;            // rings: the spelling starts at node `rot` of the concatenation (S10: before the smallest k-mer)
    uint64_t len_nodes = 0, kc = 0;
};

// The flat form of the linear contigs, as the device walk (unitig_graph_gpu.h) hands them over: no vector per contig.
// Contig c spells the records recs_flat[rec_off .. rec_off + n_recs); contigs ascend by their head's record number,
// which is the order unitig_chains appends them in.
struct UnitigFlatContig {
    uint64_t len_nodes, kc;
    uint64_t text_off;           // sum of len_nodes + k - 1 over the linear contigs in front
    uint64_t rec_off;            // into recs_flat
    uint32_t head, n_recs;
};
// where a record's nodes go: off — the text offset of its contig, ~0 for a record of no linear contig that is handed on
// (dead, ring, the dropped mirror strand); node_off — the nodes of the contig's records in front of it
struct UnitigPlace { uint64_t off, node_off; };
struct UnitigRingRec { uint32_t r, succ, mirror; };   // an alive record on no linear chain, with its links

struct UnitigGraphResult {
    // every contig once, on one strand (the writer picks min(seq, revcomp) later); with `flat`: the rings only, which
    // follow the linear contigs
    std::vector<UnitigContig> contigs;
    bool flat = false;                      // the walk ran on the device: the linear contigs are in the three vectors below
    std::vector<UnitigFlatContig> lin;
    std::vector<uint32_t> recs_flat;
    std::vector<UnitigPlace> place;         // per record
    uint64_t lin_text = 0;                  // sum of len_nodes + k - 1 over lin: where the rings' text starts
    std::vector<uint32_t> mirror;           // per record: its mirror strand's record, UG_NIL for rings / none (with `flat`: known at
                                            // the records of rings of several records only; empty when there is no such ring)
    // rings are only settled once the smallest k-mer of their records is known: resolve_rings()
    std::vector<uint32_t> need_min;         // records whose UnitigMinKey resolve_rings() wants
    uint64_t tips_removed = 0, bubbles_removed = 0;   // nodes (as the k-mer-level passes count them)
    int rounds = 0;
};

// S9 rounds on the records (tips unless !tips, bubbles unless !bubbles), then S10 chains over what is left.
// Returns 0, or -1 with err (inconsistent input: a linear record without its mirror strand).
int unitig_assemble(int k, const std::vector<UnitigRec> &recs, bool tips, bool bubbles, UnitigGraphResult &out, std::string &err);
// The S10 walk alone, from arrays that are already settled (by unitig_assemble itself, or by its device twin,
// unitig_graph_gpu.h): alive[r], mirror[r] (UG_NIL for rings) and succ[r], the simple successor of an alive linear
// record (UG_NIL: none).  Looks nothing up: heads, the strand with the smaller first k-mer, rings of several records,
// rings from the start.  Appends to out.contigs / out.need_min and sets out.mirror.
int unitig_chains(int k, const std::vector<UnitigRec> &recs, const std::vector<uint8_t> &alive, std::vector<uint32_t> &&mirror,
                  const std::vector<uint32_t> &succ, UnitigGraphResult &out, std::string &err);
// What unitig_chains and its device twin take for granted, checked: -1 with err = "unitig chains: <what>" unless succ is
// UG_NIL or an alive linear record, no two records share a successor, mirror pairs up among the alive linear records,
// mirror[succ[r]] has mirror[r] as its successor, and dead and circ records carry succ == UG_NIL.
int unitig_chains_check(const std::vector<UnitigRec> &recs, const std::vector<uint8_t> &alive, const std::vector<uint32_t> &mirror,
                        const std::vector<uint32_t> &succ, std::string &err);
// The two ring loops of unitig_chains over the ring records alone (in any order; sorted here): the alive linear records
// that reach no head, and the alive circ records.  Appends to out.contigs / out.need_min; sets out.mirror (n_recs
// entries, UG_NIL but at the ring records) when there is a ring of linear records.
int unitig_ring_chains(const std::vector<UnitigRec> &recs, std::vector<UnitigRingRec> &&rings, UnitigGraphResult &out, std::string &err);
// min_of[r] must be valid for every r in out.need_min.  Touches out.contigs only: the flat form holds no ring.  Fixes strand and rotation of the ring contigs, drops the
// mirror-strand duplicates of rings that were rings from the start.
int unitig_resolve_rings(int k, const std::vector<UnitigRec> &recs, const std::vector<UnitigMinKey> &min_of, UnitigGraphResult &out,
                         std::string &err);

}  // namespace shk
