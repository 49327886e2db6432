// exchange_plan.h — the host planning of the sharded preprocess (shard_preprocess.cpp, DESIGN.md "Multi-GPU"): plain arithmetic
// on the words the ranks exchange, between the device steps.  No HIP in here: a host compiler takes this header alone
// (tests/cpp/exchange_plan_main.cpp runs it under AddressSanitizer and UBSan, by hand-made cases; tests/test_dist.py compares
// plan_exchange and choose_partitions with sparrowhawk_amd/dist.py through the library).
//
// Every function below the plan sees the same input on every rank (the gathered size rows, the all-reduced histogram words,
// the gathered row counts), so its verdict is every rank's.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string>
#include <vector>

namespace shk {

// power of two in [64, 16384], >= world, ~per_part k-mer instances per partition
inline uint32_t choose_partitions(uint64_t total_instances_ub, uint32_t world, uint64_t per_part) {
    uint32_t P = 64;
    while (P < 16384u && (uint64_t)P * per_part < total_instances_ub) P <<= 1;
    while (P < world) P <<= 1;
    return P;
}

// part_records_all: [world][P] records rank s holds for partition p; partition p belongs to rank p % world.
struct ExchangePlan {
    std::vector<uint32_t> owned;          // partitions this rank counts, ascending
    std::vector<uint64_t> base;           // [P] record offset of partition p in the send buffer (destination-major)
    std::vector<uint64_t> send_counts;    // [world] records sent to each destination
    std::vector<uint64_t> recv_counts;    // [world] records received from each source
    std::vector<uint64_t> run_off;        // [n_owned][world] record offset of source s's run of owned partition j in the receive buffer
    std::vector<uint32_t> run_cnt;        // [n_owned][world]
};
inline int plan_exchange(const uint64_t *pr, uint32_t world, uint32_t P, uint32_t rank, ExchangePlan &out, std::string &err) {
    if (!pr || world < 1 || rank >= world || P < world) { err = "plan_exchange: bad arguments"; return -1; }
    const uint64_t *mine = pr + (uint64_t)rank * P;
    out.base.assign(P, 0); out.send_counts.assign(world, 0); out.recv_counts.assign(world, 0);
    uint64_t off = 0;
    for (uint32_t d = 0; d < world; d++)                       // destination-major, partitions ascending
        for (uint32_t p = d; p < P; p += world) { out.base[p] = off; off += mine[p]; out.send_counts[d] += mine[p]; }
    out.owned.clear();
    for (uint32_t p = rank; p < P; p += world) out.owned.push_back(p);
    const uint32_t n_owned = (uint32_t)out.owned.size();
    std::vector<uint64_t> recv_base(world, 0);
    for (uint32_t s = 0; s < world; s++) {
        uint64_t t = 0;
        for (uint32_t j = 0; j < n_owned; j++) t += pr[(uint64_t)s * P + out.owned[j]];
        out.recv_counts[s] = t;
    }
    for (uint32_t s = 1; s < world; s++) recv_base[s] = recv_base[s - 1] + out.recv_counts[s - 1];
    out.run_off.assign((uint64_t)n_owned * world, 0); out.run_cnt.assign((uint64_t)n_owned * world, 0);
    for (uint32_t s = 0; s < world; s++) {
        uint64_t within = 0;                                   // source s sends its partitions for this rank in ascending order
        for (uint32_t j = 0; j < n_owned; j++) {
            const uint64_t c = pr[(uint64_t)s * P + out.owned[j]];
            if (c > 0xFFFFFFFFull) { err = "plan_exchange: more than 2^32 records of one partition on one rank"; return -1; }
            out.run_off[(uint64_t)j * world + s] = recv_base[s] + within;
            out.run_cnt[(uint64_t)j * world + s] = (uint32_t)c;
            within += c;
        }
    }
    return 0;
}

// ---- the size row: what a rank tells the others after pass 1, one row of the size all-gather
//   [0, P)   records to send per partition (the distinct ones where the rank deduplicated)
//   [P, 2P)  raw records per partition
//   then     this rank failed; the rank's dedupe mode
enum DedupeMode : uint64_t { DEDUPE_RAW = 0, DEDUPE_AUTO = 1, DEDUPE_ALWAYS = 2 };
inline size_t size_row_words(uint32_t P) { return 2 * (size_t)P + 2; }
inline std::vector<uint64_t> size_row_fill(uint32_t P, const uint64_t *send, const uint64_t *raw, bool failed, uint64_t mode) {
    std::vector<uint64_t> row(size_row_words(P), 0);
    for (uint32_t p = 0; p < P; p++) { row[p] = send[p]; row[(size_t)P + p] = raw[p]; }
    row[2 * (size_t)P] = failed ? 1u : 0u;
    row[2 * (size_t)P + 1] = mode;
    return row;
}
struct SizeRow { const uint64_t *send, *raw; bool failed; uint64_t mode; };      // (points into the gathered rows)
inline SizeRow size_row_read(const std::vector<uint64_t> &rows, uint32_t P, uint32_t r) {
    const uint64_t *row = &rows[(size_t)r * size_row_words(P)];
    return SizeRow{row, row + P, row[2 * (size_t)P] != 0, row[2 * (size_t)P + 1]};
}

// The verdict of the gathered rows: did a rank fail, and do the records travel deduplicated, with u32 weights?  One rank in
// raw mode makes it raw for all; else one rank in `always` makes it weighted; else it is weighted when the distinct records
// of all ranks are at most half of the raw ones.  counts: [world][P] what travels; raw_counts: [world][P].
struct DedupeVerdict {
    bool peer_failed = false, weighted = true;
    std::vector<uint64_t> counts, raw_counts;
};
inline DedupeVerdict dedupe_verdict(const std::vector<uint64_t> &rows, uint32_t world, uint32_t P) {
    DedupeVerdict v;
    bool forced = false;
    uint64_t sum_dd = 0, sum_raw = 0;
    for (uint32_t r = 0; r < world; r++) {
        const SizeRow row = size_row_read(rows, P, r);
        if (row.failed) v.peer_failed = true;
        if (row.mode == DEDUPE_RAW) v.weighted = false;
        if (row.mode == DEDUPE_ALWAYS) forced = true;
        for (uint32_t p = 0; p < P; p++) { sum_dd += row.send[p]; sum_raw += row.raw[p]; }
        v.raw_counts.insert(v.raw_counts.end(), row.raw, row.raw + P);
    }
    if (v.weighted && !forced && sum_dd * 2 > sum_raw) v.weighted = false;
    for (uint32_t r = 0; r < world; r++) {
        const SizeRow row = size_row_read(rows, P, r);
        const uint64_t *from = v.weighted ? row.send : row.raw;
        v.counts.insert(v.counts.end(), from, from + P);
    }
    return v;
}

// A partition's record index — and a record's multiplicity — are 32 bits wide in pass 2: where weights travel, the RAW records
// of every partition this rank owns, summed over the ranks, must stay within that (raw travel: plan_exchange's own limit holds).
static constexpr uint64_t RAW_RECORDS_MAX = 0xFFFFFFF0ull;
inline bool raw_records_fit(const DedupeVerdict &v, uint32_t world, uint32_t P, uint32_t rank) {
    if (!v.weighted) return true;
    for (uint32_t p = rank; p < P; p += world) {
        uint64_t t = 0;
        for (uint32_t r = 0; r < world; r++) t += v.raw_counts[(size_t)r * P + p];
        if (t > RAW_RECORDS_MAX) return false;
    }
    return true;
}

// The byte layout of one all-to-all of the plan: elements of elem_bytes (a record, then 4 for its weight), rank after rank.
struct ExchangeBytes {
    std::vector<uint64_t> send_off, send_bytes, recv_off, recv_bytes;      // [world]
    uint64_t n_send = 0, n_recv = 0;                                       // elements
};
inline ExchangeBytes exchange_bytes(const ExchangePlan &plan, uint64_t elem_bytes) {
    const size_t world = plan.send_counts.size();
    ExchangeBytes x;
    x.send_off.resize(world); x.send_bytes.resize(world); x.recv_off.resize(world); x.recv_bytes.resize(world);
    for (size_t r = 0; r < world; r++) {
        x.send_off[r] = x.n_send * elem_bytes; x.send_bytes[r] = plan.send_counts[r] * elem_bytes; x.n_send += plan.send_counts[r];
        x.recv_off[r] = x.n_recv * elem_bytes; x.recv_bytes[r] = plan.recv_counts[r] * elem_bytes; x.n_recv += plan.recv_counts[r];
    }
    return x;
}

// The layout of the gathered solid set: rank r's rows behind those of the ranks in front of it, as 8-byte key words and as
// 4-byte counts.
struct GatherLayout {
    std::vector<uint64_t> off8, len8, off4, len4;      // [world], bytes
    uint64_t n_total = 0;                              // rows
};
inline GatherLayout gather_layout(const std::vector<uint64_t> &rows_per_rank) {
    const size_t world = rows_per_rank.size();
    GatherLayout g;
    g.off8.resize(world); g.len8.resize(world); g.off4.resize(world); g.len4.resize(world);
    for (size_t r = 0; r < world; r++) {
        g.off8[r] = g.n_total * 8; g.len8[r] = rows_per_rank[r] * 8;
        g.off4[r] = g.n_total * 4; g.len4[r] = rows_per_rank[r] * 4;
        g.n_total += rows_per_rank[r];
    }
    return g;
}

// The words behind the histogram bins in the histogram all-reduce.  After it, the instances counted must equal the instances
// the reads hold: a record exchange that lost or duplicated data cannot pass unnoticed.
enum HistoTail : size_t {
    HT_COUNTED = 0,       // k-mer instances this rank counted in pass 2
    HT_FAILED = 1,        // 1: this rank failed
    HT_IN_READS = 2,      // k-mer instances this rank's READS hold
    HT_WORDS = 3
};
// tail: the reduced words, from HT_COUNTED on.  "", or the message of the mismatch
inline std::string instances_mismatch(const uint64_t *tail) {
    if (tail[HT_COUNTED] == tail[HT_IN_READS]) return std::string();
    return "shard_preprocess: the ranks counted " + std::to_string(tail[HT_COUNTED]) + " k-mer instances, their reads hold " +
           std::to_string(tail[HT_IN_READS]) + ": the record exchange lost or duplicated data";
}

}  // namespace shk
